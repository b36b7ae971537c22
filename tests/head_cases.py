"""The SAC-head matrix: case tables, data classes, fp64 references, error masses, fp32 yardsticks, the comparison rule and the defects.

Shared by tests/test_head_matrix_host.py (CPU: references, masses, yardsticks, defects and the tables are checked against themselves)
and tests/test_gpu_heads.py (the kernels of csrc/heads.hip against the reference).  Nothing here touches a GPU.

Families: "mlp" (mlp_head_fwd_kernel, mlp_head_bwd_kernel, head_dx_add_kernel and the grouped reduction behind them) and "tg"
(tanh_gaussian_fwd / bwd_kernel).

The rule.  An output element is measured as |got - ref64| / mass, the distance of a case and an output is the largest over its
elements; a NaN counts as infinite and an element of mass 0 must be reproduced exactly.  The mass is the first-order size of the
rounding error honest fp32 arithmetic can make at that element:
  * mlp: the same computation with every input, weight, bias and dy replaced by its absolute value and every computed factor by its
    mass, the reference's ReLU masks kept (mass(h1) = |x| |W1|^T + |b1|, g2 = m2 o sum_j |dy_j| |W3_j|, mass(dW2) = g2^T mass(h1), ...):
    every rounding of a sum of products is bounded by 2^-24 times this sum of absolute products, whatever the order of the sum.
  * tg: the formula of heads.hip restated op by op in fp64 with a factor (1 + delta_r) on the result of every fp32 operation (an fmaf,
    an expf, a tanhf, a logf are one operation each; the two rounded constants count too); mass = sum_r |d out / d delta_r| at
    delta = 0, by autograd.  For action and tanh_mean |bias| is added.  Where tanh saturates, 1 - y^2 is a few fp32 ulps against the
    1e-6: the mass grows with exactly that sensitivity, so saturated rows are held to the same few ulps as every other row.
The yardstick Y of a (family, output, class) is this distance for two honest fp32 evaluations on the CPU -- torch fp32, and a numpy
fp32 restatement (mlp: every dot product accumulated sequentially in k, the batch contractions sequentially in the row; tg: op by op)
-- maximised over both and over the admitted cases of the class.  Nothing in Y comes from the HIP side.  A kernel passes when its
distance is at most max(MARGIN * Y, ROW_FLOOR): MARGIN = 2 is the project's margin for another summation order, ROW_FLOOR = 8 * 2^-24
its floor for an element.  Every Y that enters a bound is at most Y_CAP = 16 * 2^-24; a shape at which the yardsticks themselves break
the cap is turned away by name (NOT_ADMITTED).  A ReLU mask is discontinuous: outside the `exact` class every fp64 pre-activation of
both layers is at least KINK = 64 * 2^-24 of its mass away from 0, twice the largest bound, so no honest evaluation flips a mask; the
generators walk a fixed seed sequence until that holds.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24
MARGIN = 2.0
ROW_FLOOR = 8 * U
Y_CAP = 16 * U
KINK = 64 * U
MAX_SEEDS = 50
INF = float("inf")


def bound(Y):
    return max(MARGIN * Y, ROW_FLOOR)


# ------------------------------------------------------------------------------------------------ branch predicates, restated
# csrc/small_mma.h, csrc/heads.hip, csrc/common.h, csrc/gemm_reduce.hip
HR = 32                 # rows of one workgroup
LB = 8                  # k-groups requested together
HMAXN = 128
HMAXK = 512
REDUCE_JOBS = 8         # DGVIT_REDUCE_JOBS
STAGE_FLOATS = 256 * 16  # floats one trip of stage_x moves
TG_BLOCK = 256


def w1_loader(K0, offs):
    """loader of W1 per tower (offs: byte offset of each tower's W1 from a 16-byte boundary): w1_vec() picks the kernel,
    mm_rows_x_wrows<false> the pair or the scalar form per tower"""
    if K0 % 4 == 0 and all(o % 16 == 0 for o in offs):
        return ("vec4",) * len(offs)
    return tuple("pair" if K0 % 2 == 0 and o % 8 == 0 else "scalar" for o in offs)


def kp(K0):
    return (K0 + 7) & ~7


def kgroups(K):
    return kp(K) // 8


def lb_trips(K):
    g = kgroups(K)
    return "one" if g <= LB else ("several" if g % LB == 0 else "ragged")


def dw1_clamped_lanes(K0):
    return kp(K0) % 32 != 0


def col_blocks(K0):
    return (K0 + 31) // 32


def stage_trips(kx):
    return -(-HR * kx // STAGE_FLOATS)


def nwg(B):
    return (B + HR - 1) // HR


def direct(B):
    return nwg(B) == 1


def last_rows(B):
    r = B - (nwg(B) - 1) * HR
    return "1" if r == 1 else ("32" if r == HR else "partial")


def reduce_form(n, off_floats):
    return "vector" if n % 4 == 0 and off_floats % 4 == 0 else "scalar"


def reduce_cw_log(n, slabs):
    return 4 if n // 4 <= 1024 and slabs >= 64 else 6


def tg_blocks(B):
    return (B + TG_BLOCK - 1) // TG_BLOCK


# ------------------------------------------------------------------------------------------------ mlp: case table
MLP_CLASSES = ("normal", "rowscale", "dead", "one_row", "exact")
MLP_KINDS = ("y", "h1", "h2", "dx", "dw1", "db1", "dw2", "db2", "dw3", "db3")
PARAM_KINDS = ("dw1", "db1", "dw2", "db2", "dw3", "db3", "dw3", "db3")

# name: the case's identity; pad[s] = ldx[s] - kx[s]; w1_off: byte offset of each tower's W1; x_off: floats the first input piece's base
# is off a 16-byte boundary; g_off: the same for every parameter-gradient output; nulls: NULL slots of the backward: "dy.t.j", "din.s",
# "dpar.t.i" (i indexes the tower's parameters W1 b1 W2 b2 W3_0 b3_0 W3_1 b3_1)
MlpCase = namedtuple("MlpCase", "name cls B ks pad n1 n2 n3 towers heads3 w1_off x_off g_off nulls")


def _c(name, B, ks, n1, n2, n3, towers, heads3, pad=None, w1_off=None, x_off=0, g_off=0, nulls=(), cls="normal"):
    return MlpCase(name, cls, B, tuple(ks), tuple(pad or (0,) * len(ks)), n1, n2, n3, towers, heads3, tuple(w1_off or (0,) * towers), x_off,
                   g_off, tuple(nulls))


# A large K0 goes with few rows and a narrow second layer: the chance that some pre-activation of B * n2 lands inside the kink margin
# grows with sqrt(n1 * K0), and the seed walk has to end within MAX_SEEDS.
MLP_SHAPES = (
    _c("k1", 1, (1,), 32, 64, 1, 1, 1),
    _c("k7_scalar", 31, (7,), 64, 32, 3, 1, 2, w1_off=(4,)),
    _c("k8_twin", 32, (8,), 32, 96, 2, 2, 1),
    _c("k8_off8", 33, (8,), 96, 32, 4, 1, 2, w1_off=(8,)),
    _c("k66_mixed", 64, (64, 2), 128, 32, 2, 2, 1, w1_off=(0, 4)),
    _c("k31", 65, (30, 1), 32, 128, 2, 1, 2, pad=(2, 0)),
    _c("k33_twin2", 97, (20, 12, 1), 32, 64, 4, 2, 2),
    _c("k64_policy", 32, (64,), 128, 128, 2, 1, 2),
    _c("k67_goff", 33, (64, 3), 64, 96, 3, 1, 2, pad=(5, 0), g_off=1),
    _c("k129", 31, (128, 1), 96, 64, 1, 1, 1, g_off=1),
    _c("k290_cnn", 33, (256, 32, 2), 128, 32, 2, 2, 1, pad=(3, 0, 1)),
    _c("k508", 31, (508,), 64, 32, 2, 1, 2),
    _c("k512", 33, (512,), 128, 32, 4, 1, 1),
    _c("k512_xoff", 1, (511, 1), 32, 128, 3, 1, 2, x_off=1, pad=(1, 0)),
    _c("k66_xoff", 65, (66,), 64, 32, 2, 1, 1, x_off=1, pad=(6,)),
    _c("widest", 2, (512,), 128, 128, 4, 2, 2),          # every width at its limit: the largest LDS image both kernels can ask for
    _c("b2049", 2049, (4,), 32, 32, 2, 1, 1),
)
_NULL_BASE = dict(ks=(20, 12, 1), n1=32, n2=64, n3=3, towers=2, heads3=2)
NULL_PATTERNS = {
    "dy01": ("dy.0.1",),
    "nodin": ("din.0", "din.1", "din.2"),
    "din1": ("din.1",),
    "dpar1": ("dpar.0.0",),
    "dparN": ("dpar.0.0", "dpar.0.2", "dpar.1.1", "dpar.1.5"),
}
MLP_NULL_CASES = tuple(_c(f"null_{k}_{'direct' if B == 31 else 'partial'}", B, nulls=v, **_NULL_BASE) for k, v in NULL_PATTERNS.items()
                       for B in (31, 65))
_CLASS_SHAPES = {
    "rowscale": ("k7_scalar", "k66_mixed", "k67_goff", "k290_cnn", "k512"),
    "dead": ("k8_twin", "k33_twin2", "k67_goff", "k31"),
    "one_row": ("k8_off8", "k66_mixed", "k33_twin2", "b2049"),
}
MLP_EXACT = (
    _c("ex_direct", 31, (7, 1), 32, 64, 3, 2, 2, w1_off=(4, 0), cls="exact"),
    _c("ex_partial", 64, (8,), 64, 32, 2, 1, 2, cls="exact"),
    _c("ex_33", 33, (30, 3), 32, 32, 4, 2, 1, pad=(2, 0), g_off=1, cls="exact"),
)
# through functional.mlp_head: a column slice as input, a loss on the first third layer only, a frozen bias, an input without gradient
WRAPPER_CASE = _c("wrapper", 33, (20, 5), 64, 32, 2, 1, 2, pad=(7, 0), nulls=("dy.0.1", "din.1", "dpar.0.1"))
H2_DEAD = "k31"          # the `dead` case in which every unit of h2 is dead

# shapes at which the CPU yardsticks themselves are further than Y_CAP from fp64 (test_head_matrix_host.py asserts that this is exactly
# the set turned away)
NOT_ADMITTED = frozenset()


def mlp_cases(cls):
    if cls == "normal":
        return MLP_SHAPES + MLP_NULL_CASES
    if cls == "exact":
        return MLP_EXACT
    by = {c.name: c for c in MLP_SHAPES}
    return tuple(by[n]._replace(cls=cls) for n in _CLASS_SHAPES[cls])


def all_mlp_cases():
    return tuple(c for cls in MLP_CLASSES for c in mlp_cases(cls))


def admitted(c):
    return (c.cls, c.name) not in NOT_ADMITTED


def K0_of(c):
    return sum(c.ks)


def param_shapes(c):
    K0 = K0_of(c)
    return [(c.n1, K0), (c.n1,), (c.n2, c.n1), (c.n2,)] + [(c.n3, c.n2), (c.n3,)] * c.heads3


def reduced_tensors(c):
    """(kind, n, form) of every tensor the partial path hands to the reduction, in its order"""
    out = []
    for t in range(c.towers):
        for i, s in enumerate(param_shapes(c)):
            if f"dpar.{t}.{i}" in c.nulls or (i >= 4 and f"dy.{t}.{(i - 4) // 2}" in c.nulls):
                continue
            n = int(np.prod(s))
            out.append((PARAM_KINDS[i], n, reduce_form(n, c.g_off)))
    return out


def reduce_flushes_midway(c):
    return not direct(c.B) and sum(f == "vector" for _, _, f in reduced_tensors(c)) > REDUCE_JOBS


def twin_dx1(c):
    return c.towers == 2 and any(f"din.{s}" not in c.nulls for s in range(len(c.ks)))


# ------------------------------------------------------------------------------------------------ mlp: data
def _rng(c, seed):
    name = "null_" + c.name.rsplit("_", 1)[1] if c.name.startswith("null_") else c.name      # every NULL pattern on the same data
    return np.random.RandomState((zlib.crc32(f"{name}/{c.cls}".encode()) + 7919 * seed) % (2 ** 31))


def _draw(c, seed):
    rs = _rng(c, seed)
    K0, B = K0_of(c), c.B
    if c.cls == "exact":
        sparse = lambda shape, p: (rs.randint(-1, 2, size=shape) * (rs.rand(*shape) < p)).astype(F32)
        x = rs.randint(-2, 3, size=(B, K0)).astype(F32)
        params = [[sparse((c.n1, K0), 0.6), rs.randint(-1, 2, size=c.n1).astype(F32), sparse((c.n2, c.n1), 0.25),
                   rs.randint(-2, 3, size=c.n2).astype(F32)]
                  + [p for _ in range(c.heads3) for p in (sparse((c.n3, c.n2), 0.7), rs.randint(-1, 2, size=c.n3).astype(F32))]
                  for _ in range(c.towers)]
        dy = [[rs.randint(-2, 3, size=(B, c.n3)).astype(F32) for _ in range(c.heads3)] for _ in range(c.towers)]
    else:
        x = rs.randn(B, K0)
        params = []
        for _ in range(c.towers):
            p = [rs.randn(c.n1, K0) / K0 ** 0.5, rs.randn(c.n1) * 0.1, rs.randn(c.n2, c.n1) / c.n1 ** 0.5, rs.randn(c.n2) * 0.1]
            for _ in range(c.heads3):
                p += [rs.randn(c.n3, c.n2) / c.n2 ** 0.5, rs.randn(c.n3) * 0.1]
            params.append(p)
        dy = [[rs.randn(B, c.n3) for _ in range(c.heads3)] for _ in range(c.towers)]
        if c.cls == "rowscale":
            x *= 10.0 ** rs.uniform(-3, 3, size=(B, 1))
            for p in params:
                for i in (0, 2):
                    p[i] *= 30.0 ** rs.uniform(0, 1, size=(p[i].shape[0], 1))
                for i in range(4, len(p), 2):
                    p[i] *= 30.0 ** rs.uniform(0, 1)
        if c.cls == "dead":
            # a kill-switch input column: 0 in live rows, 1 in the dead rows, weight -10 into every unit of layer 1
            x[:, K0 - 1] = 0.0
            x[3::16, K0 - 1] = 1.0
            for p in params:
                p[0][:, K0 - 1] = -10.0
                p[1][::5] = -10.0                  # whole units of layer 1 dead
                p[3][1::7] = -10.0                 # and of layer 2
                if c.name == H2_DEAD:
                    p[3][:] = -10.0
        if c.cls == "one_row":
            for t in range(c.towers):
                for j in range(c.heads3):
                    keep = np.zeros((B, 1))
                    for blk in range(nwg(B)):
                        rows = min(HR, B - blk * HR)
                        keep[blk * HR + (7 * blk + 5) % rows] = 1.0
                    dy[t][j] = dy[t][j] * keep
    cut, xs = np.cumsum((0,) + c.ks), []
    for s in range(len(c.ks)):
        xs.append(np.ascontiguousarray(x[:, cut[s]:cut[s + 1]], dtype=F32))
    return {"x": xs, "params": [[np.ascontiguousarray(q, dtype=F32) for q in p] for p in params],
            "dy": [[np.ascontiguousarray(d, dtype=F32) for d in r] for r in dy]}


@functools.lru_cache(maxsize=None)
def _mlp_inputs(c):
    for seed in range(MAX_SEEDS + 50):
        inp = _draw(c, seed)
        if c.cls == "exact":
            if min(exact_kink_count(c, inp)) >= 1:
                return inp, seed + 1
        elif kink_ratio(c, inp) >= KINK:
            return inp, seed + 1
    raise AssertionError(f"{c.name}/{c.cls}: no admissible draw")


def mlp_inputs(c):
    """the case's fp32 inputs: x (one array per piece), params (per tower W1 b1 W2 b2 then W3 b3 per third layer), dy[t][j].  A NULL dy of
    the case is still drawn (the `null_dy_contributes` defect needs it); the reference takes it as zero."""
    return _mlp_inputs(c._replace(pad=(0,) * len(c.ks), w1_off=(0,) * c.towers, x_off=0, g_off=0, nulls=()))[0]


def seeds_walked(c):
    return _mlp_inputs(c._replace(pad=(0,) * len(c.ks), w1_off=(0,) * c.towers, x_off=0, g_off=0, nulls=()))[1]


# ------------------------------------------------------------------------------------------------ mlp: evaluation
class Np64:
    dtype = np.float64
    mm = staticmethod(lambda a, b: a @ b)
    colsum = staticmethod(lambda a: a.sum(0))


class Torch32:
    dtype = F32

    @staticmethod
    def mm(a, b):
        return (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b))).numpy()

    @staticmethod
    def colsum(a):
        return torch.from_numpy(np.ascontiguousarray(a)).sum(0).numpy()


class Seq32:
    """numpy fp32, every dot product accumulated sequentially along the contraction"""
    dtype = F32

    @staticmethod
    def mm(a, b):
        acc = np.zeros((a.shape[0], b.shape[1]), F32)
        for k in range(a.shape[1]):
            acc += a[:, k:k + 1] * b[k:k + 1, :]
        return acc

    @staticmethod
    def colsum(a):
        acc = np.zeros(a.shape[1], F32)
        for r in range(a.shape[0]):
            acc += a[r]
        return acc


MLP_DEFECTS = ("drop_k8", "drop_k4", "pad_rows", "mask_ge", "no_tower1_dx", "no_second_head", "last_slab_missing", "piece_off_by_one",
               "ldx_as_kx", "db1_last_row", "null_dy_contributes")


def defect_applies(d, c):
    K0 = K0_of(c)
    return {"drop_k8": K0 % 8 != 0, "drop_k4": K0 % 4 != 0, "pad_rows": c.B % HR != 0, "mask_ge": c.cls == "exact",
            "no_tower1_dx": twin_dx1(c), "no_second_head": c.heads3 == 2 and not any(n.startswith("dy.") for n in c.nulls),
            "last_slab_missing": not direct(c.B), "piece_off_by_one": len(c.ks) > 1 and "din.0" not in c.nulls and "din.1" not in c.nulls,
            "ldx_as_kx": any(c.pad) and c.B > 1, "db1_last_row": True,
            "null_dy_contributes": any(n.startswith("dy.") for n in c.nulls)}[d]


def padded_input(c, inp, s):
    """piece s as the kernel gets it: rows ldx floats apart, NaN between kx and ldx; flat, ends with the last row's last element"""
    x = inp["x"][s]
    buf = np.full((c.B, c.ks[s] + c.pad[s]), np.nan, F32)
    buf[:, :c.ks[s]] = x
    return buf.reshape(-1)[:(c.B - 1) * (c.ks[s] + c.pad[s]) + c.ks[s]]


def mlp_eval(c, inp, be, mass=False, masks=None, defect=None):
    """-> (outputs by name, the ReLU masks per tower, the pre-activations per tower).  Names: y.t.j h1.t h2.t dx.s dw1.t db1.t dw2.t db2.t
    dw3.t.j db3.t.j; what a NULL slot of the case leaves unwritten is absent.  mass=True: the absolute-value network under `masks`."""
    dt = be.dtype
    A = np.abs if mass else (lambda v: v)
    xs = [A(x.astype(dt)) for x in inp["x"]]
    if defect == "ldx_as_kx":
        xs = [padded_input(c, inp, s)[:c.B * k].reshape(c.B, k).astype(dt) if c.pad[s] else xs[s] for s, k in enumerate(c.ks)]
    x = np.concatenate(xs, 1)
    K0, B = x.shape[1], c.B
    if defect in ("drop_k8", "drop_k4"):
        x = x.copy()
        x[:, K0 - K0 % (8 if defect == "drop_k8" else 4):] = 0
    rows = (nwg(B) - 1) * HR if defect == "last_slab_missing" else B          # rows that reach the parameter gradients
    out, mk, pre, dxs = {}, [], [], []
    for t in range(c.towers):
        p = [A(q.astype(dt)) for q in inp["params"][t]]
        W1, b1, W2, b2 = p[:4]
        a1 = be.mm(x, W1.T) + b1
        h1 = a1 if mass else np.maximum(a1, 0)
        a2 = be.mm(h1, W2.T) + b2
        h2 = a2 if mass else np.maximum(a2, 0)
        if masks is not None:
            m1, m2 = masks[t]
        elif defect == "mask_ge":
            m1, m2 = a1 >= 0, a2 >= 0
        else:
            m1, m2 = a1 > 0, a2 > 0
        mk.append((m1, m2))
        pre.append((a1, a2))
        out[f"h1.{t}"], out[f"h2.{t}"] = h1, h2
        g2 = np.zeros((B, c.n2), dt)
        for j in range(c.heads3):
            W3, b3 = p[4 + 2 * j], p[5 + 2 * j]
            out[f"y.{t}.{j}"] = be.mm(h2, W3.T) + b3
            dyj = A(inp["dy"][t][j].astype(dt))
            if f"dy.{t}.{j}" in c.nulls:
                if defect == "null_dy_contributes":
                    g2 = g2 + be.mm(dyj, W3)
                continue
            if not (defect == "no_second_head" and j == 1):
                g2 = g2 + be.mm(dyj, W3)
            out[f"dw3.{t}.{j}"] = be.mm(dyj[:rows].T, h2[:rows])
            out[f"db3.{t}.{j}"] = be.colsum(dyj[:rows])
        g2 = np.where(m2, g2, 0).astype(dt)
        g1 = np.where(m1, be.mm(g2, W2), 0).astype(dt)
        out[f"dw2.{t}"] = be.mm(g2[:rows].T, h1[:rows])
        out[f"db2.{t}"] = be.colsum(g2[:rows])
        if defect == "pad_rows":             # the rows behind the batch: h1 = relu(b1), dh2 that of the (clamped) last row
            npad = nwg(B) * HR - B
            out[f"dw2.{t}"] = out[f"dw2.{t}"] + dt(npad) * np.outer(g2[B - 1], np.maximum(b1, 0)).astype(dt)
            out[f"db2.{t}"] = out[f"db2.{t}"] + dt(npad) * g2[B - 1]
        out[f"dw1.{t}"] = be.mm(g1[:rows].T, x[:rows])
        out[f"db1.{t}"] = be.colsum(g1[:rows - 1] if defect == "db1_last_row" else g1[:rows])
        dxs.append(be.mm(g1, W1))
    dx = dxs[0]
    if c.towers == 2 and defect != "no_tower1_dx":
        dx = dx + dxs[1]
    cut = np.cumsum((0,) + c.ks)
    if defect == "piece_off_by_one":       # the first boundary one column late: piece 1 starts with what belongs to its column 1
        dx = dx.copy()
        dx[:, cut[1]:cut[2] - 1] = dx[:, cut[1] + 1:cut[2]]
        dx[:, cut[2] - 1] = 0
    for s in range(len(c.ks)):
        if f"din.{s}" not in c.nulls:
            out[f"dx.{s}"] = np.ascontiguousarray(dx[:, cut[s]:cut[s + 1]])
    for t in range(c.towers):
        for i, kind in enumerate(PARAM_KINDS[:4 + 2 * c.heads3]):
            if f"dpar.{t}.{i}" in c.nulls:
                out.pop(f"{kind}.{t}" if i < 4 else f"{kind}.{t}.{(i - 4) // 2}", None)
    return out, mk, pre


def kink_ratio(c, inp):
    """smallest |pre-activation| / mass over both layers and every tower, in fp64"""
    _, mk, pre = mlp_eval(c, inp, Np64)
    _, _, mpre = mlp_eval(c, inp, Np64, mass=True, masks=mk)
    live = np.ones(c.B, bool)
    if c.cls == "dead":       # a dead row's h1 is exactly 0 in any arithmetic, so its layer-2 pre-activation is b2 itself: no rounding, no flip
        live = inp["x"][-1][:, -1] == 0
    return min(float((np.abs(a[live]) / m[live]).min()) for t in range(c.towers) for a, m in zip(pre[t], mpre[t]))


def exact_kink_count(c, inp):
    """per layer, the pre-activations that are exactly 0 and carry a non-zero upstream gradient (any tower)"""
    n1 = n2 = 0
    for t in range(c.towers):
        p = [q.astype(np.float64) for q in inp["params"][t]]
        x = np.concatenate(inp["x"], 1).astype(np.float64)
        a1 = x @ p[0].T + p[1]
        a2 = np.maximum(a1, 0) @ p[2].T + p[3]
        up2 = sum(inp["dy"][t][j].astype(np.float64) @ p[4 + 2 * j] for j in range(c.heads3))
        up1 = np.where(a2 > 0, up2, 0) @ p[2]
        n2 += int(((a2 == 0) & (up2 != 0)).sum())
        n1 += int(((a1 == 0) & (up1 != 0)).sum())
    return n1, n2


@functools.lru_cache(maxsize=None)
def mlp_reference(c):
    """(fp64 outputs, masses) by output name"""
    inp = mlp_inputs(c)
    ref, mk, _ = mlp_eval(c, inp, Np64)
    mass, _, _ = mlp_eval(c, inp, Np64, mass=True, masks=mk)
    return ref, mass


def exact_mass_max(c):
    return max(float(m.max()) for m in mlp_reference(c)[1].values())


def element_distance(got, ref, mass):
    got = np.asarray(got, np.float64)
    if got.shape != ref.shape:
        return INF
    err = np.abs(got - ref)
    if np.isnan(err).any() or (err[mass == 0] != 0).any():
        return INF
    nz = mass > 0
    return float((err[nz] / mass[nz]).max()) if nz.any() else 0.0


def kind_of(name):
    return name.split(".")[0]


def _by_kind(ref, mass, got):
    d = {}
    assert set(got) == set(ref), f"outputs {sorted(set(got) ^ set(ref))} differ from the reference's"
    for k in ref:
        d[kind_of(k)] = max(d.get(kind_of(k), 0.0), element_distance(got[k], ref[k], mass[k]))
    return d


@functools.lru_cache(maxsize=None)
def _mlp_yardstick_case(c):
    inp = mlp_inputs(c)
    ref, mass = mlp_reference(c)
    d = {}
    for be in (Torch32, Seq32):
        for k, v in _by_kind(ref, mass, mlp_eval(c, inp, be)[0]).items():
            d[k] = max(d.get(k, 0.0), v)
    return d


# ------------------------------------------------------------------------------------------------ tanh-Gaussian
TG_CLASSES = ("normal", "shoulder", "saturated", "deep", "tiny_scale", "clamp_edges", "zero_eps")
TG_KINDS = ("action", "tanh_mean", "log_prob", "dmean", "dlog_std")
TG_LO, TG_HI = -20.0, 2.0
HALF_LOG_2PI = 0.91893853320467274178
TG_EPSILON = 1e-6
# ups: which upstream gradients are given (d_action, d_log_prob, d_tanh_mean)
TgCase = namedtuple("TgCase", "cls B A scale_n ups")
_ALL_UPS = tuple((bool(m & 1), bool(m & 2), bool(m & 4)) for m in range(1, 8))
_TG_SHAPES = ((1, 1, 1), (255, 2, 1), (256, 3, 3), (257, 16, 16), (600, 2, 2), (257, 16, 1), (600, 1, 1))


def tg_cases(cls):
    out = [TgCase(cls, B, A, sn, _ALL_UPS[(6 + i) % 7]) for i, (B, A, sn) in enumerate(_TG_SHAPES)]
    out += [TgCase(cls, 257, 3, 3, u) for u in _ALL_UPS]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def tg_inputs(c):
    rs = np.random.RandomState(zlib.crc32(repr(c).encode()) % (2 ** 31))
    B, A = c.B, c.A
    mean, raw, eps = rs.randn(B, A), rs.randn(B, A) * 3 - 1, rs.randn(B, A)
    scale = np.array([1.0]) if c.scale_n == 1 else rs.rand(A) + 0.5
    sign = np.where(rs.rand(B, A) < 0.5, -1.0, 1.0)
    if c.cls == "shoulder":
        mean *= 4
    elif c.cls == "saturated":
        mean, raw = sign * rs.uniform(6, 10, size=(B, A)), rs.randn(B, A) - 1
    elif c.cls == "deep":
        mean, raw = sign * rs.uniform(12, 20, size=(B, A)), rs.randn(B, A) - 1
    elif c.cls == "tiny_scale":
        scale = np.array([1e-3]) if c.scale_n == 1 else np.where(np.arange(A) % 2 == 0, 1e-3, 1e-5)
    elif c.cls == "clamp_edges":
        lo, hi = F32(TG_LO), F32(TG_HI)
        edge = np.array([lo, hi, np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf)), lo - 30, hi + 5], F32)
        raw = np.where(rs.rand(B, A) < 0.2, raw, edge[(np.arange(B * A).reshape(B, A) + rs.randint(6)) % 6])
    elif c.cls == "zero_eps":
        eps = np.zeros((B, A))
    f = lambda a: np.ascontiguousarray(a, dtype=F32)
    i = {"mean": f(mean), "raw": f(raw), "eps": f(eps), "scale": f(scale), "bias": f(rs.randn(c.scale_n)), "lo": TG_LO, "hi": TG_HI,
         "d_action": f(rs.randn(B, A)) if c.ups[0] else None, "d_log_prob": f(rs.randn(B)) if c.ups[1] else None,
         "d_tanh_mean": f(rs.randn(B, A)) if c.ups[2] else None}
    return i


class _Pert:
    """v -> v (1 + delta) with delta a zero leaf: the rounding of one fp32 operation"""

    def __init__(self, on):
        self.on, self.leaves = on, []

    def __call__(self, v):
        if not self.on:
            return v
        d = torch.zeros_like(v, requires_grad=True)
        self.leaves.append(d)
        return v * (1 + d)


def _tt(i, c, dtype):
    t = lambda a: None if a is None else torch.from_numpy(a).to(dtype)
    sc, bi = t(i["scale"]).expand(c.A), t(i["bias"]).expand(c.A)
    return t(i["mean"]), t(i["raw"]), t(i["eps"]), sc, bi, t(i["d_action"]), t(i["d_log_prob"]), t(i["d_tanh_mean"])


def tg_formula(c, i, perturbed, dtype=torch.float64):
    """tanh_gaussian_fwd_kernel and tanh_gaussian_bwd_kernel op by op in torch -> ({output: tensor}, {output: the leaves it depends on})"""
    m, raw, e, sc, bi, dact, dlp, dtm = _tt(i, c, dtype)
    lo, hi = i["lo"], i["hi"]
    ls = raw.clamp(lo, hi)
    const = lambda r, v: r(torch.full_like(m, v))
    out, leaves = {}, {}
    # forward
    r = _Pert(perturbed)
    y = r(torch.tanh(r(r(torch.exp(ls)) * e + m)))
    out["action"] = r(y * sc + bi)
    n_act = len(r.leaves)
    r2 = _Pert(perturbed)
    out["tanh_mean"] = r2(r2(torch.tanh(m)) * sc + bi)
    t = r(r(r((-0.5 * e) * e) - ls) - const(r, HALF_LOG_2PI))
    t = r(t - r(torch.log(r(sc * r(1 - r(y * y)) + const(r, TG_EPSILON)))))
    lp = t[:, 0]
    for a in range(1, c.A):
        lp = r(lp + t[:, a])
    out["log_prob"] = lp
    leaves.update(action=r.leaves[:n_act], tanh_mean=r2.leaves, log_prob=r.leaves)
    # backward
    r = _Pert(perturbed)
    sd = r(torch.exp(ls))
    y = r(torch.tanh(r(sd * e + m)))
    omy = r(1 - r(y * y))
    dx = torch.zeros_like(m)
    if dact is not None:
        dx = r(r(dact * sc) * omy)
    if dlp is not None:
        gl = dlp[:, None].expand_as(m)
        q = r(r(r(r((gl * 2) * y) * sc) * omy) / r(sc * omy + const(r, TG_EPSILON)))
        dx = r(dx + q) if dact is not None else q
    n_dx = len(r.leaves)
    dmean = dx
    if dtm is not None:
        tm = r(torch.tanh(m))
        dmean = r(dx + r(r(dtm * sc) * r(1 - r(tm * tm))))
    out["dmean"] = dmean
    n_dm = len(r.leaves)
    g = r(r(dx * sd) * e)
    if dlp is not None:
        g = r(g - gl)
    out["dlog_std"] = torch.where((raw >= lo) & (raw <= hi), g, torch.zeros_like(g))
    leaves.update(dmean=r.leaves[:n_dm], dlog_std=r.leaves[:n_dx] + r.leaves[n_dm:])
    return out, leaves


@functools.lru_cache(maxsize=None)
def tg_reference(c):
    """(fp64 outputs, masses) by output name, as numpy"""
    i = tg_inputs(c)
    ref = {k: v.numpy() for k, v in tg_formula(c, i, False)[0].items()}
    out, leaves = tg_formula(c, i, True)
    mass = {}
    for k, o in out.items():
        ms = torch.zeros_like(o)
        if o.requires_grad:
            for g in torch.autograd.grad(o.sum(), leaves[k], allow_unused=True, retain_graph=True):
                if g is None:
                    continue
                ms = ms + (g.abs() if g.shape == o.shape else g.abs().sum(1))
        if k in ("action", "tanh_mean"):
            ms = ms + torch.from_numpy(i["bias"]).double().abs().expand(c.A)
        mass[k] = ms.numpy()
    return ref, mass


def tg_autograd(c, i, dtype, dist=False):
    """the reference's own op sequence (torch clamp / exp / tanh / log) under autograd, as tests/test_gpu_round2.py has it.  dist=True takes
    the Gaussian term from torch.distributions.Normal as the reference does, ((x - mean) / std)^2 / 2 recovered from x; dist=False
    takes it as eps^2 / 2, which is what x = mean + std * eps makes it.  Recovering eps from x cancels: the error is ulp(mean) / std, and
    std goes down to e^-20, so only dist=False is an honest evaluation of the function at every log_std."""
    t = lambda a: None if a is None else torch.from_numpy(a).to(dtype)
    m, raw = t(i["mean"]).requires_grad_(True), t(i["raw"]).requires_grad_(True)
    e, sc, bi = t(i["eps"]), t(i["scale"]), t(i["bias"])
    ls = torch.clamp(raw, min=i["lo"], max=i["hi"])
    normal = torch.distributions.Normal(m, ls.exp())
    x_t = m + ls.exp() * e
    y_t = torch.tanh(x_t)
    act = y_t * sc + bi
    gauss = normal.log_prob(x_t) if dist else -0.5 * e * e - ls - HALF_LOG_2PI
    lp = (gauss - torch.log(sc * (1 - y_t.pow(2)) + TG_EPSILON)).sum(1)
    tm = torch.tanh(m) * sc + bi
    loss = 0
    for o, w in ((act, i["d_action"]), (lp, i["d_log_prob"]), (tm, i["d_tanh_mean"])):
        if w is not None:
            loss = loss + (o * t(w)).sum()
    loss.backward()
    return {"action": act.detach().numpy(), "tanh_mean": tm.detach().numpy(), "log_prob": lp.detach().numpy(), "dmean": m.grad.numpy(),
            "dlog_std": (torch.zeros_like(raw) if raw.grad is None else raw.grad).numpy()}


def tg_torch32(c, i):
    """the kernels' op sequence in torch fp32.  (torch *autograd* in fp32 is no yardstick for dmean: its tanh backward rounds 1 - y^2 in one
    step where the forward's y.pow(2) rounds twice, the two meet as numerator and denominator of omy / (scale * omy + 1e-6), and the
    cancellation the kernel keeps by using one omy is lost: up to 150 * 2^-24 of the mass on the shoulder of the tanh.)"""
    return {k: v.numpy() for k, v in tg_formula(c, i, False, torch.float32)[0].items()}


TG_DEFECTS = ("no_epsilon", "log_scale_outside", "clamp_pass_outside", "clamp_block_on_bounds", "no_minus_gl", "scale_scalar")


def tg_defect_applies(d, c):
    return {"no_epsilon": True, "log_scale_outside": c.cls == "tiny_scale", "clamp_pass_outside": c.cls in ("normal", "clamp_edges"),
            "clamp_block_on_bounds": c.cls == "clamp_edges", "no_minus_gl": c.ups[1], "scale_scalar": c.scale_n == c.A and c.A > 1}[d]


def tg_numpy32(c, i, defect=None):
    """the two kernels op by op in numpy fp32"""
    one, two, half = F32(1), F32(2), F32(0.5)
    m, raw, e = i["mean"], i["raw"], i["eps"]
    sc = np.broadcast_to(i["scale"][:1] if defect == "scale_scalar" else i["scale"], (c.A,))
    bi = np.broadcast_to(i["bias"], (c.A,))
    lo, hi, k6, kh = F32(i["lo"]), F32(i["hi"]), F32(TG_EPSILON), F32(HALF_LOG_2PI)
    with np.errstate(all="ignore"):
        ls = np.minimum(np.maximum(raw, lo), hi)
        sd = np.exp(ls)
        y = np.tanh(sd * e + m)
        omy = one - y * y
        out = {"action": y * sc + bi, "tanh_mean": np.tanh(m) * sc + bi}
        if defect == "no_epsilon":
            lg = np.log(sc * omy)
        elif defect == "log_scale_outside":
            lg = np.log(sc) + np.log(omy + k6)
        else:
            lg = np.log(sc * omy + k6)
        t = -half * e * e - ls - kh - lg
        lp = t[:, 0].copy()
        for a in range(1, c.A):
            lp = lp + t[:, a]
        out["log_prob"] = lp
        dx = np.zeros_like(m)
        gl = None if i["d_log_prob"] is None else np.broadcast_to(i["d_log_prob"][:, None], m.shape)
        if i["d_action"] is not None:
            dx = i["d_action"] * sc * omy
        if gl is not None:
            dx = dx + gl * two * y * sc * omy / (sc * omy + k6)
        dmean = dx
        if i["d_tanh_mean"] is not None:
            tm = np.tanh(m)
            dmean = dx + i["d_tanh_mean"] * sc * (one - tm * tm)
        g = dx * sd * e
        if gl is not None and defect != "no_minus_gl":
            g = g - gl
        inside = (raw > lo) & (raw < hi) if defect == "clamp_block_on_bounds" else (raw >= lo) & (raw <= hi)
        out["dmean"] = dmean
        out["dlog_std"] = g if defect == "clamp_pass_outside" else np.where(inside, g, F32(0))
    assert all(v.dtype == F32 for v in out.values())
    return out


@functools.lru_cache(maxsize=None)
def _tg_yardstick_case(c):
    i = tg_inputs(c)
    ref, mass = tg_reference(c)
    d = {}
    for got in (tg_torch32(c, i), tg_numpy32(c, i)):
        for k in ref:
            d[k] = max(d.get(k, 0.0), element_distance(got[k], ref[k], mass[k]))
    return d


# ------------------------------------------------------------------------------------------------ the rule
def cases(fam, cls):
    return mlp_cases(cls) if fam == "mlp" else tg_cases(cls)


def yardstick_case(fam, c):
    return _mlp_yardstick_case(c) if fam == "mlp" else _tg_yardstick_case(c)


@functools.lru_cache(maxsize=None)
def yardsticks(fam, cls):
    """{output kind: Y} over the admitted cases of the class"""
    Y = {}
    for c in cases(fam, cls):
        if fam == "tg" or admitted(c):
            for k, v in yardstick_case(fam, c).items():
                Y[k] = max(Y.get(k, 0.0), v)
    return Y


def distances(fam, c, got):
    """{output kind: distance of `got` (outputs by name) to the fp64 reference}"""
    ref, mass = mlp_reference(c) if fam == "mlp" else tg_reference(c)
    if fam == "mlp":
        return _by_kind(ref, mass, got)
    return {k: element_distance(got[k], ref[k], mass[k]) for k in ref}


def violations(fam, c, got):
    Y = yardsticks(fam, c.cls)
    return [(k, v, bound(Y[k])) for k, v in distances(fam, c, got).items() if not v <= bound(Y[k])]
