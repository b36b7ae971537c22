"""The row-kernel matrix: case tables, row generators, fp64 references, fp32 yardsticks, the comparison rule and the defects.

Shared by tests/test_row_kernel_matrix_host.py (CPU: reference, yardsticks, defects and the table are checked against themselves) and
tests/test_gpu_row_kernels.py (the kernels of csrc/norm.hip and csrc/misc_bf16.hip against the reference).  Nothing here touches a GPU.

Families: "ln" (fp32 LayerNorm forward + backward), "lnb_fwd" / "lnb_bwd" (the bf16 configuration's LayerNorm), "rms" (RMSNorm forward +
backward), "colsum" (fp32 column sums).  residual_add_bf16 and transpose_cast_f32_bf16 are exact operations: their cases are here, their
reference is torch itself.

The rule.  A ROW output (y, dx, mean, rstd) is measured per row as max |got - ref64| over the row divided by the row's max |ref64|
(a NaN counts as infinite; a row whose reference is all zero must be reproduced exactly); the distance of a case is the largest over
its rows.  Two exceptions to the divisor: `mean` is a single number that may lie arbitrarily close to zero, so it is divided by the row's
max |x|, the scale its rounding error has; and the RMSNorm dx of a one-element row (D = 1) is zero by cancellation (u - xh (u . xh)
with xh = +-1), so it is divided by |u| / n, the size of the terms that cancel.
A COLUMN SUM (dgamma, dbeta, dg, colsum) is measured as max |err| over the columns divided by the largest column's sum over t of
|summand64|; where every summand is exactly zero (dgamma of constant rows) the divisor is the largest
sum over t of |dy|.
The yardstick Y of a (family, output, row class) is the same distance, for two honest fp32 evaluations on the CPU -- torch fp32, and the
kernel's two-pass algorithm restated in numpy fp32 -- maximised over both and over every case of the class.  Nothing in Y comes from the
HIP side.  A kernel passes a case when its distance is at most max(MARGIN * Y, floor): MARGIN = 2 is the project's margin for the same
arithmetic in another summation order, the floor counts roundings: 8 * 2^-24 for an element of a row output (subtract, scale, multiply,
add and the rounding of each of the two statistics they use), (T + 8) * 2^-24 for a sum of T terms.  A bf16 output may in addition be half
a bf16 ulp of the reference away (`slack`).  Rows are admitted only where honest fp32 arithmetic is within Y_CAP = 1e-4 of fp64: data on
which fp32 itself is that far off tests nothing.  Every class meets the cap at all but four of its shapes; admitted() turns those four
away (NOT_ADMITTED), so every Y that enters a bound is at most Y_CAP.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

F32 = np.float32
U = 2.0 ** -24
MARGIN = 2.0
ROW_FLOOR = 8 * U
Y_CAP = 1e-4
EPS_LN = float(F32(1e-5))
EPS_RMS = float(F32(1e-12))


def sum_floor(T):
    return (T + 8) * U


def bound(Y, floor):
    return max(MARGIN * Y, floor)


# ------------------------------------------------------------------------------------------------ branch predicates, restated
# csrc/norm.hip
def ln_nch(D):                      # template parameter of layernorm_bwd_kernel / layernorm_fwd_bf16_kernel: 256-column chunks per row
    return (D + 255) // 256


def ln_last_chunk_lanes(D):         # lanes of the last chunk that hold columns (a lane owns four)
    return (D - (ln_nch(D) - 1) * 256 + 3) // 4


def ln_bwd_blocks_f32(T):           # layernorm_bwd_blocks_f32
    return (T + 3) // 4 if T < 2048 else 512


def ln_bwd_blocks_bf16(T):          # layernorm_bwd_blocks
    return (T + 3) // 4 if T < 2048 else (512 if T < 16384 else 2048)


def ln_bwd_grid_strides(T, blocks):  # some wave of the backward takes a second row
    return T > 4 * blocks


def ln_bwd_accepts(D):
    return D > 0 and D % 4 == 0 and D <= 1024


def rms_bwd_blocks(B):              # rmsnorm_bwd_blocks
    return (B + 3) // 4 if B < 256 else 64


def rms_bwd_accepts(D):
    return 0 < D <= 4096


def colsum_blocks(T):               # colsum_blocks
    return 1 if T < 64 else (16 if T < 16384 else 64)


def colsum_bf16_blocks(T):          # csrc/misc_bf16.hip; reached through op_wgrad_bf16 (tests/test_gpu_bf16.py::test_wgrad_bf16)
    return 1 if T < 4096 else (64 if T < 16384 else 256)


def colsum_row(t, rgrp, plus_one=True):
    """physical row of logical row t: t, or t + t / rgrp + 1 (frames of rgrp + 1 tokens, token 0 skipped)"""
    return t if rgrp <= 0 else t + t // rgrp + (1 if plus_one else 0)


def colsum_phys_rows(T, rgrp):
    return colsum_row(T - 1, rgrp) + 1


def colsum_takes_vec(c):            # colsum(): colsum4_kernel or colsum_kernel (the scratch is always 16-byte aligned)
    return c.N % 4 == 0 and c.lda % 4 == 0 and c.off % 4 == 0


def colsum4_trips(T):
    """(full, ragged) trips of one thread's eight-row loop in colsum4_kernel, over all threads: a trip loads rows t0 + j * step,
    j < 8, step = 4 * blocks; it is ragged when some of them are past T (clamped load, factor 0)."""
    step = 4 * colsum_blocks(T)
    full = ragged = 0
    for first in range(min(step, T)):
        for t0 in range(first, T, 8 * step):
            if t0 + 7 * step < T:
                full += 1
            else:
                ragged += 1
    return full, ragged


# ------------------------------------------------------------------------------------------------ case tables
LN_D = (4, 32, 252, 256, 260, 516, 768, 772, 1024)
LN_D_FWD_ONLY = 1028                 # the forward takes any multiple of 4; the backward keeps a row in registers and refuses it
LN_CLASSES = ("normal", "offset", "tight", "spike", "scaled", "const")
RMS_CLASSES = ("normal", "zero_rows", "tiny", "scaled", "spike", "huge")
RMS_B = (1, 3, 255, 259)
RMS_D = (1, 3, 63, 65, 256, 768, 4096)

LnCase = namedtuple("LnCase", "cls T D rs")
LnbFwdCase = namedtuple("LnbFwdCase", "cls T D rs variant")
LnbBwdCase = namedtuple("LnbBwdCase", "cls T D rs")
RmsCase = namedtuple("RmsCase", "cls B D")
ColCase = namedtuple("ColCase", "T N lda off rgrp")

# variants of the bf16 LayerNorm forward -> (number of branch outputs added, xout given, mean / rstd given); the dispatch of
# dgvit_diag_layernorm_forward_bf16 (= encoder_bf16.hip): "plain*" layernorm_fwd_bf16 (ADD 0); "add" add_layernorm_fwd_bf16 (ADD 1);
# "add_noxout" / "add2*" add2_layernorm_fwd_bf16 (ADD 1 with xout NULL / ADD 2), contiguous rows only
LNB_VARIANTS = {"plain": (0, False, True), "plain_nostat": (0, False, False), "add": (1, True, True), "add_noxout": (1, False, False),
                "add2": (2, True, False), "add2_noxout": (2, False, False)}
LNB_STRIDED = ("plain", "add")


def lnb_add(variant):               # the ADD template parameter the variant reaches
    return LNB_VARIANTS[variant][0]


@functools.lru_cache(maxsize=None)
def ln_cases(cls):
    """fp32 LayerNorm: every D at T = 5 (two workgroups, the second ragged) contiguous and strided; the backward's block counts at
    T = 1, 2047 (the last T without a grid-stride loop), 2051 (512 workgroups, three of their waves take a second row) for one-chunk
    and ragged two-chunk rows."""
    out = [LnCase(cls, 5, D, rs) for D in LN_D for rs in (1, 5)]
    out += [LnCase(cls, T, D, 1) for T in (1, 2047, 2051) for D in (32, 260)]
    out.append(LnCase(cls, 2051, 32, 5))
    return out


@functools.lru_cache(maxsize=None)
def lnb_fwd_cases(cls):
    out = []
    for D in LN_D:
        for v in LNB_VARIANTS:
            out.append(LnbFwdCase(cls, 5, D, 1, v))
            if v in LNB_STRIDED:
                out.append(LnbFwdCase(cls, 5, D, 5, v))
    return out


@functools.lru_cache(maxsize=None)
def lnb_bwd_cases(cls):
    """bf16 LayerNorm backward: every D at T = 5; the three block counts (T = 5, 2051, 16387) at D = 64"""
    out = [LnbBwdCase(cls, 5, D, rs) for D in LN_D for rs in (1, 5)]
    out += [LnbBwdCase(cls, T, 64, 1) for T in (2051, 16387)]
    return out


@functools.lru_cache(maxsize=None)
def rms_cases(cls):
    return [RmsCase(cls, B, D) for B in RMS_B for D in RMS_D]


COL_T = (1, 63, 64, 515, 16387)
# (N, lda, offset of the base pointer in floats): the vector kernel dense and padded; the scalar kernel for N = 7 with a dense (odd) and
# a padded odd lda, and for a vector-shaped matrix whose base is one float past 16-byte alignment
COL_SHAPES = ((256, 256, 0), (256, 260, 0), (7, 7, 0), (7, 9, 0), (256, 256, 1))


@functools.lru_cache(maxsize=None)
def col_cases():
    return [ColCase(T, N, lda, off, rgrp) for T in COL_T for (N, lda, off) in COL_SHAPES for rgrp in (0, 4)]


TRANSPOSE_SHAPES = ((8, 8), (64, 64), (72, 136), (200, 8))
RESIDUAL_CASES = ((5, 4, 1), (5, 260, 5), (37, 260, 1), (1030, 64, 5))      # (rows, D, row step): one workgroup, ..., 65 workgroups


def _seed(*key):
    h = 0
    for k in key:
        for ch in str(k):
            h = (h * 131 + ord(ch)) % 2147483629
    return h


# ------------------------------------------------------------------------------------------------ rows
def ln_rows(cls, T, D, seed):
    r = np.random.RandomState(seed)
    z = r.standard_normal((T, D))
    if cls == "normal":
        x = 2.0 * z + 0.5
    elif cls == "offset":               # mean^2 is 1e6 times the variance: E[x^2] - mean^2 cancels to nothing in fp32
        x = 1000.0 + z
    elif cls == "tight":                # variance 1e-6 below eps = 1e-5: eps decides rstd, the offset is 250 standard deviations
        x = 0.25 + 1e-3 * z
    elif cls == "spike":                # one element carries the row's variance
        x = z
        x[np.arange(T), r.randint(0, D, size=T)] = 1e4
    elif cls == "scaled":               # neighbouring rows differ by up to 1e6 in scale: a statistic taken from the wrong row shows
        x = z * 10.0 ** r.uniform(-3, 3, size=(T, 1))
    elif cls == "const":                # every partial sum of 3.75 is exact in fp32: mean = 3.75 and y = beta in any summation order
        x = np.full((T, D), 3.75)
    else:
        raise ValueError(cls)
    return x.astype(F32)


def rms_rows(cls, B, D, seed):
    r = np.random.RandomState(seed)
    z = r.standard_normal((B, D))
    if cls == "normal":
        x = z
    elif cls == "zero_rows":            # norm 0: the clamp branch with nothing to project
        x = z
        x[::3] = 0.0
    elif cls == "tiny":                 # norm below 1e-12: the clamp branch with x != 0
        x = 1e-15 * z
    elif cls == "scaled":
        x = z * 10.0 ** r.uniform(-12, 12, size=(B, 1))
    elif cls == "spike":
        x = z
        x[np.arange(B), r.randint(0, D, size=B)] = 1e6
    elif cls == "huge":                 # norm^3 is past the fp32 range, norm^2 is not
        x = z * 10.0 ** r.uniform(13, 15, size=(B, 1))
    else:
        raise ValueError(cls)
    return x.astype(F32)


def _bf16_round(a):
    return torch.from_numpy(np.array(a, dtype=F32)).to(torch.bfloat16).float().numpy()


@functools.lru_cache(maxsize=None)
def ln_inputs(cls, T, D):
    """x, gamma, beta, dy, dres (numpy fp32; shared by every case of the shape, never modified)"""
    s = _seed("ln", cls, T, D)
    r = np.random.RandomState(s + 1)
    d = {"x": ln_rows(cls, T, D, s), "gamma": (1.0 + 0.5 * r.standard_normal(D)).astype(F32), "beta": r.standard_normal(D).astype(F32),
         "dy": r.standard_normal((T, D)).astype(F32), "dres": r.standard_normal((T, D)).astype(F32)}
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def lnb_inputs(cls, T, D):
    """the bf16 configuration: delta, delta2 and dy hold bf16 values (kept as fp32 arrays), x1 = x + delta and x2 = (x + delta) + delta2
    are the fp32 sums in torch's arithmetic"""
    d = dict(ln_inputs(cls, T, D))
    r = np.random.RandomState(_seed("lnb", cls, T, D))
    d["delta"], d["delta2"] = _bf16_round(r.standard_normal((T, D))), _bf16_round(r.standard_normal((T, D)))
    d["dy"] = _bf16_round(d["dy"])
    x1 = torch.from_numpy(np.array(d["x"])) + torch.from_numpy(d["delta"])
    d["x1"], d["x2"] = x1.numpy(), (x1 + torch.from_numpy(d["delta2"])).numpy()
    for v in d.values():
        v.setflags(write=False)
    return d


def lnb_row_input(c):
    """the row the LayerNorm of a bf16 forward case normalises: x, x + delta or (x + delta) + delta2"""
    return lnb_inputs(c.cls, c.T, c.D)[("x", "x1", "x2")[lnb_add(c.variant)]]


@functools.lru_cache(maxsize=None)
def rms_inputs(cls, B, D):
    s = _seed("rms", cls, B, D)
    r = np.random.RandomState(s + 1)
    d = {"x": rms_rows(cls, B, D, s), "g": (1.0 + 0.5 * r.standard_normal(D)).astype(F32), "dy": r.standard_normal((B, D)).astype(F32)}
    for v in d.values():
        v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def col_inputs(c):
    """flat buffer of off + rows * lda floats, NaN everywhere but the logical elements (padding columns, the rows the map skips, the
    floats before the base); "rows": the (T, N) logical matrix"""
    r = np.random.RandomState(_seed("col", *c))
    rows = r.standard_normal((c.T, c.N)).astype(F32)
    R = colsum_phys_rows(c.T, c.rgrp)
    buf = np.full(c.off + R * c.lda, np.nan, dtype=F32)
    m = buf[c.off:].reshape(R, c.lda)
    m[[colsum_row(t, c.rgrp) for t in range(c.T)], :c.N] = rows
    buf.setflags(write=False)
    rows.setflags(write=False)
    return {"buf": buf, "rows": rows}


def transpose_input(rows, cols):
    return np.random.RandomState(_seed("tr", rows, cols)).standard_normal((rows, cols)).astype(F32) * F32(3.0)


# ------------------------------------------------------------------------------------------------ fp64 references
def ln_ref64(x, gamma, beta, dy=None, dres=None):
    x, gamma, beta = x.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64)
    mu = x.mean(1, keepdims=True)
    xc = x - mu
    rstd = 1.0 / np.sqrt((xc * xc).mean(1, keepdims=True) + EPS_LN)
    xh = xc * rstd
    out = {"y": xh * gamma + beta, "mean": mu[:, 0], "rstd": rstd[:, 0], "_xmax": np.abs(x).max(1)}
    if dy is not None:
        dy = dy.astype(np.float64)
        g = dy * gamma
        dx = rstd * (g - g.mean(1, keepdims=True) - xh * (g * xh).mean(1, keepdims=True))
        out["dx"] = dx if dres is None else dx + dres.astype(np.float64)
        out["dgamma"], out["dbeta"] = (dy * xh).sum(0), dy.sum(0)
        out["_mass_dgamma"], out["_mass_dbeta"] = np.abs(dy * xh).sum(0), np.abs(dy).sum(0)
    return out


def rms_ref64(x, g, dy):
    """F.normalize(x, dim=-1) * sqrt(D) * g (eps 1e-12) and its gradients; sqrt(D) and eps are the fp32 constants of the kernels"""
    x, g, dy = x.astype(np.float64), g.astype(np.float64), dy.astype(np.float64)
    sc = float(np.sqrt(F32(x.shape[1])))
    nr = np.sqrt((x * x).sum(1, keepdims=True))
    clamped = nr < EPS_RMS
    n = np.where(clamped, EPS_RMS, nr)
    u = dy * g * sc
    proj = np.where(clamped, 0.0, (x / n) * ((u * x).sum(1, keepdims=True) / n))
    summand = dy * x / n * sc
    return {"y": x / n * sc * g, "dx": (u - proj) / n, "dg": summand.sum(0), "_mass_dg": np.abs(summand).sum(0),
            "_mass_dy": np.abs(dy).sum(0), "_clamped": clamped[:, 0], "_umax": np.abs(u / n).max(1)}


def col_ref64(c):
    rows = col_inputs(c)["rows"].astype(np.float64)
    return {"sum": rows.sum(0), "_mass": np.abs(rows).sum(0)}


# ------------------------------------------------------------------------------------------------ fp32 evaluations (yardsticks, defects)
LN_DEFECTS = ("one_pass_variance", "drop_c2", "c1_without_gamma", "padded_mean", "neighbour_rstd")
RMS_DEFECTS = ("drop_projection", "clamp_keeps_projection", "n_cubed")
COL_DEFECTS = ("rgrp_without_plus_one",)


def ln_f32(x, gamma, beta, dy=None, dres=None, defect=None):
    """the kernels' two-pass algorithm in numpy fp32 (every operation rounds to fp32; numpy's own summation order)"""
    assert x.dtype == F32 and gamma.dtype == F32 and beta.dtype == F32
    D = x.shape[1]
    with np.errstate(all="ignore"):
        div = F32(ln_nch(D) * 256 if defect == "padded_mean" else D)
        mu = x.sum(1, dtype=F32, keepdims=True) / div
        xc = x - mu
        if defect == "one_pass_variance":
            var = (x * x).sum(1, dtype=F32, keepdims=True) / F32(D) - mu * mu
        else:
            var = (xc * xc).sum(1, dtype=F32, keepdims=True) / F32(D)
        rstd = F32(1.0) / np.sqrt(var + F32(EPS_LN))
        if defect == "neighbour_rstd":
            rstd = np.roll(rstd, 1, axis=0)
        xh = xc * rstd
        out = {"y": xh * gamma + beta, "mean": mu[:, 0], "rstd": rstd[:, 0]}
        if dy is not None:
            g = dy * gamma
            c1 = (dy if defect == "c1_without_gamma" else g).sum(1, dtype=F32, keepdims=True) / F32(D)
            c2 = F32(0.0) * c1 if defect == "drop_c2" else (g * xh).sum(1, dtype=F32, keepdims=True) / F32(D)
            dx = rstd * (g - c1 - xh * c2)
            out["dx"] = dx if dres is None else dx + dres
            out["dgamma"], out["dbeta"] = (dy * xh).sum(0, dtype=F32), dy.sum(0, dtype=F32)
    assert all(v.dtype == F32 for v in out.values())
    return out


def ln_torch32(x, gamma, beta, dy=None, dres=None):
    xt = torch.from_numpy(np.array(x)).requires_grad_(dy is not None)
    gt = torch.from_numpy(np.array(gamma)).requires_grad_(dy is not None)
    bt = torch.from_numpy(np.array(beta)).requires_grad_(dy is not None)
    y, mean, rstd = torch.native_layer_norm(xt, (x.shape[1],), gt, bt, 1e-5)
    out = {"y": y.detach().numpy(), "mean": mean.detach().reshape(-1).numpy(), "rstd": rstd.detach().reshape(-1).numpy()}
    if dy is not None:
        y.backward(torch.from_numpy(np.array(dy)))
        dx = xt.grad if dres is None else xt.grad + torch.from_numpy(np.array(dres))
        out.update(dx=dx.numpy(), dgamma=gt.grad.numpy(), dbeta=bt.grad.numpy())
    return out


def rms_f32(x, g, dy, defect=None):
    """rmsnorm_fwd_kernel / rmsnorm_bwd_kernel in numpy fp32.  "n_cubed" is the kernel before its repair (k = (u.x) / n^3)."""
    assert x.dtype == F32 and g.dtype == F32 and dy.dtype == F32
    with np.errstate(all="ignore"):
        sc = np.sqrt(F32(x.shape[1]))
        nr = np.sqrt((x * x).sum(1, dtype=F32, keepdims=True))
        clamped = nr < F32(EPS_RMS)
        n = np.where(clamped, F32(EPS_RMS), nr)
        u = dy * g * sc
        ux = (u * x).sum(1, dtype=F32, keepdims=True)
        if defect == "n_cubed":
            k = np.where(clamped, F32(0.0), ux / (n * n * n))
            dx = u / n - x * k
        else:
            p = ux / n
            if defect == "drop_projection":
                p = F32(0.0) * p
            elif defect != "clamp_keeps_projection":
                p = np.where(clamped, F32(0.0), p)
            dx = (u - x / n * p) / n
        out = {"y": x / n * sc * g, "dx": dx, "dg": (dy * x / n * sc).sum(0, dtype=F32)}
    assert all(v.dtype == F32 for v in out.values())
    return out


def rms_torch32(x, g, dy):
    xt, gt = torch.from_numpy(np.array(x)).requires_grad_(True), torch.from_numpy(np.array(g)).requires_grad_(True)
    y = torch.nn.functional.normalize(xt, dim=-1) * (x.shape[1] ** 0.5) * gt
    y.backward(torch.from_numpy(np.array(dy)))
    return {"y": y.detach().numpy(), "dx": xt.grad.numpy(), "dg": gt.grad.numpy()}


def col_f32(c, defect=None):
    m = col_inputs(c)["buf"][c.off:].reshape(-1, c.lda)
    rows = m[[colsum_row(t, c.rgrp, plus_one=defect != "rgrp_without_plus_one") for t in range(c.T)], :c.N]
    with np.errstate(all="ignore"):
        return {"sum": rows.sum(0, dtype=F32)}


def col_torch32(c):
    return {"sum": torch.from_numpy(np.array(col_inputs(c)["rows"])).sum(0).numpy()}


# ------------------------------------------------------------------------------------------------ distances
def bf16_half_ulp(ref):
    """half a bf16 ulp (8 significant bits) at every element of the fp64 reference"""
    a = np.abs(ref)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(a, where=a > 0, out=np.zeros_like(a)))
    return np.where(a > 0, 2.0 ** (e - 8), 0.0)


def row_dist(got, ref, scale=None, slack=None):
    T = ref.shape[0]
    got, ref = np.asarray(got, dtype=np.float64).reshape(T, -1), ref.reshape(T, -1)
    err = np.abs(got - ref)
    err[~np.isfinite(got)] = np.inf
    if slack is not None:
        err = np.maximum(err - slack.reshape(T, -1), 0.0)
    worst = err.max(1)
    den = np.abs(ref).max(1) if scale is None else scale
    with np.errstate(all="ignore"):
        r = np.where(den > 0, worst / den, np.where(worst == 0, 0.0, np.inf))
    return float(r.max())


def col_dist(got, ref, mass, alt=None):
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    err[~np.isfinite(got)] = np.inf
    worst, den = float(err.max()), float(mass.max())
    if den == 0 and alt is not None:
        den = float(alt.max())
    if den == 0:
        return 0.0 if worst == 0 else float("inf")
    return worst / den


def ln_distances(got, ref, bf16_y=False):
    """output name -> distance, for the outputs `got` holds"""
    d = {}
    for k in ("y", "dx", "rstd"):
        if k in got:
            d[k] = row_dist(got[k], ref[k], slack=bf16_half_ulp(ref[k]) if (bf16_y and k == "y") else None)
    if "mean" in got:
        d["mean"] = row_dist(got["mean"], ref["mean"], scale=ref["_xmax"])
    if "dgamma" in got:
        d["dgamma"] = col_dist(got["dgamma"], ref["dgamma"], ref["_mass_dgamma"], ref["_mass_dbeta"])
    if "dbeta" in got:
        d["dbeta"] = col_dist(got["dbeta"], ref["dbeta"], ref["_mass_dbeta"])
    return d


def rms_distances(got, ref):
    d = {}
    if "y" in got:
        d["y"] = row_dist(got["y"], ref["y"])
    if "dx" in got:
        d["dx"] = row_dist(got["dx"], ref["dx"], scale=ref["_umax"] if ref["dx"].shape[1] == 1 else None)
    if "dg" in got:
        d["dg"] = col_dist(got["dg"], ref["dg"], ref["_mass_dg"], ref["_mass_dy"])
    return d


def col_distances(got, ref):
    return {"sum": col_dist(got["sum"], ref["sum"], ref["_mass"])}


def floor_of(output, T):
    """the rounding-count floor of an output of a case with T rows"""
    return sum_floor(T) if output in ("dgamma", "dbeta", "dg", "sum") else ROW_FLOOR


# ------------------------------------------------------------------------------------------------ per-family evaluation
FAMILIES = ("ln", "lnb_fwd", "lnb_bwd", "rms", "colsum")


def family_classes(fam):
    return {"ln": LN_CLASSES, "lnb_fwd": LN_CLASSES, "lnb_bwd": LN_CLASSES, "rms": RMS_CLASSES, "colsum": ("normal",)}[fam]


def family_cases(fam, cls):
    if fam == "colsum":
        return col_cases()
    return {"ln": ln_cases, "lnb_fwd": lnb_fwd_cases, "lnb_bwd": lnb_bwd_cases, "rms": rms_cases}[fam](cls)


def case_rows(fam, c):
    return c.B if fam == "rms" else c.T


def _operands(fam, c):
    """the arguments of the family's evaluators for a case (the strided and the NULL-output variants share them)"""
    if fam == "ln":
        i = ln_inputs(c.cls, c.T, c.D)
        return (i["x"], i["gamma"], i["beta"], i["dy"], i["dres"])
    if fam == "lnb_fwd":
        i = lnb_inputs(c.cls, c.T, c.D)
        return (lnb_row_input(c), i["gamma"], i["beta"])
    if fam == "lnb_bwd":
        i = lnb_inputs(c.cls, c.T, c.D)
        return (i["x"], i["gamma"], i["beta"], i["dy"], i["dres"])
    if fam == "rms":
        i = rms_inputs(c.cls, c.B, c.D)
        return (i["x"], i["g"], i["dy"])
    raise ValueError(fam)


def _shape_key(fam, c):
    """cases with the same key have the same reference and the same fp32 evaluations"""
    if fam == "colsum":
        return c
    if fam == "lnb_fwd":
        return (c.cls, c.T, c.D, lnb_add(c.variant))
    return (c.cls, case_rows(fam, c), c.D)


@functools.lru_cache(maxsize=None)
def _reference(fam, key, c):
    if fam == "colsum":
        return col_ref64(c)
    return (rms_ref64 if fam == "rms" else ln_ref64)(*_operands(fam, c))


def reference(fam, c):
    return _reference(fam, _shape_key(fam, c), c if fam == "colsum" else _canonical(fam, c))


def _canonical(fam, c):
    """one representative per shape key, so that the caches hold one entry per key"""
    if fam in ("ln", "lnb_bwd"):
        return c._replace(rs=1)
    if fam == "lnb_fwd":
        return c._replace(rs=1, variant=("plain", "add", "add2")[lnb_add(c.variant)])
    return c


def distances(fam, c, got):
    ref = reference(fam, c)
    if fam == "rms":
        return rms_distances(got, ref)
    if fam == "colsum":
        return col_distances(got, ref)
    return ln_distances(got, ref, bf16_y=fam == "lnb_fwd")


def fp32_evaluations(fam, c, defect=None):
    """the honest fp32 evaluations of a case (torch, numpy restatement), or the restatement with a defect alone"""
    if fam == "colsum":
        return [col_f32(c, defect)] if defect else [col_torch32(c), col_f32(c)]
    ops = _operands(fam, c)
    if fam == "rms":
        return [rms_f32(*ops, defect=defect)] if defect else [rms_torch32(*ops), rms_f32(*ops)]
    return [ln_f32(*ops, defect=defect)] if defect else [ln_torch32(*ops), ln_f32(*ops)]


@functools.lru_cache(maxsize=None)
def _fp32_distances(fam, key, c):
    out = {}
    for ev in fp32_evaluations(fam, c):
        for k, v in distances(fam, c, ev).items():
            out[k] = max(out.get(k, 0.0), v)
    return out


def fp32_distances(fam, c):
    """output -> the larger fp32 distance of the two honest evaluations on case c"""
    return _fp32_distances(fam, _shape_key(fam, c), c if fam == "colsum" else _canonical(fam, c))


def admitted(fam, c):
    """The rule is applied to a case only if honest fp32 arithmetic is within Y_CAP of fp64 on it, for every output.  The cap was set
    for the row classes at moderate shapes; two kinds of shape of the "offset" class (1000 + N(0, 1)) exceed it by up to 2.4 times: D = 4,
    where the four-element row maximum that divides the error is often small, and rows of 32 columns by the thousand, where the largest
    of 2047 row distances is a tail value.  Those shapes (NOT_ADMITTED, pinned by the host test) still run for the bit-exact conditions."""
    return all(v <= Y_CAP for v in fp32_distances(fam, c).values())


# (family, class, rows, D) of the shapes admitted() turns away; tests/test_row_kernel_matrix_host.py checks that these are all of them
NOT_ADMITTED = (("ln", "offset", 5, 4), ("ln", "offset", 2047, 32), ("ln", "offset", 2051, 32), ("lnb_bwd", "offset", 5, 4))


@functools.lru_cache(maxsize=None)
def yardsticks(fam, cls):
    """output -> Y of the (family, class): the largest fp32 distance over the class's admitted cases and both evaluations"""
    Y = {}
    for c in family_cases(fam, cls):
        if admitted(fam, c):
            for k, v in fp32_distances(fam, c).items():
                Y[k] = max(Y.get(k, 0.0), v)
    return Y


def violations(fam, c, got):
    """[(output, distance, bound)] of the outputs of `got` that break the rule on case c"""
    assert admitted(fam, c), c
    Y = yardsticks(fam, "normal" if fam == "colsum" else c.cls)
    T = case_rows(fam, c)
    return [(k, v, bound(Y[k], floor_of(k, T))) for k, v in distances(fam, c, got).items() if not v <= bound(Y[k], floor_of(k, T))]
