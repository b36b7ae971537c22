"""The fp32 attention matrix: case table, dispatch restated, data classes, fp64 reference, error masses, CPU yardstick, rule and defects.

Shared by tests/test_attention_fp32_matrix_host.py (CPU: everything here is checked against itself) and
tests/test_gpu_attention_fp32_matrix.py (the kernels of csrc/attention.hip and csrc/attention_long.hip against the reference).  Nothing
here touches a GPU; the reference and the masses run on whatever device their operands are on, so the GPU file may evaluate the
many-item problems of the pipelined kernel in torch fp64 on the device (one of them is compared with the CPU result there).  The
structure is that of tests/attention_bf16_cases.py without the bf16 roundings.

Layout: qkv (B, N, 3 H dh) fp32 = [q | k | v], head h in columns dh h .. dh h + dh - 1 of each third; out (B, N, H dh); lse (B, H, N),
base 2; dqkv like qkv.  dh is 64 or 32; scale = fp32(1 / sqrt(dh)), qscale = fp32(scale * fp32(log2 e)) as the kernels form them.

The rule.  v = 2^-24 is the unit roundoff of fp32.  Every output element has an error MASS: the first-order size of what the rounding
points the kernels have by design can do to it, with S the scaled scores (natural units), P = softmax(S), A_ij = scale sum_d |q_id k_jd|:
  * scores and the exponent: a probability's numerator carries e_ij = A_ij + |S_ij - max_i| + 1 units of v (the sum of products with the
    pre-scaled q, the one rounding of the difference, exp2), one more with dropout (the product with fp32(1 / keep)); the backward
    recomputes P from the fp32 lse, which adds ln2 (|S2_ij| + |lse_i|) v for the two roundings of the difference of two large base-2
    numbers, and ln2 mass(lse_i) for the lse it is given;
  * fp32 accumulation of every product: v times the sum of absolute products; the reciprocal of the row sum and the product with it (the
    un-scaling of bwd64's dk alike): 2 v |stored value|;
  * delta = rowsum(dout o out) from the fp32 `out` the backward is given: mass(delta_i) = sum_d |dout_id| mass(out_id) +
    v sum_d |dout_id out_id|, which enters dS as P_ij mass(delta_i) scale -- the leading term of `offset-v`, where dP - delta cancels two
    numbers of size 100 sum |dout|;
  * lse: v (log2e sum_j P_ij e_ij + 2 |lse_i| + |max2_i| + 1);
  * underflow: a probability below TINY = 2^-126, the smallest normal fp32 number, is a denormal on the CPU and may be flushed to zero
    by the kernels' exp2: every probability carries TINY absolutely, beside its relative units, in each product it enters (moving-max
    with one query has probabilities of 1e-40, whose relative mass would be 1e-45: without this term the restatement alone had Y of
    5.6e4 there).
  With dropout (mask m in {0, 1}, keep) the products P V and P^T dO take m o P / keep in place of P, and dP = (dO V^T) o m / keep.
The YARDSTICK Y of a case and an output is the largest |restatement - fp64| / mass over the output's elements, where the restatement
(restate_fwd, restate_bwd) is plain torch fp32 on the CPU: q pre-scaled by qscale, whole-row softmax in base 2, no tiles.  The forward
has more honest orders of the same products, and Y is the largest over all of them: restate_fwd_online (the online softmax over trips of
64 keys) and restate_fwd_sequential (the kernels' order of steps: two products per step with every operation rounded on its own, the
same as two chained fma, and with the scores in the one-query kernels' tree order); the backward has restate_bwd_sequential, the
two-phase kernel's order in chained fma.  The last was added because the
kernels broke the rule of the first two in five of 1576 cases on the MI355X: a CPU matrix product sums in blocks, the
matrix cores two products per step, one step after the other.  A kernel element passes when
        |got - fp64| <= max(MARGIN * Y * mass, FLOOR),      MARGIN = 2,
for every element, with no exclusions; a NaN never passes.  FLOOR = one fp32 ulp of the reference value + the mass: a second honest
summation order of the same products may differ by that much, and Y is luck where the reference cancels to nothing (N = 1: dq and dk
are exactly 0 in exact arithmetic, the restatement's and the kernels' are two different fp32 noises).  For lse, FLOOR =
LSE_FLOOR_ULPS = 4 fp32 ulps of the reference value.  Y comes from the reference side only; the host test asserts
0 <= Y <= Y_CAP = 8 for every problem and output, and Y > 0 outside the exact classes.

Data classes: gauss; moving-max (q x 4 and the keys of one 32-key tile x 6; the tile is the first, a middle, the last full and the
partial last one in turn over the items of a problem); flat (q x 2^-6); offset-v (V = 100 + N(0, 1)); token0 (backward: dout is zero
outside row 0); and two constructed classes in which a property is exact:
  * select: every token has a CODE: two coordinates c1 < c2 of the head and two signs.  k_j = 128 (s1 e_c1 + s2 e_c2) of j's code, q_i the
    same vector of pi(i)'s code.  A score has at most two non-zero products, each +-16384 qscale, so it is the same fp32 number in every
    summation order AND in both operation orders the kernels use ((q qscale) . k in the forward, the dq pass, bwd64 and the one-query
    kernels; (q . k) qscale in the dk / dv pass): 32768 qscale for the selected key, at most 16384 qscale for any other, a lead of 2954
    (dh 64) or 4178 (dh 32) base-2 units (every other probability is a zero in fp32 and in the fp64 reference alike).  So every rescale of junk accumulated before the
    selected key multiplies by an exact zero, and out[i] == V[pi(i)], lse == fp32(32768 qscale), dv[j] == dout[pi^-1(j)] bit for bit and
    dq == dk == 0 (dout and V are small integers in the backward so that dP == delta exactly).  (The +-16 sign codes of the bf16 matrix
    would not do here: their score is a sum of dh equal products of a 24-bit number, whose partial sums 3 x, 5 x, ... round, so lse and
    the recomputed P of the backward would be exact in no kernel -- the pre-scaled q of fp32 is what the bf16 kernels do not have.)
  * tie: select with every code shared by two keys (an odd last key has its own and is never selected): p = 1, 1, l = 2, and out[i] ==
    RN_fp32(V_a + V_b) / 2 bit for bit.
  The bf16 matrix's near-tie is about bf16 probabilities and has no counterpart here.
"""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

import layer_dropout_ref as LD

V32 = 2.0 ** -24
MARGIN = 2.0
Y_CAP = 8.0
LSE_FLOOR_ULPS = 4
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
INF = float("inf")
DROP_SEED, DROP_LAYER = 0x1234ABCD5, 3        # the seed (more than 32 bits) and layer of every dropout case
CODE_AMP = 128.0
TINY = 2.0 ** -126                            # the smallest normal fp32 number: exp2 of the kernels flushes what lies below


def scale32(dh):
    return float(np.float32(1.0) / np.sqrt(np.float32(dh)))


def qscale32(dh):
    """the kernels' qscale = scale * DGVIT_LOG2E, in fp32"""
    return float(np.float32(scale32(dh)) * np.float32(LOG2E))


def select_lse(dh):
    return float(np.float32(2 * CODE_AMP * CODE_AMP) * np.float32(qscale32(dh)))        # exact: a power of two times qscale


FWD_CLASSES = ("gauss", "moving-max", "flat", "tie", "offset-v", "select")
BWD_CLASSES = FWD_CLASSES + ("token0",)
EXACT_CLASSES = ("select", "tie")
FWD_OUTPUTS = ("out", "lse")
BWD_OUTPUTS = ("dq", "dk", "dv")
QUERY_ROWS = ("out", "lse", "dq")            # outputs with one row per query: only rows < nq exist

# ------------------------------------------------------------------------------------------------ the dispatch, restated
FWD_KERNELS = ("tile1", "tile2", "tile4", "pipe", "q1", "tiled", "drop", "tiled_drop")
BWD_KERNELS = ("two-phase1", "two-phase2", "two-phase4", "bwd64", "q1", "tiled", "drop", "tiled_drop")
PIPE_ITEMS = 2048
MAX_TOKENS = 288

# op: "fwd" | "bwd"; entry: "fused" (attention_fwd / attention_bwd) | "tiled"; q1 / bwd64: the value given to
# dgvit_set_attention_single_query / dgvit_set_attention_bwd_single_pass, None = left at the default (on); lse: a non-NULL lse (forward);
# keep < 1: the _drop entry points with DROP_SEED and DROP_LAYER
Case = namedtuple("Case", "op entry cls B N H dh nq lse q1 bwd64 keep")


def case_id(c):
    s = f"{c.op}-{c.entry}-{c.cls}-B{c.B}H{c.H}N{c.N}d{c.dh}"
    s += (f"-nq{c.nq}" if c.nq != c.N else "") + ("" if c.lse else "-nolse")
    s += (f"-q1.{c.q1}" if c.q1 is not None else "") + (f"-b64.{c.bwd64}" if c.bwd64 is not None else "")
    return s + (f"-keep{c.keep}" if c.keep < 1 else "")


def kernel_reached(c):
    """the kernel that attention_fwd / attention_bwd / attention_fwd_tiled / attention_bwd_tiled launch for the case"""
    drop = c.keep < 1.0
    if c.entry == "tiled":
        return "tiled_drop" if drop else "tiled"
    assert c.entry == "fused" and 1 <= c.N <= MAX_TOKENS and c.dh in (64, 32)
    q1 = 1 if c.q1 is None else int(bool(c.q1))
    b64 = 1 if c.bwd64 is None else int(bool(c.bwd64))
    nt = (c.N + 31) // 32
    waves = 1 if nt == 1 else 2 if nt == 2 else 4
    if drop:
        return "drop"
    if q1 and c.nq == 1 and c.N <= 64:
        return "q1"
    if c.op == "fwd":
        if c.nq == c.N and 32 < c.N <= 64 and c.B * c.H >= PIPE_ITEMS:
            return "pipe"
        return f"tile{waves}"
    if b64 and c.nq == c.N and 32 < c.N <= 64:
        return "bwd64"
    return f"two-phase{waves}"


def drop_waves(c):
    """the instantiation behind `drop` (the general kernels at 1, 2 or 4 waves)"""
    nt = (c.N + 31) // 32
    return 1 if nt == 1 else 2 if nt == 2 else 4


def items_per_workgroup(items):
    """(fewest, most) items a workgroup of the pipelined kernel walks: its grid is min(items, 1024)"""
    grid = min(items, 4 * 256)
    return items // grid, -(-items // grid)


# ------------------------------------------------------------------------------------------------ the case table
TILE1_N = (1, 2, 31, 32)
TILE2_N = (33, 34, 35, 40, 41, 48, 49, 50, 56, 57, 63, 64)
TILE4_N = (65, 96, 97, 128, 129, 160, 161, 197, 224, 225, 256, 257, 287, 288)
Q1_N = (1, 17, 32, 33, 50, 64)
Q1_ITEMS = ((1, 1), (1, 3), (2, 2), (5, 1), (10, 13))            # 1, 3, 4, 5, 130 items
TILED_N = (1, 63, 64, 65, 127, 128, 129, 192, 193, 257, 289, 321, 513)
DROP_N = (7, 33, 50, 65, 197, 288)
DROP_TILED_N = DROP_N + (321,)
DROP_KEEPS = (0.5, 0.9)
PIPE_SHAPES = ((512, 4), (683, 3), (83, 37))                      # 2048, 2049, 3071 items
NOT_PIPE_SHAPE = (89, 23)                                         # 2047 items
DHS = (64, 32)
LISTED_N = {
    ("fwd", "tile1"): TILE1_N, ("fwd", "tile2"): TILE2_N, ("fwd", "tile4"): TILE4_N, ("fwd", "pipe"): TILE2_N, ("fwd", "q1"): Q1_N,
    ("fwd", "tiled"): TILED_N, ("fwd", "drop"): DROP_N, ("fwd", "tiled_drop"): DROP_TILED_N,
    ("bwd", "two-phase1"): TILE1_N, ("bwd", "two-phase2"): TILE2_N, ("bwd", "two-phase4"): TILE4_N, ("bwd", "bwd64"): TILE2_N,
    ("bwd", "q1"): Q1_N, ("bwd", "tiled"): TILED_N, ("bwd", "drop"): DROP_N, ("bwd", "tiled_drop"): DROP_TILED_N,
}
RICH_N = {TILE1_N: 32, TILE2_N: 50, TILE4_N: 197, TILED_N: 321}     # every class at these token counts


def classes_of(cls_list, N):
    # tie needs a pair of keys
    return tuple(k for k in cls_list if not (k == "tie" and N < 2))


def thinned(cls_list, ns):
    """(N, class) pairs: every N of the family, every class, every class at the family's rich N, gauss at every N"""
    out = []
    for i, N in enumerate(ns):
        cl = classes_of(cls_list, N)
        pick = cl if N == RICH_N.get(ns) else dict.fromkeys(("gauss", cl[i % len(cl)], cl[(i + 3) % len(cl)]))
        out += [(N, k) for k in pick]
    return out


def small_shape(i):
    """B in {2, 3}, H in {2, 3}: frame and head strides both matter"""
    return ((2, 3), (3, 2), (3, 3), (2, 2))[i % 4]


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []

    def add(op, entry, cls, B, N, H, dh, nq=None, lse=True, q1=None, bwd64=None, keep=1.0):
        out.append(Case(op, entry, cls, B, N, H, dh, N if nq is None else nq, lse, q1, bwd64, keep))

    for dh in DHS:
        # ---- the fused kernels, forward and backward, nq = N: tile1 / tile2 / tile4, two-phase 1 / 2 / 4 and bwd64
        for fam in (TILE1_N, TILE2_N, TILE4_N):
            for i, (N, cls) in enumerate(thinned(FWD_CLASSES, fam)):
                B, H = small_shape(i)
                add("fwd", "fused", cls, B, N, H, dh)
            for i, (N, cls) in enumerate(thinned(BWD_CLASSES, fam)):
                B, H = small_shape(i)
                add("bwd", "fused", cls, B, N, H, dh)
                if fam is TILE2_N:
                    add("bwd", "fused", cls, B, N, H, dh, bwd64=0)
        # ---- nq < N on the tile kernels (33 queries: two query tiles, the second with one row), and with the one-query knob off
        for N in (50, 64, 65, 197, 288):
            for cls in ("gauss", "select"):
                for op in ("fwd", "bwd"):
                    add(op, "fused", cls, 2, N, 3, dh, nq=33)
        for N in (65, 197, 288):
            for cls in ("gauss", "select"):
                for op in ("fwd", "bwd"):
                    add(op, "fused", cls, 2, N, 3, dh, nq=1)
        # ---- the one-query kernels: every N at every item count, classes in turn; the same cases on the tile kernels (knob off)
        for i, N in enumerate(Q1_N):
            for j, (B, H) in enumerate(Q1_ITEMS):
                for op, classes in (("fwd", FWD_CLASSES), ("bwd", BWD_CLASSES)):
                    cl = classes_of(classes, N)
                    for cls in dict.fromkeys((cl[(i + j) % len(cl)], "gauss" if (i + j) % 2 else "select")):
                        add(op, "fused", cls, B, N, H, dh, nq=1)
                        add(op, "fused", cls, B, N, H, dh, nq=1, q1=0)
        # ---- lse NULL on every forward kernel
        for N, kw in ((32, {}), (50, {}), (197, {}), (50, dict(nq=1)), (50, dict(keep=0.5)), (50, dict(nq=1, q1=0))):
            for cls in ("gauss",) if "keep" in kw else ("gauss", "select"):
                add("fwd", "fused", cls, 2, N, 3, dh, lse=False, **kw)
        for kw in ({}, dict(keep=0.5)):
            add("fwd", "tiled", "gauss", 2, 257, 2, dh, lse=False, **kw)
        # ---- the pipelined forward: 2048 items at every N; 2049 and 3071 items (two or three items per workgroup) at fewer; 2047 -> tile2
        for s, (B, H) in enumerate(PIPE_SHAPES):
            ns = TILE2_N if s == 0 else ((33, 41, 50, 57, 64) if dh == 64 else (33, 50, 64))
            for i, N in enumerate(ns):
                classes = FWD_CLASSES if (s == 0 and N == 50) else dict.fromkeys(("gauss" if i % 2 else "select", FWD_CLASSES[i % 6]))
                for cls in classes:
                    add("fwd", "fused", cls, B, N, H, dh)
        add("fwd", "fused", "gauss", PIPE_SHAPES[0][0], 50, PIPE_SHAPES[0][1], dh, lse=False)
        for cls in ("gauss", "select"):
            add("fwd", "fused", cls, NOT_PIPE_SHAPE[0], 50, NOT_PIPE_SHAPE[1], dh)
        # ---- the tiled kernels
        for op, classes in (("fwd", FWD_CLASSES), ("bwd", BWD_CLASSES)):
            for i, (N, cls) in enumerate(thinned(classes, TILED_N)):
                add(op, "tiled", cls, 2, N, 2 + i % 2, dh)
            for N in (65, 129, 257, 513):
                for nq in (1, 33):
                    add(op, "tiled", "gauss", 2, N, 2, dh, nq=nq)
                    add(op, "tiled", "select", 2, N, 2, dh, nq=nq)
        # ---- dropout: both keeps at every N (N % 4 != 0 on purpose), every query count
        for keep in DROP_KEEPS:
            for op in ("fwd", "bwd"):
                for i, N in enumerate(DROP_N):
                    add(op, "fused", "gauss", 2, N, 3, dh, keep=keep)
                    add(op, "fused", ("offset-v", "moving-max", "flat")[i % 3], 3, N, 2, dh, keep=keep)
                for i, N in enumerate(DROP_TILED_N):
                    add(op, "tiled", "gauss", 2, N, 2, dh, keep=keep)
                    add(op, "tiled", ("offset-v", "moving-max", "flat")[i % 3], 2, N, 3, dh, keep=keep)
                for N in (50, 197):
                    for nq in (1, 33):
                        add(op, "fused", "gauss", 2, N, 3, dh, nq=nq, keep=keep)
                        add(op, "tiled", "gauss", 2, N, 2, dh, nq=nq, keep=keep)
    return tuple(dict.fromkeys(out))


Problem = namedtuple("Problem", "op cls B N H dh nq keep")        # operands without their path; nq < N only in the backward


def problem(c):
    return Problem(c.op, c.cls, c.B, c.N, c.H, c.dh, c.nq if c.op == "bwd" else c.N, c.keep)


def problem_id(p):
    return f"{p.op}-{p.cls}-B{p.B}H{p.H}N{p.N}d{p.dh}" + (f"-nq{p.nq}" if p.nq != p.N else "") + (f"-keep{p.keep}" if p.keep < 1 else "")


# ------------------------------------------------------------------------------------------------ operands per data class
# qkv, dout: CPU fp32 (dout rows >= nq are zero: the backward must not read them); meta: the class's construction (pi, mask, ...)
Operands = namedtuple("Operands", "qkv dout B N H dh nq keep meta")


def _gen(p, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(repr((tuple(p[:6]), salt)).encode()))


def heads(x, H):
    B, N, I = x.shape
    return x.reshape(B, N, H, I // H).permute(0, 2, 1, 3)


def unheads(x):
    B, H, N, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, N, H * dh)


def split(qkv, H):
    I = qkv.shape[-1] // 3
    return heads(qkv[..., :I], H), heads(qkv[..., I:2 * I], H), heads(qkv[..., 2 * I:], H)


def join(q, k, v):
    return torch.cat([unheads(q), unheads(k), unheads(v)], dim=-1).contiguous()


def moving_max_tile(N, pos):
    """the 32-key tile that `moving-max` scales for position 0..3 (first, middle, last full, partial last)"""
    nkt, full = (N + 31) // 32, N // 32
    return (0, nkt // 2, max(full - 1, 0), nkt - 1)[pos % 4]


def n_codes(dh):
    return dh * (dh - 1) // 2 * 4


def _code_vectors(idx, dh):
    """(..., dh) fp32: code number -> CODE_AMP (s1 e_c1 + s2 e_c2)"""
    pairs = torch.combinations(torch.arange(dh), 2)
    pr, sg = pairs[idx // 4], idx % 4
    vec = torch.zeros(idx.shape + (dh,))
    vec.scatter_(-1, pr[..., :1], (1.0 - 2.0 * (sg // 2).float())[..., None] * CODE_AMP)
    vec.scatter_(-1, pr[..., 1:], (1.0 - 2.0 * (sg % 2).float())[..., None] * CODE_AMP)
    return vec


def _codes(g, B, H, n, dh):
    """n distinct codes per item"""
    return torch.stack([torch.randperm(n_codes(dh), generator=g)[:n] for _ in range(B * H)]).reshape(B, H, n)


def _perms(g, B, H, n):
    return torch.stack([torch.randperm(n, generator=g) for _ in range(B * H)]).reshape(B, H, n)


def attention_mask(B, H, N, keep, layer=DROP_LAYER, seed=DROP_SEED, row_stride=None, frames=None):
    """the {0, 1} fp64 mask (B, H, N, N) of the attention probabilities (site 0 of include/dgvit_hip.h): layer_dropout_ref.mask, or with
    row_stride given the same Philox words at float4 group row * row_stride + key // 4 (a defect: the stride is ceil(N / 4))"""
    if row_stride is None:
        return LD.mask(LD.SITE_ATTN, layer, (B, H, N, N), seed, keep, frames)
    n4 = (N + 3) // 4
    rows = np.arange(B * H * N, dtype=np.uint64).reshape(B, H, N, 1)
    i4 = rows * np.uint64(row_stride) + np.arange(n4, dtype=np.uint64)
    m = LD._keep_words(i4, LD.site_tag(LD.SITE_ATTN, layer), seed, keep).reshape(B, H, N, 4 * n4)[..., :N]
    return torch.from_numpy(m.astype(np.float64))


@functools.lru_cache(maxsize=8)
def operands(p):
    """the operands of a problem, by its class; deterministic in the problem (the same q, k, v whatever nq and keep)"""
    g = _gen(p)
    B, N, H, dh = p.B, p.N, p.H, p.dh
    I = H * dh
    meta = {}
    q, k, v = (torch.randn(B, H, N, dh, generator=g) for _ in range(3))
    dout = torch.randn(B, N, I, generator=g)
    if p.cls == "moving-max":
        q = q * 4.0
        for it in range(B * H):
            t = moving_max_tile(N, it)
            k[it // H, it % H, 32 * t:32 * t + 32] *= 6.0
    elif p.cls == "flat":
        q = q * 2.0 ** -6
    elif p.cls == "offset-v":
        v = v + 100.0
    elif p.cls == "token0":
        dout[:, 1:] = 0.0
    elif p.cls in ("select", "tie"):
        assert N <= n_codes(dh)
        code = _codes(g, B, H, N, dh)
        if p.cls == "select":
            pi = _perms(g, B, H, N)
        else:
            npair = N // 2
            code[:, :, npair:2 * npair] = code[:, :, :npair]
            sig = _perms(g, B, H, npair)
            pi = torch.gather(sig, 2, (torch.arange(N) % npair).expand(B, H, N))       # query i selects the pair pi(i), pi(i) + npair
            meta["npair"] = npair
        k = _code_vectors(code, dh)
        q = _code_vectors(torch.gather(code, 2, pi), dh)
        meta["pi"] = pi
        if p.op == "bwd":                                                               # dP == delta exactly on small integers
            v = torch.randint(-4, 5, (B, H, N, dh), generator=g).float()
            dout = torch.randint(-3, 4, (B, N, I), generator=g).float()
        _assert_selected(q, k, pi, meta.get("npair"), dh)
    else:
        assert p.cls == "gauss", p.cls
    if p.nq < N:
        dout[:, p.nq:] = 0.0
    if p.keep < 1:
        assert p.cls not in EXACT_CLASSES
        meta["mask"] = attention_mask(B, H, N, p.keep)
    return Operands(join(q, k, v), dout if p.op == "bwd" else None, B, N, H, dh, p.nq, p.keep, meta)


def _assert_selected(q, k, pi, npair, dh):
    """fp64: everything but the selected key (or pair) of a row is more than 200 base-2 units below it, and the selected logit is the
    fp32 number select_lse(dh) in both operation orders of the kernels"""
    s = q.double() @ k.double().transpose(-1, -2)
    N = s.shape[-1]
    sel = torch.zeros_like(s, dtype=torch.bool).scatter_(-1, pi[..., None], True)
    if npair is not None:
        sel.scatter_(-1, (pi + npair)[..., None], True)
    assert bool((s[sel] == 2 * CODE_AMP * CODE_AMP).all()), "select / tie: a selected score is not 2 a^2"
    if N > (1 if npair is None else 2):
        rest = s.masked_fill(sel, -INF).amax(-1)
        assert float(rest.max()) <= CODE_AMP * CODE_AMP, "select / tie: an unselected key shares both coordinates"
    assert CODE_AMP * CODE_AMP * qscale32(dh) > 200.0 + math.log2(max(N, 2))
    qs = np.float32(CODE_AMP) * np.float32(qscale32(dh))
    assert float(np.float32(qs * np.float32(CODE_AMP)) * 2) == select_lse(dh) == float(np.float32(2 * CODE_AMP * CODE_AMP) * np.float32(qscale32(dh)))


def select_expect(ops, p):
    """what the exact classes promise, as tensors in the layout of the outputs (absent: no promise for that output)"""
    _, _, v = split(ops.qkv, ops.H)
    B, N, H, dh = ops.B, ops.N, ops.H, ops.dh
    pi = ops.meta["pi"]
    idx = pi[..., None].expand(B, H, N, dh)
    if p.cls == "select":
        exp = {"out": unheads(torch.gather(v, 2, idx)), "lse": torch.full((B, H, N), select_lse(dh), dtype=torch.float32)}
        if p.op == "bwd":
            do = heads(ops.dout, H)
            dv = torch.zeros_like(do).scatter_(2, idx, do)                  # dv[pi(i)] = dout[i] (rows >= nq of dout are zero)
            exp.update(dq=torch.zeros_like(ops.dout), dk=torch.zeros_like(ops.dout), dv=unheads(dv))
        return exp
    va, vb = torch.gather(v, 2, idx), torch.gather(v, 2, (pi + ops.meta["npair"])[..., None].expand(B, H, N, dh))
    return {"out": unheads((va + vb) * 0.5)}


# ------------------------------------------------------------------------------------------------ fp64 reference and masses
def reference(ops, device="cpu"):
    """fp64 forward (and gradient where the operands have a dout) with the mass of every output: {name: (ref, mass)} in the outputs'
    layouts.  The gradient is the true one: of the fp64 forward, not of a rounded `out`."""
    H, dh = ops.H, ops.dh
    sc = scale32(dh)
    q, k, v = split(ops.qkv.to(device).double(), H)
    S = (q @ k.transpose(-1, -2)) * sc
    mx = S.amax(-1, keepdim=True)
    E = torch.exp(S - mx)
    P = E / E.sum(-1, keepdim=True)
    lse = (mx + torch.log(E.sum(-1, keepdim=True))).squeeze(-1) * LOG2E
    del E
    drop = ops.keep < 1
    md = ops.meta["mask"].to(device) / float(np.float32(ops.keep)) if drop else None      # m / keep, keep the fp32 number the kernels get
    Pd = P * md if drop else P
    out = Pd @ v
    A = (q.abs() @ k.abs().transpose(-1, -2)) * sc
    e = A + (S - mx).abs() + (2.0 if drop else 1.0)
    Pe = Pd * e
    PV = Pd @ v.abs()
    vsum = v.abs().sum(-2, keepdim=True) * (float(md.max()) if drop else 1.0)
    m_out = V32 * (Pe @ v.abs() + (P * e).sum(-1, keepdim=True) * out.abs() + PV + 2.0 * out.abs()) + TINY * (vsum + S.shape[-1] * out.abs())
    m_lse = V32 * (LOG2E * (P * e).sum(-1) + 2.0 * lse.abs() + LOG2E * mx.squeeze(-1).abs() + 1.0)
    res = {"out": (unheads(out), unheads(m_out)), "lse": (lse, m_lse)}
    if ops.dout is None:
        return res
    del Pe, PV
    do = heads(ops.dout.to(device).double(), H)
    dPd = do @ v.transpose(-1, -2)
    dP = dPd * md if drop else dPd
    delta = (do * out).sum(-1, keepdim=True)
    dS = P * (dP - delta) * sc
    dq, dk, dv = dS @ k, dS.transpose(-1, -2) @ q, Pd.transpose(-1, -2) @ do
    ep = V32 * (A + LN2 * ((S * LOG2E).abs() + lse.abs()[..., None]) + 1.0) + LN2 * m_lse[..., None]
    AdP = do.abs() @ v.abs().transpose(-1, -2)
    if drop:
        AdP = 2.0 * AdP * md
    m_delta = (do.abs() * m_out).sum(-1, keepdim=True) + V32 * (do * out).abs().sum(-1, keepdim=True)
    W = ((P * ep + TINY) * (dP - delta).abs() + P * (V32 * AdP + m_delta)) * sc + 2.0 * V32 * dS.abs()
    Wp = Pd * (ep + V32) + TINY * (md if drop else 1.0)
    res["dq"] = (unheads(dq), unheads(W @ k.abs() + 2.0 * V32 * dq.abs()))
    res["dk"] = (unheads(dk), unheads(W.transpose(-1, -2) @ q.abs() + 3.0 * V32 * dk.abs()))
    res["dv"] = (unheads(dv), unheads(Wp.transpose(-1, -2) @ do.abs() + 2.0 * V32 * dv.abs()))
    return res


# ------------------------------------------------------------------------------------------------ the CPU restatement (and the defects)
def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _mask_of(ops, defect):
    """(forward mask, factor) of a dropped problem, fp32, with the mask defects"""
    B, N, H = ops.B, ops.N, ops.H
    m = ops.meta["mask"]
    if defect == "mask_transposed":
        m = m.transpose(-1, -2)
    if defect == "mask_stride":
        m = attention_mask(B, H, N, ops.keep, row_stride=N // 4)
    if defect == "mask_other_layer":
        m = attention_mask(B, H, N, ops.keep, layer=DROP_LAYER + 1)
    inv = _f32(1.0) if defect == "no_inv_keep" else _f32(1.0) / _f32(ops.keep)
    return m.float() * inv


def restate_fwd(ops, defect=None):
    """plain torch fp32: q pre-scaled by qscale, base-2 softmax over the whole row, out = (P V) (1 / l), lse = m + log2(l).
    -> out (B, N, I), lse (B, H, N)"""
    H, N, dh = ops.H, ops.N, ops.dh
    q, k, v = split(ops.qkv, H)
    if defect == "head_v":
        v = torch.roll(v, -1, 1)
    if defect == "frame_k":
        k = torch.roll(k, -1, 0)
    if defect == "stale_k":                          # item i > 0 computes on item i - 1's K image
        kk = k.reshape(-1, N, dh)
        k = torch.cat([kk[:1], kk[:-1]]).reshape(k.shape)
    if defect == "pad_key":                          # keys N .. NP - 1 taken into the softmax with their zero rows
        pad = (-N) % 32
        k = torch.nn.functional.pad(k, (0, 0, 0, pad))
        v = torch.nn.functional.pad(v, (0, 0, 0, pad))
    qs = q * _f32(scale32(dh) if defect == "no_log2e" else qscale32(dh))
    s = qs @ k.transpose(-1, -2)
    if defect == "drop_last":
        s[..., -1] = -INF
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    l = p.sum(-1, keepdim=True)
    pd = p
    if ops.keep < 1:
        pd = p * _mask_of(ops, defect)
        if defect == "lse_dropped":
            l = pd.sum(-1, keepdim=True)
    out = (pd @ v) * (1.0 / l)
    lse = m + torch.log2(l)
    if defect == "lse_nat":
        lse = lse * LN2
    if defect == "lse_nomax":
        lse = torch.log2(l)
    return unheads(out), lse.squeeze(-1)


def restate_fwd_online(ops, defect=None):
    """restate_fwd with the softmax taken online over pairs of 32-key tiles, as every tile kernel walks them (a running maximum, the
    accumulator rescaled when it moves): only here can the two tile-order defects be stated, and this is the key-tile-sequential fp32
    accumulation of O.  Without a defect it meets the rule like restate_fwd."""
    H, N, dh = ops.H, ops.N, ops.dh
    assert ops.keep == 1.0
    q, k, v = split(ops.qkv, H)
    pad = (-N) % 64
    k, v = torch.nn.functional.pad(k, (0, 0, 0, pad)), torch.nn.functional.pad(v, (0, 0, 0, pad))
    ntr = (N + pad) // 64
    s = (q * _f32(qscale32(dh))) @ k.transpose(-1, -2)
    s[..., N:] = -INF
    m = torch.full(s.shape[:-1] + (1,), -INF)
    l, o = torch.zeros_like(m), torch.zeros(q.shape)
    for t in range(ntr):
        st = s[..., 64 * t:64 * t + 64]
        vt = v[..., 64 * t:64 * t + 64, :]
        if defect == "swap_tiles" and 64 * t + 32 < N:          # the V tiles of a pair change places, the K tiles do not
            vt = torch.cat([vt[..., 32:, :], vt[..., :32, :]], -2)
        mn = torch.maximum(m, st.amax(-1, keepdim=True))
        alpha = torch.exp2(m - mn)
        if defect == "no_rescale" and t > 0:
            alpha = torch.ones_like(alpha)
        p = torch.exp2(st - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p @ vt
        m = mn
    return unheads(o * (1.0 / l)), (m + torch.log2(l)).squeeze(-1)


def mfma_pairs(n):
    """the order in which a chain of 32x32x2 MFMA steps contracts n (a multiple of 8) indices: pairs (i, i + 4), i = 0..3 of each group of
    eight (mfma_rows_x_frags over the head dimension; acc_row over the keys of a tile)"""
    return [(8 * g + x, 8 * g + x + 4) for g in range(n // 8) for x in range(4)]


def _fma(a, b, c):
    """fp32 fma(a, b, c): the product is exact in fp64 and the sum is rounded there once more before the rounding to fp32"""
    return (a.double() * b.double() + c.double()).float()


def restate_fwd_sequential(ops, device="cpu", fused=False, tree=False):
    """the forward in the kernels' ORDER, every operation a separate fp32 rounding (elementwise torch only: the same bits on every
    machine): scores accumulated over the head dimension two products per step, the online softmax over trips of 64 keys, the row sum
    register by register per half wave, O accumulated two keys per step.  What the matrix cores do inside a step is not documented; this
    is the order of the steps.  It gives the yardstick the rounding the blocked sums of a CPU matrix product do not have: at N = 1 lse
    is the score itself, and a long row of equal probabilities (flat) or of equal-signed values (offset-v) sums 144 partial sums one
    after the other.  fused: a step is two chained fma (the products are not rounded); tree: the scores in the one-query kernels'
    order instead (dot4 of four neighbours, then a butterfly over the dh / 4 lanes of a key)."""
    H, N, dh = ops.H, ops.N, ops.dh
    q, k, v = split(ops.qkv.to(device), H)
    pad = (-N) % 64
    k, v = torch.nn.functional.pad(k, (0, 0, 0, pad)), torch.nn.functional.pad(v, (0, 0, 0, pad))
    qs = q * _f32(qscale32(dh)).to(device)
    s = torch.zeros(q.shape[:-1] + (N + pad,), device=device)
    if tree:
        pr = qs[..., :, None, :] * k[..., None, :, :]
        part = (pr[..., 0::4] + pr[..., 1::4]) + (pr[..., 2::4] + pr[..., 3::4])
        while part.shape[-1] > 1:
            half = part.shape[-1] // 2
            part = part[..., :half] + part[..., half:]
        s = part[..., 0]
    else:
        for d0, d1 in mfma_pairs(dh):
            a0, b0, a1, b1 = qs[..., :, None, d0], k[..., None, :, d0], qs[..., :, None, d1], k[..., None, :, d1]
            s = _fma(a1, b1, _fma(a0, b0, s)) if fused else s + a0 * b0 + a1 * b1
    s[..., N:] = -INF
    mf = _mask_of(ops, None).to(device) if ops.keep < 1 else None
    m = torch.full(s.shape[:-1] + (1,), -INF, device=device)
    l, o = torch.zeros_like(m), torch.zeros(q.shape, device=device)
    for t in range((N + pad) // 64):
        st = s[..., 64 * t:64 * t + 64]
        mn = torch.maximum(m, st.amax(-1, keepdim=True))
        alpha = torch.exp2(m - mn)
        p = torch.exp2(st - mn)
        ts = [torch.zeros_like(m), torch.zeros_like(m)]
        for r in range(16):
            for h in range(2):
                i = (r & 3) + 8 * (r >> 2) + 4 * h
                ts[h] = ts[h] + (p[..., i:i + 1] + p[..., i + 32:i + 33])
        l = l * alpha + (ts[0] + ts[1])
        if mf is not None:
            p = p * torch.nn.functional.pad(mf, (0, pad))[..., 64 * t:64 * t + 64]
        if t > 0:
            o = o * alpha
        for half in (0, 32):
            for i0, i1 in mfma_pairs(32):
                j0, j1 = 64 * t + half + i0, 64 * t + half + i1
                if j0 >= N:
                    continue
                p0, v0, p1, v1 = p[..., half + i0, None], v[..., None, j0, :], p[..., half + i1, None], v[..., None, j1, :]
                o = _fma(p1, v1, _fma(p0, v0, o)) if fused else o + p0 * v0 + p1 * v1
        m = mn
    return unheads(o * (1.0 / l)).cpu(), (m + torch.log2(l)).squeeze(-1).cpu()


def restate_bwd(ops, out, lse, defect=None):
    """the gradient as the kernels form it: P = exp2(s - lse) and dP in fp32, delta from the fp32 `out` it is given, rows >= nq without
    a gradient.  -> dqkv (B, N, 3 I); rows >= nq of dq are zero here (the kernels leave them alone)"""
    H, N, dh, nq = ops.H, ops.N, ops.dh, ops.nq
    q, k, v = split(ops.qkv, H)
    do, o = heads(ops.dout, H)[:, :, :nq], heads(out, H)[:, :, :nq]
    sc = _f32(scale32(dh))
    s = (q[:, :, :nq] * _f32(qscale32(dh))) @ k.transpose(-1, -2)
    P = torch.exp2(s - lse[..., :nq, None])
    if defect == "bwd_drop_last":
        P[..., -1] = 0.0
    dP = do @ v.transpose(-1, -2)
    Pd = P
    if ops.keep < 1:
        mf = _mask_of(ops, defect)[:, :, :nq]
        if defect == "bwd_mask_differs":
            mf = (attention_mask(ops.B, H, N, ops.keep, seed=DROP_SEED + 1).float() * (_f32(1.0) / _f32(ops.keep)))[:, :, :nq]
        dP, Pd = dP * mf, P * mf
    delta = (do * o).sum(-1, keepdim=True)
    dS = P * (dP if defect == "no_delta" else dP - delta) * sc
    dq, dk, dv = dS @ k, dS.transpose(-1, -2) @ q[:, :, :nq], Pd.transpose(-1, -2) @ do
    if defect == "no_scale_dk":
        dk = dk / sc
    if defect == "dq_scaled_twice":
        dq = dq * sc
    dq = torch.nn.functional.pad(dq, (0, 0, 0, N - nq))
    return join(dq, dk, dv)


def restate_bwd_sequential(ops, out, lse, device="cpu"):
    """the gradient in the two-phase kernel's order of steps, every step two chained fma (restate_fwd_sequential, fused): S and dP over
    the head dimension; dq over the keys from P = exp2(S' - lse) with the pre-scaled q; dk and dv over the queries from
    P = exp2((q . k) qscale - lse), the second orientation's own recomputation; delta as the two half-wave sums of rounded products.
    Elementwise torch only: the same bits on every machine.  -> dqkv (B, N, 3 I), rows >= nq of dq zero"""
    H, N, dh, nq = ops.H, ops.N, ops.dh, ops.nq
    q, k, v = split(ops.qkv.to(device), H)
    q = q[:, :, :nq]
    do, o, lq = heads(ops.dout.to(device), H)[:, :, :nq], heads(out.to(device), H)[:, :, :nq], lse.to(device)[..., :nq, None]
    sc, qsc = _f32(scale32(dh)).to(device), _f32(qscale32(dh)).to(device)
    qs = q * qsc
    s1 = torch.zeros(q.shape[:-1] + (N,), device=device)
    s2, dp = torch.zeros_like(s1), torch.zeros_like(s1)
    for d0, d1 in mfma_pairs(dh):
        k0, k1 = k[..., None, :, d0], k[..., None, :, d1]
        s1 = _fma(qs[..., :, None, d1], k1, _fma(qs[..., :, None, d0], k0, s1))
        s2 = _fma(q[..., :, None, d1], k1, _fma(q[..., :, None, d0], k0, s2))
        dp = _fma(do[..., :, None, d1], v[..., None, :, d1], _fma(do[..., :, None, d0], v[..., None, :, d0], dp))
    pr = do * o
    dsum = [torch.zeros_like(lq), torch.zeros_like(lq)]
    for g in range(dh // 8):
        for h in range(2):
            c = 8 * g + 4 * h
            dsum[h] = dsum[h] + ((pr[..., c:c + 1] + pr[..., c + 1:c + 2]) + (pr[..., c + 2:c + 3] + pr[..., c + 3:c + 4]))
    delta = dsum[0] + dsum[1]
    P1, P2 = torch.exp2(s1 - lq), torch.exp2(s2 * qsc - lq)
    Pd = P2
    if ops.keep < 1:
        mf = _mask_of(ops, None).to(device)[:, :, :nq]
        dp, Pd = dp * mf, P2 * mf
    dS1, dS2 = P1 * (dp - delta) * sc, P2 * (dp - delta) * sc
    dq = torch.zeros(q.shape, device=device)
    dk, dv = torch.zeros(k.shape, device=device), torch.zeros(k.shape, device=device)
    for base in range(0, N, 32):
        for i0, i1 in mfma_pairs(32):
            j0, j1 = base + i0, min(base + i1, N - 1)
            if j0 >= N:
                continue
            w1 = dS1[..., j1, None] if base + i1 < N else torch.zeros_like(dS1[..., j0, None])
            dq = _fma(w1, k[..., None, j1, :], _fma(dS1[..., j0, None], k[..., None, j0, :], dq))
    for base in range(0, nq, 32):
        for i0, i1 in mfma_pairs(32):
            for i in (base + i0, base + i1):
                if i < nq:
                    dv = _fma(Pd[..., i, :, None], do[..., i, None, :], dv)
                    dk = _fma(dS2[..., i, :, None], q[..., i, None, :], dk)
    dq = torch.nn.functional.pad(dq, (0, 0, 0, N - nq))
    return join(dq, dk, dv).cpu()


@functools.lru_cache(maxsize=8)
def backward_inputs(p):
    """the `out` and `lse` a backward case is given: the restated forward's, so that a backward case does not depend on a forward
    kernel (all N rows; the GPU file poisons the rows >= nq)"""
    assert p.op == "bwd"
    return restate_fwd(operands(p))


# name -> (op, classes it must be caught on, smallest N, how it is stated, needs dropout)
#   * pad_key: a zero-score key weighs e^-max: below 2^-24 of the row in moving-max and nothing at all in select / tie
#   * no_rescale: the maximum of tie is in the first pair of tiles for some rows only by chance; of select and the others it moves
#   * swap_tiles: by select, which is what it is for (the bounds need not see it, and tie's pairs can sit symmetrically)
#   * drop_last: tie's odd last key is the unpaired one, which no row selects
#   * no_scale_dk, dq_scaled_twice: dq and dk are exactly zero in select and tie; token0's dq has one row, its dk every row
#   * no_log2e, lse_nat: the exact classes see them in lse (select) or not at all in `out` (tie: out is exact whatever the base), so tie
#     is judged on lse by the rule
#   * frame_k / head_v / stale_k on tie and select: another item's codes select nothing or something else
ALL = FWD_CLASSES
NUMERIC = ("gauss", "moving-max", "flat", "offset-v")
Defect = namedtuple("Defect", "name op classes min_n online drop")
DEFECTS = (
    Defect("drop_last", "fwd", ALL, 2, False, False),
    Defect("pad_key", "fwd", ("gauss", "flat", "offset-v"), 1, False, False),
    Defect("no_log2e", "fwd", ALL, 1, False, False),
    Defect("no_rescale", "fwd", NUMERIC + ("select",), 65, True, False),
    Defect("swap_tiles", "fwd", ("select",), 33, True, False),
    Defect("head_v", "fwd", ALL, 1, False, False),
    Defect("frame_k", "fwd", ALL, 1, False, False),
    Defect("stale_k", "fwd", ALL, 1, False, False),
    Defect("lse_nat", "fwd", ALL, 1, False, False),
    Defect("lse_nomax", "fwd", ALL, 1, False, False),
    Defect("no_delta", "bwd", BWD_CLASSES, 1, False, False),
    Defect("no_scale_dk", "bwd", NUMERIC + ("token0",), 2, False, False),
    Defect("dq_scaled_twice", "bwd", NUMERIC + ("token0",), 2, False, False),
    Defect("bwd_drop_last", "bwd", BWD_CLASSES, 2, False, False),
    Defect("no_inv_keep", "fwd", NUMERIC, 1, False, True),
    Defect("mask_transposed", "fwd", NUMERIC, 2, False, True),
    Defect("mask_stride", "fwd", NUMERIC, 5, False, True),
    Defect("mask_other_layer", "fwd", NUMERIC, 1, False, True),
    Defect("lse_dropped", "fwd", NUMERIC, 1, False, True),
    Defect("no_inv_keep", "bwd", NUMERIC, 1, False, True),
    Defect("mask_transposed", "bwd", NUMERIC, 2, False, True),
    Defect("mask_stride", "bwd", NUMERIC, 5, False, True),
    Defect("bwd_mask_differs", "bwd", NUMERIC, 1, False, True),
)


def defect_applies(d, p):
    if d.op != p.op or p.cls not in d.classes or p.N < d.min_n or d.drop != (p.keep < 1):
        return False
    if d.name == "bwd_drop_last" and p.nq < p.N:
        return False                                  # the last key may weigh nothing in the few rows < nq (select: selected by none)
    if (d.name == "head_v" and p.H < 2) or (d.name == "frame_k" and p.B < 2) or (d.name == "stale_k" and p.B * p.H < 2):
        return False                                  # no neighbour to take the operand from
    if d.name == "no_rescale" and p.cls in ("gauss", "flat", "offset-v") and p.N < 96:
        return False                                  # a second trip of one key: it must be a row's maximum to be seen
    if d.name == "pad_key":
        return p.N % 32 != 0
    if d.name == "mask_stride":
        return p.N % 4 != 0
    if d.name in ("drop_last", "bwd_drop_last") and p.cls == "tie":
        return p.N % 2 == 0
    return True


# ------------------------------------------------------------------------------------------------ the rule
def ulp_f32(x):
    _, e = torch.frexp(x.double().abs())
    return torch.where(x == 0, torch.zeros((), dtype=torch.float64, device=x.device), torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 1 - 23))


def floor_of(name, ref, mass):
    return LSE_FLOOR_ULPS * ulp_f32(ref) if name == "lse" else ulp_f32(ref) + mass


def _worst(num, den):
    t = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num == 0, 0.0, INF))
    t = torch.where(torch.isnan(t), torch.full_like(t, INF), t)
    return float(t.max()) if t.numel() else 0.0


def distance(got, ref, mass):
    """largest |got - ref| / mass; a NaN or an error at an element of mass 0 is infinite"""
    return _worst((got.double().to(ref.device) - ref).abs(), mass)


def tightness(name, got, ref, mass, Y):
    """largest |got - ref| / max(MARGIN Y mass, FLOOR): the element passes the rule at <= 1"""
    return _worst((got.double().to(ref.device) - ref).abs(), torch.maximum(MARGIN * Y * mass, floor_of(name, ref, mass)))


def split_dqkv(dqkv, H):
    I = dqkv.shape[-1] // 3
    return {"dq": dqkv[..., :I], "dk": dqkv[..., I:2 * I], "dv": dqkv[..., 2 * I:]}


def rows(x, name, nq):
    """the rows that exist: rows < nq of out, lse and dq (out, dq: (B, N, I); lse: (B, H, N)); every row of dk and dv"""
    if name not in QUERY_ROWS:
        return x
    return x[..., :nq] if name == "lse" else x[:, :nq]


@functools.lru_cache(maxsize=8)
def cpu_reference(p):
    return reference(operands(p))


def restated(p, defect=None, online=False, sequential=None, device="cpu"):
    """sequential: None, "rounded", "fused" or "tree" (restate_fwd_sequential)"""
    ops = operands(p)
    if p.op == "fwd" and sequential:
        assert defect is None
        return dict(zip(FWD_OUTPUTS, restate_fwd_sequential(ops, device, fused=sequential == "fused", tree=sequential == "tree")))
    if p.op == "fwd":
        return dict(zip(FWD_OUTPUTS, (restate_fwd_online if online else restate_fwd)(ops, defect)))
    if sequential:
        assert defect is None
        return split_dqkv(restate_bwd_sequential(ops, *backward_inputs(p), device), p.H)
    return split_dqkv(restate_bwd(ops, *backward_inputs(p), defect), p.H)


def backward_forms(p, device="cpu"):
    return {"whole-row": restated(p), "step order, fused": restated(p, sequential="fused", device=device)}


def forms_of(p, device="cpu"):
    return forward_forms(p, device) if p.op == "fwd" else backward_forms(p, device)


def forward_forms(p, device="cpu"):
    """the honest restatements of a forward problem, by name"""
    forms = {"whole-row": restated(p)}
    forms.update({"step order, " + kind: restated(p, sequential=kind, device=device) for kind in ("rounded", "fused", "tree")})
    if p.keep == 1:
        forms["key-tile-sequential"] = restated(p, online=True)
    return forms


def yardsticks(p, ref=None, nq=None):
    """Y per output of the problem, from the restatement alone: the largest over the whole-row form, in the forward the
    key-tile-sequential one (undropped), and the ones in the kernels' order of steps -- all honest orders of the same products; the
    last run on the device of `ref` (elementwise fp32: the same bits as on the CPU)"""
    ref = cpu_reference(p) if ref is None else ref
    nq = p.nq if nq is None else nq
    forms = list(forms_of(p, ref["out"][0].device).values())
    return {k: max(distance(rows(f[k], k, nq), rows(ref[k][0].cpu(), k, nq), rows(ref[k][1].cpu(), k, nq)) for f in forms) for k in forms[0]}


def judge(p, got, ref=None, Y=None, nq=None):
    """{output: (tightness, distance, Y)} of the kernel's (or a defect's) outputs `got` against the rule; passes when every tightness <= 1"""
    ref = cpu_reference(p) if ref is None else ref
    nq = p.nq if nq is None else nq
    Y = yardsticks(p, ref, nq) if Y is None else Y
    res = {}
    for k, g in got.items():
        r, m = (rows(t, k, nq) for t in ref[k])
        res[k] = (tightness(k, rows(g, k, nq), r, m, Y[k]), distance(rows(g, k, nq), r, m), Y[k])
    return res


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


def exact_violations(p, got, nq=None):
    """the exact promises of select / tie that `got` breaks (names of outputs): out and lse bit for bit; dq, dk and dv as numbers (a zero
    of dv is 0 x dout, of either sign)"""
    if p.cls not in EXACT_CLASSES:
        return []
    nq = p.nq if nq is None else nq
    bad = []
    for k, e in select_expect(operands(p), p).items():
        if k not in got:
            continue
        g, e = rows(got[k].detach().cpu(), k, nq), rows(e, k, nq)
        ok = bool((g == 0).all()) if k in ("dq", "dk") else bool((g == e).all()) if k == "dv" else same_bits(g, e)
        if not ok:
            bad.append(k)
    return bad


def rows_kept(after, before, nq, name):
    """nq < N: rows >= nq of out / lse / dq hold the bits they held before the call"""
    a, b = (after[..., nq:], before[..., nq:]) if name == "lse" else (after[:, nq:], before[:, nq:])
    return same_bits(a, b)


def clear_caches():
    for f in (operands, backward_inputs, cpu_reference):
        f.cache_clear()
