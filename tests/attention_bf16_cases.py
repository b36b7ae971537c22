"""The bf16 attention matrix: case table, dispatch restated, data classes, fp64 reference, error masses, CPU yardstick, rule and defects.

Shared by tests/test_attention_bf16_matrix_host.py (CPU: everything here is checked against itself) and
tests/test_gpu_attention_bf16_matrix.py (the kernels of csrc/attention_bf16.hip and csrc/attention_bf16_long.hip against the
reference).  Nothing here touches a GPU; the reference and the masses run on whatever device their operands are on, so the GPU file
may evaluate the many-item problems in torch fp64 on the device (one of them is compared with the CPU result there).

Layout: qkv (B, N, 3 H 64) bf16 = [q | k | v], head h in columns 64 h .. 64 h + 63 of each third; out (B, N, H 64) bf16; lse (B, H, N)
fp32, base 2; dqkv like qkv; delta (B H N) fp32 = rowsum(dout o out).

The rule.  u = 2^-8 is the unit roundoff of bf16 (8 significant bits, round to nearest even), v = 2^-24 that of fp32.  Every output
element has an error MASS: the first-order size of what the rounding points the kernels have by design can do to it, with S the scaled
scores (natural units), P = softmax(S), A_ij = sum_d |q_id k_jd| / 8:
  * scores in fp32 and the exponent: a probability's numerator carries e_ij = A_ij + |S_ij - max_i| + 1 units of v (the sum of
    products, the one rounding of the scaled difference, exp2); the backward recomputes P from the fp32 lse, which adds
    ln2 (|S2_ij| + |lse_i|) v for the two roundings of the difference of two large base-2 numbers, and ln2 mass(lse_i) for the lse;
  * probabilities rounded to bf16 before P V: u sum_j P_ij |V_jd|;
  * one bf16 rounding of each stored output: u |out_id|, u |dq|, u |dk|, u |dv|;
  * fp32 accumulation of every product: v times the sum of absolute products;
  * delta from the bf16 `out`: mass(delta_i) = sum_d |dout_id| mass(out_id) + v sum_d |dout_id out_id|, which enters dS as
    P_ij mass(delta_i) / 8 -- present in every class, it is the leading term of `offset-v`, where dP - delta cancels two numbers of
    size 100 sum|dout| (no class needs a term the others do not have);
  * dS and P as bf16 operands of the gradient products: u |dS_ij|, u P_ij;
  * lse in fp32: v (log2e sum_j P_ij e_ij + 2 |lse_i| + |max2_i| + 1).
  (sum_j P_ij e_ij |V_jd - out_id| is bounded by (P e) |V| + rowsum(P e) |out| so that no N x N x 64 tensor is needed; it multiplies v.)
The YARDSTICK Y of a case and an output is the largest |restatement - fp64| / mass over the output's elements, where the restatement
(restate_fwd, restate_bwd) is plain torch fp32 on the CPU with these rounding points and nothing else of the kernels: whole-row
softmax, no tiles, no swizzles, no deferred rescale.  A kernel element passes when
        |got - fp64| <= max(MARGIN * Y * mass, FLOOR),      MARGIN = 2,
for every element, with no exclusions; a NaN never passes.  MARGIN is for the summation order and for the rounding flips the
restatement cannot share with the kernel.  FLOOR is the unit cost of exactly those.  A stored bf16 value is RN(x) of an fp32 x; kernel
and restatement hold x's that differ by summation order, so their stored values differ by 0 or by one step of the bf16 grid at that
value, and the fp64 value lies within half a step of one of them: one bf16 ulp of the reference value, 2^(floor(log2 |ref|) - 7)
(0 at ref = 0: an exact zero has no flip).  And two honest fp32 sums of the same products in two orders differ by up to v times the sum
of the absolute products: the fp32 part of the mass (the mass with u = 0).  It is 2^-16 of the rest except where the reference cancels
to nothing -- N = 1, where dq and dk are (dP - delta) k / 8 with dP and delta two such sums of the 64 products dout o V, one on the
matrix cores and one lane-sequential: the kernels leave a few 1e-7 there, the restatement on one CPU as much and on another possibly 0,
so a bound made of Y alone would be luck.  FLOOR = that ulp + the fp32 part of the mass.  lse is m + log2(l) in fp32: the maximum's product, log2's result
and the sum are each within one fp32 ulp of a number of lse's size, and the restatement's scaled difference is not fused: FLOOR =
LSE_FLOOR_ULPS = 4 fp32 ulps of the reference value.  The floor never exceeds the mass (u (sum P |V| + |out|) >= 2 u |out| >= ulp).

Data classes: gauss; moving-max (q x 4 and the keys of one 32-key tile x 6; the tile is the first, a middle, the last full and the
partial last one in turn over the items of a problem); flat (q x 2^-6); offset-v (V = 100 + N(0, 1)); token0 (backward: dout is zero
outside row 0); and three constructed classes in which a property is exact:
  * select: q_i = 16 code(pi(i)), k_j = 16 code(j), codes of 64 random signs per item: the selected base-2 logit is 2^14 sc exactly and
    leads every other by more than 200 (asserted; about 1300 in practice), so every other probability is an fp32 zero, every rescale of
    junk accumulated before the selected key multiplies by an exact zero, and out[i] == V[pi(i)], lse == fp32(2^14 sc), dv[j] ==
    dout[pi^-1(j)] bit for bit and dq == dk == 0 (dout and V are small integers in the backward so that dP == delta exactly).
  * tie: select with every code shared by two keys (an odd last key has its own and is never selected): p = 1, 1, l = 2, and out[i] ==
    RN_bf16((V_a + V_b) / 2) bit for bit, a value that is in general NOT representable: the one exact check of the store's rounding mode.
  * near-tie: q = (a, 0, ...), even keys (1, 0, ...), odd keys (1 - 2^-8, 0, ...): the odd probabilities are 1 - 1.2e-4 and round to 1,
    V = +c on even and -15/16 c on odd keys (c of two significant bits: every partial sum of P V is exact in fp32), so the honest P V
    cancels to c / 32 and the honest error is a few hundredths of the mass, while probabilities truncated to bf16 leave another c 2^-9:
    half the mass.  (Truncation errs at most twice what rounding does, element by element: without this class the factor 2 of the
    rule would admit it.)
"""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

DH = 64
U = 2.0 ** -8
V32 = 2.0 ** -24
MARGIN = 2.0
LSE_FLOOR_ULPS = 4
LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
SC32 = float(np.float32(0.125) * np.float32(LOG2E))        # the kernels' sc = scale * log2(e), a power of two times fp32(log2 e)
SELECT_LSE = float(np.float32(16384.0) * np.float32(SC32))  # exact in fp32
INF = float("inf")

FWD_CLASSES = ("gauss", "moving-max", "flat", "tie", "near-tie", "offset-v", "select")
BWD_CLASSES = FWD_CLASSES + ("token0",)
EXACT_CLASSES = ("select", "tie")
FWD_OUTPUTS = ("out", "lse")
BWD_OUTPUTS = ("dq", "dk", "dv")

# ------------------------------------------------------------------------------------------------ the dispatch, restated
FWD_KERNELS = ("item4", "item8", "item9", "stream", "stream288", "tiled8", "tiled4", "tiled_drop")
BWD_KERNELS = ("dq8+dkv", "dq9+dkv", "tiled8", "tiled4", "tiled_drop")
LONG_DEFAULT, WAVES_DEFAULT = 3, 8          # csrc/knobs.h: g_attn_bf16_long, g_attn_bf16_tiled_waves
PERSIST_ITEMS = 512

# op: "fwd" | "bwd"; entry: "short" (attention_fwd_bf16 / attention_bwd_bf16), "tiled", "tiled_drop" (keep = 1); long / waves: the value
# given to dgvit_set_attention_bf16_long / _tiled_waves, None = left at the default; lse: a non-NULL lse (forward)
Case = namedtuple("Case", "op entry cls B N H nq lse long waves")


def case_id(c):
    s = f"{c.op}-{c.entry}-{c.cls}-B{c.B}H{c.H}N{c.N}"
    if c.op == "fwd":
        s += (f"-nq{c.nq}" if c.nq != c.N else "") + ("" if c.lse else "-nolse")
    return s + (f"-long{c.long}" if c.long is not None else "") + (f"-w{c.waves}" if c.waves is not None else "")


def kernel_reached(c):
    """the kernel(s) that attention_fwd_bf16 / attention_bwd_bf16 / fwd_tiled / bwd_tiled launch for the case"""
    long_bits = LONG_DEFAULT if c.long is None else c.long & 3
    waves = WAVES_DEFAULT if c.waves not in (4, 8) else c.waves
    if c.entry == "tiled":
        return f"tiled{waves}"
    if c.entry == "tiled_drop":
        return "tiled_drop"                      # keep = 1: the plain kernels behind the _drop entry points' own checks
    assert c.entry == "short" and 1 <= c.N <= 288
    nkt, items = (c.N + 31) // 32, c.B * c.H
    if c.op == "bwd":
        return "dq9+dkv" if nkt * 32 > 256 and long_bits & 2 else "dq8+dkv"
    if c.N <= 224 and nkt > 4 and items >= PERSIST_ITEMS:
        return "stream"
    if c.N > 224 and long_bits & 1 and items >= PERSIST_ITEMS:
        return "stream288"
    nqt = (c.nq + 31) // 32
    return "item9" if nqt > 8 and long_bits & 2 else ("item8" if nqt > 4 else "item4")


def items_per_workgroup(c, cus):
    """(fewest, most) items a persistent workgroup walks"""
    items = c.B * c.H
    grid = min(items, cus)
    return items // grid, -(-items // grid)


# ------------------------------------------------------------------------------------------------ the case table
ITEM4_N = (1, 2, 31, 32, 33, 64, 65, 96, 127, 128)
ITEM8_N = (129, 160, 161, 197, 224, 225, 255, 256)
ITEM8_LONG0_N = (257, 288)
ITEM9_N = (257, 287, 288)
STREAM_N = (129, 160, 161, 197, 223, 224)
STREAM288_N = (225, 256, 257, 287, 288)
TILED_N = (1, 33, 127, 128, 129, 255, 256, 257, 289, 321, 513)
BWD_SHORT_N = (1, 32, 33, 64, 65, 128, 129, 160, 161, 224, 225, 256)      # the item Ns thinned to the tile boundaries, and N = 1
LISTED_N = {
    ("fwd", "item4"): ITEM4_N, ("fwd", "item8"): ITEM8_N + ITEM8_LONG0_N, ("fwd", "item9"): ITEM9_N, ("fwd", "stream"): STREAM_N,
    ("fwd", "stream288"): STREAM288_N, ("fwd", "tiled8"): TILED_N, ("fwd", "tiled4"): TILED_N, ("fwd", "tiled_drop"): TILED_N,
    ("bwd", "dq8+dkv"): BWD_SHORT_N + ITEM8_LONG0_N, ("bwd", "dq9+dkv"): ITEM9_N, ("bwd", "tiled8"): TILED_N, ("bwd", "tiled4"): TILED_N,
    ("bwd", "tiled_drop"): TILED_N,
}
IB, IH = 2, 3          # item paths: frame and head strides both matter
TB, TH = 2, 2          # tiled paths


def factor_items(n):
    """(B, H) with B * H == n and H a small odd number where n has such a divisor"""
    for h in (3, 5, 7, 9, 11, 13, 15, 17, 19):
        if n % h == 0:
            return n // h, h
    return n, 1


def classes_of(cls_list, N):
    # tie needs a pair of keys
    return tuple(k for k in cls_list if not (k == "tie" and N < 2))


@functools.lru_cache(maxsize=None)
def all_cases(cus=256):
    out = []

    def fwd(entry, cls, B, N, H, nq=None, lse=True, long=None, waves=None):
        out.append(Case("fwd", entry, cls, B, N, H, N if nq is None else nq, lse, long, waves))

    def bwd(entry, cls, B, N, H, long=None, waves=None):
        out.append(Case("bwd", entry, cls, B, N, H, N, True, long, waves))

    # ---- forward, per-item kernels
    for N in ITEM4_N + ITEM8_N:
        for cls in classes_of(FWD_CLASSES, N):
            fwd("short", cls, IB, N, IH)
    for N in ITEM8_LONG0_N:
        for cls in FWD_CLASSES:
            fwd("short", cls, IB, N, IH, long=0)
    for N in ITEM9_N:
        for cls in FWD_CLASSES:
            fwd("short", cls, IB, N, IH)
    for N, long in ((33, None), (128, None), (129, None), (197, None), (256, None), (288, 0)):        # nq < N on item4 and item8
        for nq in (1, 33):
            for cls in ("gauss", "select"):
                fwd("short", cls, IB, N, IH, nq=nq, long=long)
    for N, long in ((1, None), (128, None), (129, None), (256, None), (288, 0), (288, None)):          # lse NULL
        for cls in ("gauss", "select"):
            fwd("short", cls, IB, N, IH, lse=False, long=long)
    # ---- forward, persistent kernels: 512, 2 C + 1 and 3 C - 1 items at every N; 511 items (the per-item kernels) at the ends of each range
    many = [(128, 4)] + [factor_items(n) for n in (2 * cus + 1, 3 * cus - 1)]
    for fam, rich in ((STREAM_N, 197), (STREAM288_N, 257)):
        for N in fam:
            for cls in FWD_CLASSES if N in (fam[0], rich, fam[-1]) else ("gauss", "select"):
                fwd("short", cls, 128, N, 4)
        for B, H in many[1:]:
            for N in fam:
                for cls in ("gauss", "select"):
                    fwd("short", cls, B, N, H)
        for N in (fam[0], fam[-1]):
            fwd("short", "select", 73, N, 7)
        fwd("short", "gauss", 73, fam[-1], 7)
        for nq in (1, 33):
            for cls in ("gauss", "select"):
                fwd("short", cls, 128, rich, 4, nq=nq)
        for cls in ("gauss", "select"):
            fwd("short", cls, 128, fam[-1], 4, lse=False)
    # ---- forward, tiled
    for waves in (8, 4):
        for N in TILED_N:
            for cls in classes_of(FWD_CLASSES, N):
                fwd("tiled", cls, TB, N, TH, waves=waves)
        for N in (33, 129, 257, 513):
            for nq in (1, 33):
                for cls in ("gauss", "select"):
                    fwd("tiled", cls, TB, N, TH, nq=nq, waves=waves)
        for cls in ("gauss", "select"):
            fwd("tiled", cls, TB, 257, TH, lse=False, waves=waves)
    for N in TILED_N:
        for cls in ("gauss", "select"):
            fwd("tiled_drop", cls, TB, N, TH)
    fwd("tiled_drop", "gauss", TB, 257, TH, nq=1)
    fwd("tiled_drop", "gauss", TB, 257, TH, lse=False)
    # ---- backward
    for N in BWD_SHORT_N:
        for cls in classes_of(BWD_CLASSES, N):
            bwd("short", cls, IB, N, IH)
    for N in ITEM8_LONG0_N:
        for cls in BWD_CLASSES:
            bwd("short", cls, IB, N, IH, long=0)
    for N in ITEM9_N:
        for cls in BWD_CLASSES:
            bwd("short", cls, IB, N, IH)
    for waves in (8, 4):
        for N in TILED_N:
            for cls in classes_of(BWD_CLASSES, N):
                bwd("tiled", cls, TB, N, TH, waves=waves)
    for N in TILED_N:
        for cls in ("gauss", "select"):
            bwd("tiled_drop", cls, TB, N, TH)
    return tuple(dict.fromkeys(out))      # (nq = 33 at N = 33 is the dense case again)


Problem = namedtuple("Problem", "op cls B N H")        # operands without their path


def problem(c):
    return Problem(c.op, c.cls, c.B, c.N, c.H)


# ------------------------------------------------------------------------------------------------ operands per data class
Operands = namedtuple("Operands", "qkv dout B N H meta")     # qkv, dout: CPU bf16; meta: the class's construction (pi, pairs, ...)


def _gen(p, salt=0):
    return torch.Generator().manual_seed(zlib.crc32(repr((tuple(p), salt)).encode()))


def _bf(x):
    return x.float().to(torch.bfloat16)


def heads(x, H):
    B, N, _ = x.shape
    return x.reshape(B, N, H, DH).permute(0, 2, 1, 3)


def unheads(x):
    B, H, N, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, N, H * DH)


def split(qkv, H):
    I = H * DH
    return heads(qkv[..., :I], H), heads(qkv[..., I:2 * I], H), heads(qkv[..., 2 * I:], H)


def join(q, k, v):
    return torch.cat([unheads(q), unheads(k), unheads(v)], dim=-1).contiguous()


def moving_max_tile(N, pos):
    """the 32-key tile that `moving-max` scales for position 0..3 (first, middle, last full, partial last)"""
    nkt, full = (N + 31) // 32, N // 32
    return (0, nkt // 2, max(full - 1, 0), nkt - 1)[pos % 4]


def _codes(g, B, H, N):
    return (torch.randint(0, 2, (B, H, N, DH), generator=g) * 2 - 1).float()


def _perms(g, B, H, n):
    return torch.stack([torch.randperm(n, generator=g) for _ in range(B * H)]).reshape(B, H, n)


@functools.lru_cache(maxsize=16)
def operands(p):
    """the operands of a problem, by its class; deterministic in the problem"""
    g = _gen(p)
    B, N, H = p.B, p.N, p.H
    I = H * DH
    meta = {}
    q, k, v = (torch.randn(B, H, N, DH, generator=g) for _ in range(3))
    dout = torch.randn(B, N, I, generator=g)
    if p.cls == "moving-max":
        q = q * 4.0
        for it in range(B * H):
            t = moving_max_tile(N, it)
            k[it // H, it % H, 32 * t:32 * t + 32] *= 6.0
    elif p.cls == "flat":
        q = _bf(q).float() * 2.0 ** -6
    elif p.cls == "offset-v":
        v = v + 100.0
    elif p.cls == "token0":
        dout[:, 1:] = 0.0
    elif p.cls in ("select", "tie"):
        code = _codes(g, B, H, N)
        if p.cls == "select":
            pi = _perms(g, B, H, N)
            groups = None
        else:
            npair = N // 2
            code[:, :, npair:2 * npair] = code[:, :, :npair]
            sig = _perms(g, B, H, npair)
            pi = torch.gather(sig, 2, (torch.arange(N) % npair).expand(B, H, N))       # query i selects the pair pi(i), pi(i) + npair
            meta["npair"] = npair
            v = torch.sign(v) * v.abs().clamp(2.0 ** -6, 8.0)                          # V_a + V_b is exact in fp32
        k = 16.0 * code
        q = 16.0 * torch.gather(code, 2, pi[..., None].expand(B, H, N, DH))
        meta["pi"] = pi
        if p.op == "bwd":                                                               # dP == delta exactly on small integers
            v = torch.randint(-4, 5, (B, H, N, DH), generator=g).float()
            dout = torch.randint(-3, 4, (B, N, I), generator=g).float()
        _assert_selected(q, k, pi, meta.get("npair"))
    elif p.cls == "near-tie":
        a = torch.where(torch.arange(N) % 2 == 0, 0.25, 0.125)
        q = torch.zeros(B, H, N, DH)
        q[..., 0] = a
        k = torch.zeros(B, H, N, DH)
        k[..., 0] = torch.where(torch.arange(N) % 2 == 0, 1.0, 1.0 - 2.0 ** -8)
        c = torch.tensor([0.5, 0.75, 1.0, 1.5, 2.0, 3.0])[torch.randint(0, 6, (B, H, 1, DH), generator=g)]
        v = c * torch.where(torch.arange(N) % 2 == 0, 1.0, -(1.0 - 2.0 ** -4))[None, None, :, None]
    else:
        assert p.cls == "gauss", p.cls
    return Operands(_bf(join(q, k, v)), _bf(dout) if p.op == "bwd" else None, B, N, H, meta)


def _assert_selected(q, k, pi, npair):
    """fp64: everything but the selected key (or pair) of a row has a softmax weight below 2^-200"""
    s2 = (q.double() @ k.double().transpose(-1, -2)) * (0.125 * LOG2E)
    N = s2.shape[-1]
    sel = torch.zeros_like(s2, dtype=torch.bool).scatter_(-1, pi[..., None], True)
    if npair is not None:
        sel.scatter_(-1, (pi + npair)[..., None], True)
    top = s2.masked_fill(~sel, -INF).amax(-1)
    assert bool((s2[sel] == 16384.0 * (0.125 * LOG2E)).all()), "select / tie: a selected logit is not 2^14 sc"
    rest = s2.masked_fill(sel, -INF).amax(-1) if N > (1 if npair is None else 2) else torch.full_like(top, -INF)
    assert float((rest - top).max()) + math.log2(N) < -200.0, "select / tie: an unselected key is not negligible"


def select_expect(ops, p):
    """what the exact classes promise, as tensors in the layout of the outputs (None: no promise for that output)"""
    _, _, v = split(ops.qkv, ops.H)
    B, N, H = ops.B, ops.N, ops.H
    pi = ops.meta["pi"]
    idx = pi[..., None].expand(B, H, N, DH)
    if p.cls == "select":
        exp = {"out": unheads(torch.gather(v, 2, idx)), "lse": torch.full((B, H, N), SELECT_LSE, dtype=torch.float32)}
        if p.op == "bwd":
            do = heads(ops.dout, H)
            dv = torch.zeros_like(do).scatter_(2, idx, do)                  # dv[pi(i)] = dout[i]
            exp.update(dq=torch.zeros_like(ops.dout), dk=torch.zeros_like(ops.dout), dv=unheads(dv))
        return exp
    va, vb = torch.gather(v, 2, idx).float(), torch.gather(v, 2, (pi + ops.meta["npair"])[..., None].expand(B, H, N, DH)).float()
    return {"out": unheads(((va + vb) * 0.5).to(torch.bfloat16))}


# ------------------------------------------------------------------------------------------------ fp64 reference and masses
def reference(ops, device="cpu"):
    """fp64 forward (and gradient where the operands have a dout) with the masses of every output: {name: (ref, mass, the fp32 part of
    the mass)} in the outputs' layouts.  The gradient is the true one: of the fp64 forward, not of a rounded `out`."""
    H = ops.H
    q, k, v = split(ops.qkv.to(device).double(), H)
    S = (q @ k.transpose(-1, -2)) * 0.125
    mx = S.amax(-1, keepdim=True)
    E = torch.exp(S - mx)
    P = E / E.sum(-1, keepdim=True)
    out = P @ v
    lse = (mx + torch.log(E.sum(-1, keepdim=True))).squeeze(-1) * LOG2E
    A = (q.abs() @ k.abs().transpose(-1, -2)) * 0.125
    Pe = P * (A + (S - mx).abs() + 1.0)
    del E
    PV = P @ v.abs()
    m32_out = V32 * (Pe @ v.abs() + Pe.sum(-1, keepdim=True) * out.abs() + PV)
    m_out = U * (PV + out.abs()) + m32_out
    m_lse = V32 * (LOG2E * Pe.sum(-1) + 2.0 * lse.abs() + LOG2E * mx.squeeze(-1).abs() + 1.0)
    res = {"out": (unheads(out), unheads(m_out), unheads(m32_out)), "lse": (lse, m_lse, m_lse)}
    if ops.dout is None:
        return res
    del Pe, PV
    do = heads(ops.dout.to(device).double(), H)
    dP = do @ v.transpose(-1, -2)
    delta = (do * out).sum(-1, keepdim=True)
    dS = P * (dP - delta) * 0.125
    dq, dk, dv = dS @ k, dS.transpose(-1, -2) @ q, P.transpose(-1, -2) @ do
    ep = V32 * (A + LN2 * ((S * LOG2E).abs() + lse.abs()[..., None]) + 1.0) + LN2 * m_lse[..., None]
    AdP = do.abs() @ v.abs().transpose(-1, -2)

    def masses(u, m_out_x):
        """u = U: the whole mass; u = 0 with the fp32 part of mass(out): the fp32 part alone"""
        m_delta = (do.abs() * m_out_x).sum(-1, keepdim=True) + V32 * (do * out).abs().sum(-1, keepdim=True)
        W = (P * ep * (dP - delta).abs() + P * (V32 * AdP + m_delta)) * 0.125 + (V32 + u) * dS.abs()
        Wp = P * (ep + u + V32)
        return (unheads(W @ k.abs() + u * dq.abs()), unheads(W.transpose(-1, -2) @ q.abs() + u * dk.abs()),
                unheads(Wp.transpose(-1, -2) @ do.abs() + u * dv.abs()), m_delta.squeeze(-1))

    full, part = masses(U, m_out), masses(0.0, m32_out)
    for i, (k_, r) in enumerate((("dq", unheads(dq)), ("dk", unheads(dk)), ("dv", unheads(dv)), ("delta", delta.squeeze(-1)))):
        res[k_] = (r, full[i], part[i])
    return res


# ------------------------------------------------------------------------------------------------ the CPU restatement (and the defects)
def _trunc_bf16(x):
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def _rn_bf16(x):
    return x.to(torch.bfloat16).float()


def restate_fwd(ops, defect=None):
    """plain torch fp32 with the kernels' rounding points: fp32 scores, base-2 softmax over the whole row, P rounded to bf16 for P V only,
    one bf16 rounding of out, lse = m + log2(l) in fp32.  -> out (B, N, I) bf16, lse (B, H, N) fp32"""
    H, N = ops.H, ops.N
    q, k, v = split(ops.qkv.float(), H)
    if defect == "head_v":
        v = torch.roll(v, -1, 1)
    if defect == "frame_k":
        k = torch.roll(k, -1, 0)
    if defect == "stale_k":                          # item i > 0 computes on item i - 1's K image
        kk = k.reshape(-1, N, DH)
        k = torch.cat([kk[:1], kk[:-1]]).reshape(k.shape)
    if defect == "pad_key":                          # keys N .. NP - 1 taken into the softmax with their zero rows
        pad = (-N) % 32
        k = torch.nn.functional.pad(k, (0, 0, 0, pad))
        v = torch.nn.functional.pad(v, (0, 0, 0, pad))
    s = q @ k.transpose(-1, -2)
    if defect == "drop_last":
        s[..., -1] = -INF
    sc = torch.tensor(0.125 if defect == "no_log2e" else SC32, dtype=torch.float32)
    m = s.amax(-1, keepdim=True) * sc
    p = torch.exp2(s * sc - m)
    l = p.sum(-1, keepdim=True)
    pb = _trunc_bf16(p) if defect == "p_trunc" else _rn_bf16(p)
    o = (pb @ v) / l
    out = _trunc_bf16(o).to(torch.bfloat16) if defect == "out_trunc" else o.to(torch.bfloat16)
    lse = m + torch.log2(l)
    if defect == "lse_nat":
        lse = lse * LN2
    if defect == "lse_nomax":
        lse = torch.log2(l)
    return unheads(out), lse.squeeze(-1)


def restate_fwd_online(ops, defect=None):
    """restate_fwd with the softmax taken online over 32-key tiles (a running maximum, the accumulator rescaled when it moves): only
    here can the two tile-order defects be stated.  Without a defect it meets the rule like restate_fwd."""
    H, N = ops.H, ops.N
    q, k, v = split(ops.qkv.float(), H)
    pad = (-N) % 32
    k, v = torch.nn.functional.pad(k, (0, 0, 0, pad)), torch.nn.functional.pad(v, (0, 0, 0, pad))
    nkt = (N + pad) // 32
    s = (q @ k.transpose(-1, -2)) * torch.tensor(SC32, dtype=torch.float32)
    s[..., N:] = -INF
    vt = list(range(nkt))
    if defect == "swap_tiles" and nkt >= 2:          # the V tiles of the first pair change places, the K tiles do not
        vt[0], vt[1] = 1, 0
    m = torch.full(s.shape[:-1] + (1,), -INF)
    l, o = torch.zeros_like(m), torch.zeros(q.shape)
    for t in range(nkt):
        st = s[..., 32 * t:32 * t + 32]
        mn = torch.maximum(m, st.amax(-1, keepdim=True))
        alpha = torch.exp2(m - mn)
        if defect == "no_rescale" and t > 0:
            alpha = torch.ones_like(alpha)
        p = torch.exp2(st - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + _rn_bf16(p) @ v[..., 32 * vt[t]:32 * vt[t] + 32, :]
        m = mn
    return unheads((o / l).to(torch.bfloat16)), (m + torch.log2(l)).squeeze(-1)


def restate_bwd(ops, out, lse, defect=None):
    """the gradient with the kernels' rounding points: P = exp2(s sc - lse) and dP in fp32, delta from the bf16 `out`, dS and P rounded
    to bf16 as operands of the three products, one bf16 rounding of dq, dk, dv.  -> dqkv (B, N, 3 I) bf16, delta (B, H, N) fp32"""
    H = ops.H
    q, k, v = split(ops.qkv.float(), H)
    do, o = heads(ops.dout.float(), H), heads(out.float(), H)
    s = q @ k.transpose(-1, -2)
    P = torch.exp2(s * torch.tensor(SC32, dtype=torch.float32) - lse[..., None])
    if defect == "bwd_drop_last":
        P[..., -1] = 0.0
    dP = do @ v.transpose(-1, -2)
    delta = (do * o).sum(-1, keepdim=True)
    dS = P * (dP if defect == "no_delta" else dP - delta) * 0.125
    dSb, Pb = _rn_bf16(dS), _rn_bf16(P)
    dq, dk, dv = dSb @ k, dSb.transpose(-1, -2) @ q, Pb.transpose(-1, -2) @ do
    if defect == "no_scale_dk":
        dk = dk * 8.0
    return join(dq, dk, dv).to(torch.bfloat16), delta.squeeze(-1)


@functools.lru_cache(maxsize=16)
def backward_inputs(p):
    """the `out` (bf16) and `lse` (fp32) a backward case is given: the restated forward's, so that a backward case does not depend on a
    forward kernel"""
    assert p.op == "bwd"
    return restate_fwd(operands(p))


# name -> (op, classes it must be caught on, smallest N, needs, how it is stated)
#   * pad_key: a zero-score key weighs e^-max: below 2^-24 of the row in moving-max and nothing at all in select / tie
#   * p_trunc: p = 1 exactly in select / tie (nothing to truncate); elsewhere truncation errs at most twice what rounding does, element by
#     element, which MARGIN = 2 admits by construction: near-tie is the class built to catch it
#   * out_trunc: the same factor two: caught bit for bit by tie (and only there: select's values are representable)
#   * no_rescale: the maximum of near-tie, and of tie below 66 tokens, is in the first tile for every row; swap_tiles: by select, which is
#     what it is for (the bounds need not see it, and tie's pairs j, j + N/2 can sit symmetrically in the swapped tiles)
#   * drop_last: tie's odd last key is the unpaired one, which no row selects
#   * no_scale_dk: dk is exactly zero in select
ALL = FWD_CLASSES
Defect = namedtuple("Defect", "name op classes min_n online")
DEFECTS = (
    Defect("drop_last", "fwd", ALL, 2, False),
    Defect("pad_key", "fwd", ("gauss", "flat", "offset-v", "near-tie"), 1, False),
    Defect("no_log2e", "fwd", ALL, 1, False),
    Defect("p_trunc", "fwd", ("near-tie",), 2, False),
    Defect("out_trunc", "fwd", ("tie",), 2, False),
    Defect("no_rescale", "fwd", ("gauss", "moving-max", "flat", "offset-v", "select"), 33, True),
    Defect("swap_tiles", "fwd", ("select",), 33, True),
    Defect("head_v", "fwd", ALL, 1, False),
    Defect("frame_k", "fwd", ("gauss", "moving-max", "flat", "offset-v", "select", "tie"), 1, False),      # near-tie: every frame has the same K
    Defect("stale_k", "fwd", ("gauss", "moving-max", "flat", "offset-v", "select", "tie"), 1, False),
    Defect("lse_nat", "fwd", ALL, 1, False),
    Defect("lse_nomax", "fwd", ALL, 1, False),
    Defect("no_delta", "bwd", BWD_CLASSES, 1, False),
    Defect("no_scale_dk", "bwd", tuple(c for c in BWD_CLASSES if c != "select"), 2, False),
    Defect("bwd_drop_last", "bwd", BWD_CLASSES, 2, False),
)


def defect_applies(d, p):
    if d.op != p.op or p.cls not in d.classes or p.N < d.min_n:
        return False
    if d.name == "pad_key":
        return p.N % 32 != 0
    if d.name in ("drop_last", "bwd_drop_last") and p.cls == "tie":
        return p.N % 2 == 0
    return True


# ------------------------------------------------------------------------------------------------ the rule
def ulp_bf16(x):
    _, e = torch.frexp(x.double().abs())
    return torch.where(x == 0, torch.zeros((), dtype=torch.float64, device=x.device), torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 1 - 7))


def ulp_f32(x):
    _, e = torch.frexp(x.double().abs())
    return torch.where(x == 0, torch.zeros((), dtype=torch.float64, device=x.device), torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 1 - 23))


def floor_of(name, ref, mass32):
    return LSE_FLOOR_ULPS * ulp_f32(ref) if name == "lse" else ulp_bf16(ref) + mass32


def distance(got, ref, mass):
    """largest |got - ref| / mass; a NaN or an error at an element of mass 0 is infinite"""
    err = (got.double().to(ref.device) - ref).abs()
    d = torch.where(mass > 0, err / mass.clamp_min(1e-300), torch.where(err == 0, 0.0, INF))
    d = torch.where(torch.isnan(d), torch.full_like(d, INF), d)
    return float(d.max()) if d.numel() else 0.0


def tightness(name, got, ref, mass, mass32, Y):
    """largest |got - ref| / max(MARGIN Y mass, FLOOR): the element passes the rule at <= 1"""
    err = (got.double().to(ref.device) - ref).abs()
    bound = torch.maximum(MARGIN * Y * mass, floor_of(name, ref, mass32))
    t = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, INF))
    t = torch.where(torch.isnan(t), torch.full_like(t, INF), t)
    return float(t.max()) if t.numel() else 0.0


def split_dqkv(dqkv, H):
    I = H * DH
    return {"dq": dqkv[..., :I], "dk": dqkv[..., I:2 * I], "dv": dqkv[..., 2 * I:]}


def rows(x, name, nq):
    """the rows < nq of an output (out: (B, N, I); lse: (B, H, N))"""
    return x[..., :nq] if name == "lse" else x[:, :nq]


@functools.lru_cache(maxsize=8)
def cpu_reference(p):
    return reference(operands(p))


def yardsticks(p, ref=None, nq=None):
    """Y per output of the problem, from the CPU restatement alone"""
    ops = operands(p)
    ref = cpu_reference(p) if ref is None else ref
    nq = p.N if nq is None else nq
    if p.op == "fwd":
        got = dict(zip(FWD_OUTPUTS, restate_fwd(ops)))
    else:
        got = split_dqkv(restate_bwd(ops, *backward_inputs(p))[0], p.H)
    return {k: distance(rows(g, k, nq), rows(ref[k][0].cpu(), k, nq), rows(ref[k][1].cpu(), k, nq)) for k, g in got.items()}


def judge(p, got, ref=None, Y=None, nq=None):
    """{output: (tightness, distance, Y)} of the kernel's (or a defect's) outputs `got` against the rule; passes when every tightness <= 1"""
    ref = cpu_reference(p) if ref is None else ref
    Y = yardsticks(p, ref, nq) if Y is None else Y
    nq = p.N if nq is None else nq
    res = {}
    for k, g in got.items():
        r, m, m32 = (rows(t, k, nq) for t in ref[k])
        res[k] = (tightness(k, rows(g, k, nq), r, m, m32, Y[k]), distance(rows(g, k, nq), r, m), Y[k])
    return res


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


def exact_violations(p, got, nq=None):
    """the bit-exact promises of select / tie that `got` breaks (names of outputs); dq and dk are compared as numbers (0 == -0)"""
    if p.cls not in EXACT_CLASSES:
        return []
    nq = p.N if nq is None else nq
    bad = []
    for k, e in select_expect(operands(p), p).items():
        if k not in got:
            continue
        g, e = rows(got[k].detach().cpu(), k, nq), rows(e, k, nq)
        ok = bool((g.float() == 0).all()) if k in ("dq", "dk") else same_bits(g.to(e.dtype), e)
        if not ok:
            bad.append(k)
    return bad


def rows_kept(after, before, nq, name):
    """nq < N: rows >= nq of out / lse hold the bits they held before the call"""
    a, b = (after[..., nq:], before[..., nq:]) if name == "lse" else (after[:, nq:], before[:, nq:])
    return same_bits(a, b)


def clear_caches():
    for f in (operands, backward_inputs, cpu_reference):
        f.cache_clear()
