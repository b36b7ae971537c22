"""The fp32 GEMM epilogue matrix: case table, operands, fp64 reference, bound and the dispatch predicates of csrc/gemm.hip restated.

Shared by tests/test_gemm_epilogue_matrix_host.py (CPU: the reference, the bound and the table are checked against themselves and
against the library's host entry points) and tests/test_gpu_gemm_epilogues.py (the kernels against the reference).  Nothing here
touches a GPU.

dgvit_gemm has nine legal (layout, epilogue) pairs - NT x {0, 1, 6, 8, 3} and NN x {0, 2, 7, 4} - plus the TN weight-gradient form.
Epilogue 0 runs in four variants (bias and residual, bias, residual, neither), so a "pair variant" is (layout, epilogue, variant).
"""
import functools
import math
from collections import namedtuple

import torch

NT, NN, TN = 0, 1, 2
PAIRS = [(NT, 0), (NT, 1), (NT, 6), (NT, 8), (NT, 3), (NN, 0), (NN, 2), (NN, 7), (NN, 4)]
E0_VARIANTS = ("br", "b", "r", "")           # epilogue 0: which of bias / residual are given
TILES = [(128, 128, 32), (128, 128, 16), (64, 64, 32), (64, 64, 64), (128, 64, 32), (64, 128, 32), (64, 128, 16), (64, 64, 16)]   # DGVIT_TILES
CLASSES = ("vec", "pad", "elem", "scalar", "tiny", "split", "split-wide")

# A case: one dgvit_gemm call.  Leading dimensions are in floats; ldr / ldc2 / ldaux are given whether or not the epilogue uses them.
Case = namedtuple("Case", "cls layout epi variant M N K lda ldb ldc ldr ldc2 ldaux")


def has_bias(c):
    return c.layout != TN and (c.epi in (1, 6, 8, 3) or (c.epi == 0 and "b" in c.variant))


def has_res(c):
    return c.layout != TN and c.epi == 0 and "r" in c.variant


def has_aux(c):
    return c.epi in (2, 7, 4)


def has_c2(c):
    return c.epi in (1, 6)


def pair_variants(layout, epi):
    return [(layout, epi, v) for v in (E0_VARIANTS if epi == 0 else ("",))]


def _case(cls, layout, epi, variant, M, N, K, dlda=0, dldb=0, dldc=0, dldr=0, dldc2=0, dldaux=0):
    kb = K if layout == NT else N            # B's contiguous extent: k for NT, n for NN
    return Case(cls, layout, epi, variant, M, N, K, K + dlda, kb + dldb, N + dldc, N + dldr, N + dldc2, N + dldaux)


_PAD = dict(dlda=4, dldb=8, dldc=12, dldr=4, dldc2=20, dldaux=8)       # every stride distinct, all multiples of 4
_ELEM = dict(dldc=1, dldr=5, dldc2=7, dldaux=3)                        # float4 loader, element-wise epilogue
_ODD = dict(dlda=3, dldb=5, dldc=1, dldr=5, dldc2=7, dldaux=3)         # the padded-odd variant of the scalar class


def class_cases(cls, layout, epi):
    """Every case of class ``cls`` for the pair (layout, epi): all variants of epilogue 0, all shapes of the class."""
    out = []
    for (_, _, v) in pair_variants(layout, epi):
        mk = functools.partial(_case, cls, layout, epi, v)
        if cls == "vec":
            out.append(mk(130, 132, 72))
        elif cls == "pad":
            out.append(mk(130, 132, 72, **_PAD))
        elif cls == "elem":
            out.append(mk(130, 132, 72, **_ELEM))
        elif cls == "scalar":
            out += [mk(67, 70, 50), mk(67, 70, 50, **_ODD)]
        elif cls == "tiny":
            out += [mk(1, 4, 4), mk(1, 2, 128)]
        elif cls == "split":
            out += [mk(70, 68, 520), mk(70, 68, 520, **_PAD)]
        elif cls == "split-wide":
            out.append(mk(70, 516, 304) if layout == NN else mk(70, 1028, 304))
        else:
            raise ValueError(cls)
    return out


def tn_cases():
    """The weight-gradient form: A (K x M, lda = M + 4), B (K x N, ldb = N + 8), dense C.  Float4 loader, then scalar."""
    return [Case("TN", TN, 0, "", M, N, 300, M + 4, N + 8, N, N, N, N) for (M, N) in ((72, 68), (70, 66))]


def all_cases():
    return [c for (layout, epi) in PAIRS for cls in CLASSES for c in class_cases(cls, layout, epi)] + tn_cases()


# ------------------------------------------------------------------------------------------------ bound
def tol(K):
    """test_gemm_epilogues asserts 1e-4 absolute for these operands up to K = 256; the project's fp32 accumulation bounds grow
    like sqrt(K)."""
    return 1e-4 * max(1.0, math.sqrt(K / 256.0))


def bound(c, ops):
    """Element-wise bound on |got - ref| of C (and C2): tol(K) * max(1, |f|), f the multiplicative factor of epilogues 2 and 7."""
    b = torch.full((c.M, c.N), tol(c.K), dtype=torch.float64)
    if c.epi == 2:
        b = b * gelu_grad(ops["aux"].double()).abs().clamp_min(1.0)
    elif c.epi == 7:
        b = b * ops["aux"].double().abs().clamp_min(1.0)
    return b


def worst_ratio(c, ops, got, ref):
    """max over outputs and elements of error / bound; inf where an element is NaN or was not written."""
    b = bound(c, ops)
    worst = 0.0
    for k, r in ref.items():
        ratio = (got[k].double() - r).abs() / b
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        worst = max(worst, float(ratio.max()))
    return worst


# ------------------------------------------------------------------------------------------------ reference arithmetic (any dtype)
def gelu(t):
    return t * 0.5 * (1 + torch.erf(t / math.sqrt(2)))


def gelu_grad(t):
    return 0.5 * (1 + torch.erf(t / math.sqrt(2))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi)


def gelu_tanh(t):
    return 0.5 * t * (1 + torch.tanh(math.sqrt(2 / math.pi) * (t + 0.044715 * t ** 3)))


def gelu_tanh_grad(t):
    u = math.sqrt(2 / math.pi) * (t + 0.044715 * t ** 3)
    th = torch.tanh(u)
    return 0.5 * (1 + th) + 0.5 * t * (1 - th * th) * math.sqrt(2 / math.pi) * (1 + 3 * 0.044715 * t * t)


# ------------------------------------------------------------------------------------------------ operands
def _seed(c):
    return (c.layout * 7 + c.epi) * 1000003 + c.M * 10007 + c.N * 101 + c.K + CLASSES.index(c.cls) * 17 if c.cls != "TN" else c.M + c.N


@functools.lru_cache(maxsize=None)
def operands(c):
    """fp32 CPU operands of a case, logical shapes (no padding): A ~ N(0, 1), B ~ N(0, 1) * 3 / sqrt(K) (pre-activations of standard
    deviation ~3, the regime of test_gemm_epilogues), bias / res / aux ~ N(0, 1).  Planted: bias columns at +8 and -8 (the saturated
    tails of erf) and, for epilogue 4, aux entries that are exactly 0.0 and -0.0 (both mask).  No denormals.  Epilogues 0 variants
    of one shape share A and B.  Treat the tensors as read-only."""
    g = torch.Generator().manual_seed(_seed(c))
    ops = {}
    if c.layout == TN:
        ops["A"] = torch.randn(c.K, c.M, generator=g)
        ops["B"] = torch.randn(c.K, c.N, generator=g) * (3 / math.sqrt(c.K))
        return ops
    ops["A"] = torch.randn(c.M, c.K, generator=g)
    ops["B"] = (torch.randn(c.N, c.K, generator=g) if c.layout == NT else torch.randn(c.K, c.N, generator=g)) * (3 / math.sqrt(c.K))
    bias, res, aux = torch.randn(c.N, generator=g), torch.randn(c.M, c.N, generator=g), torch.randn(c.M, c.N, generator=g)
    bias[c.N - 1], bias[(c.N - 1) // 2] = 8.0, -8.0
    if has_bias(c):
        ops["bias"] = bias
    if has_res(c):
        ops["res"] = res
    if has_aux(c):
        if c.epi == 4:
            for i, (m, n) in enumerate(zero_sites(c)):
                aux[m, n] = -0.0 if i % 2 == 0 else 0.0
        ops["aux"] = aux
    return ops


def zero_sites(c):
    """Where epilogue 4's aux is exactly zero: -0.0 at the even entries of this list, +0.0 at the odd ones.  The last row and column
    (the ragged tile) are among them; at most half of a tiny problem's elements are planted."""
    sites = [(c.M - 1, c.N - 1), (0, 0), (c.M // 2, c.N // 3), (c.M // 3, c.N // 2), (c.M - 1, 0), (0, c.N - 1)]
    uniq = []
    for s in sites:
        if s not in uniq:
            uniq.append(s)
    return uniq[:max(1, min(len(uniq), c.M * c.N // 2))]


# ------------------------------------------------------------------------------------------------ evaluation
def evaluate(c, ops, dtype=torch.float64, mutant=None):
    """The case's outputs {"C": ..., "C2": ...} from ``ops``, computed in ``dtype`` on the CPU.  dtype float64 with mutant None is the
    reference; float32 is the plain fp32 evaluation the bound must admit; ``mutant`` names a deliberately wrong evaluation the bound
    must reject (see MUTANTS) - wrong arithmetic on the CPU, nothing on the GPU is involved."""
    A, B = ops["A"].to(dtype), ops["B"].to(dtype)
    if mutant == "split_drops_last_slice":
        kk = 512
        A = A[:, :kk]
        B = B[:, :kk] if c.layout == NT else B[:kk]
    if c.layout == TN:
        return {"C": A.T @ B}
    acc = A @ (B.T if c.layout == NT else B)
    bias = ops["bias"].to(dtype) if "bias" in ops else None
    if mutant == "bias_dropped":
        bias = None
    zero = torch.zeros((), dtype=dtype)
    b0 = bias if bias is not None else zero
    pre, post = (zero, b0) if mutant == "bias_after_activation" else (b0, zero)
    act, dact = (gelu_tanh, gelu_tanh_grad) if mutant == "tanh_gelu" else (gelu, gelu_grad)

    def side(name, ld):
        s = ops[name].to(dtype)
        if mutant == "side_from_next_row":
            s = torch.roll(s, -1, 0)
        if mutant == "aux_stride_n" and name == "aux":
            s = _restride(s, c.N, pitch_write=ld, pitch_read=c.N)
        return s

    out = {}
    if c.epi == 0:
        out["C"] = acc + b0 + (side("res", c.ldr) if "res" in ops else zero)
    elif c.epi == 1:
        out["C"] = acc + b0
        out["C2"] = act(acc + pre) + post
    elif c.epi == 2:
        out["C"] = acc * dact(side("aux", c.ldaux))
    elif c.epi == 3:
        out["C"] = torch.relu(acc + pre) + post
    elif c.epi == 4:
        a = side("aux", c.ldaux)
        out["C"] = torch.where((a >= 0) if mutant == "aux_ge_zero" else (a > 0), acc, torch.zeros_like(acc))
    elif c.epi == 6:
        out["C"] = dact(acc + pre) + post
        out["C2"] = act(acc + pre) + post
    elif c.epi == 7:
        out["C"] = acc * side("aux", c.ldaux)
    elif c.epi == 8:
        out["C"] = act(acc + pre) + post
    else:
        raise ValueError(c.epi)
    if mutant == "c2_with_ldc":
        out["C2"] = _restride(out["C2"], c.N, pitch_write=c.ldc, pitch_read=c.ldc2)
    return out


def _restride(x, N, pitch_write, pitch_read):
    """An (M, N) matrix laid into a NaN-filled flat buffer with row pitch ``pitch_write`` and read back with ``pitch_read``: what a
    kernel that uses the wrong leading dimension sees (reads) or leaves (writes)."""
    M = x.shape[0]
    flat = torch.full((M * max(pitch_write, pitch_read) + N,), float("nan"), dtype=x.dtype)
    idx_w = (torch.arange(M)[:, None] * pitch_write + torch.arange(N)[None, :]).reshape(-1)
    flat[idx_w] = x.reshape(-1)
    idx_r = (torch.arange(M)[:, None] * pitch_read + torch.arange(N)[None, :]).reshape(-1)
    return flat[idx_r].reshape(M, N)


@functools.lru_cache(maxsize=None)
def reference(c):
    """fp64 reference from the fp32-rounded operands.  Computed once per case and shared; read-only."""
    return evaluate(c, operands(c))


# The wrong evaluations the bound must reject, with the cases each applies to.  A rule depends on the case's description only, never on
# values.  Where a mutant changes nothing by construction it does not apply:
#  * tanh_gelu: the tanh and erf forms differ by more than tol only for about 0.5 < |t| < 3.5.  A column with the planted +-8 bias keeps t in
#    the saturated tails, so the case needs columns without a planted bias (N >= 4) - and, for epilogue 2 whose argument is aux ~ N(0, 1)
#    times acc, more than a handful of elements.
#  * side_from_next_row needs a second row; aux_stride_n and c2_with_ldc need a stride that differs from the one it is mistaken for;
#  * split_drops_last_slice: the "split" class (K = 520 = 512 + 8).
MUTANTS = {
    "tanh_gelu": lambda c: c.epi in (1, 6, 8) and c.N >= 4 or c.epi == 2 and c.M * c.N >= 64,
    "bias_dropped": has_bias,
    "bias_after_activation": lambda c: c.epi in (1, 6, 8, 3),
    "side_from_next_row": lambda c: (has_res(c) or has_aux(c)) and c.M > 1,
    "aux_stride_n": lambda c: has_aux(c) and c.ldaux != c.N,
    "c2_with_ldc": lambda c: has_c2(c) and c.ldc2 != c.ldc,
    "aux_ge_zero": lambda c: c.epi == 4,
    "split_drops_last_slice": lambda c: c.cls == "split",
}


# ------------------------------------------------------------------------------------------------ csrc/gemm.hip's dispatch, restated
# Base pointers: every operand the tests pass is 16-byte aligned (asserted where the buffers are made), so al16() is true throughout.
def vec4(c):
    """gemm_f32: the float4 loader, or the scalar 64 x 64 x 32 variant."""
    v = c.lda % 4 == 0 and c.ldb % 4 == 0
    if c.layout == NT:
        return v and c.K % 4 == 0
    if c.layout == NN:
        return v and c.K % 4 == 0 and c.N % 4 == 0
    return v and c.M % 4 == 0 and c.N % 4 == 0


def evec(c):
    """gemm_f32: the vector epilogue, or the element-wise one (which forces the 64 x 64 x 32 tile).  TN: C is the slab buffer, ldc = N."""
    return (c.N % 4 == 0 and c.ldc % 4 == 0 and (not has_res(c) or c.ldr % 4 == 0) and (not has_c2(c) or c.ldc2 % 4 == 0)
            and (not has_aux(c) or c.ldaux % 4 == 0))


def auto_tile(layout, M, N):
    if layout == TN:
        return (128, 128, 32) if (M >= 128 and N >= 128) else (64, 64, 32)
    if layout == NN and N >= 512:
        return (64, 128, 16)
    return (64, 128, 16) if N >= 1024 else (64, 64, 32)


def tile_used(c, hint=None):
    """pick_tile: ``hint`` is dgvit_set_gemm_tile's tile, None the automatic choice."""
    if not vec4(c) or not evec(c):
        return (64, 64, 32)
    return hint if hint else auto_tile(c.layout, c.M, c.N)


def wg_per_cu(layout, tile):
    BM, BN, BK = tile
    a = BM * (BK + 4) if layout != TN else BK * (BM + 4)
    b = BN * (BK + 4) if layout == NT else BK * (BN + 4)
    return min(8, (160 * 1024) // (2 * (a + b) * 4))


SplitPlan = namedtuple("SplitPlan", "tiles nsplit split_from kchunk slab_floats")


def split_plan(M, N, K, tile, occ):
    BM, BN, BK = tile
    tiles = -(-M // BM) * -(-N // BN)
    none = SplitPlan(tiles, 1, tiles, 0, 0)
    KT, cus = -(-K // BK), 256
    slots = cus * occ
    if KT < 8 or tiles <= 0:
        return none
    S, frm = 1, tiles
    if tiles * 2 <= slots:
        S, frm = min(KT // 4, slots // tiles), 0
    elif tiles > slots:
        r = tiles % cus
        if 0 < r <= cus // 2:
            S, frm = min(KT // 4, cus // r), tiles - r
    if S < 2:
        return none
    kt_per = -(-KT // S)
    S = -(-KT // kt_per)
    if S < 2:
        return none
    return SplitPlan(tiles, S, frm, kt_per * BK, (tiles - frm) * S * BM * BN)


def gemm_split_plan(layout, M, N, K):
    """The plan dgvit_gemm_scratch_floats and dgvit_gemm size their scratch with: the automatic tile, whatever the strides."""
    if layout == TN or M <= 0 or N <= 0 or K <= 0:
        return SplitPlan(0, 1, 0, 0, 0)
    t = auto_tile(layout, M, N)
    return split_plan(M, N, K, t, wg_per_cu(layout, t))


def al4(n):
    return (n + 3) & ~3


def scratch_floats(layout, M, N, K):
    """dgvit_gemm_scratch_floats for the NT / NN forms."""
    pl = gemm_split_plan(layout, M, N, K)
    return al4(pl.tiles) + al4(pl.slab_floats) if pl.nsplit > 1 else 0


def takes_split(c, hint=None, scratch=None):
    """Whether `launch` cuts this case's tiles into k-slices: the shape plans a split on the automatic tile (dgvit_gemm attaches the
    scratch only then), the float4 loader and the vector epilogue run, and the plan for the tile actually used fits ``scratch`` floats
    (None: exactly dgvit_gemm_scratch_floats)."""
    if c.layout == TN:
        return False
    need = scratch_floats(c.layout, c.M, c.N, c.K)
    if need == 0 or not vec4(c) or not evec(c):
        return False
    auto = gemm_split_plan(c.layout, c.M, c.N, c.K)
    t = tile_used(c, hint)
    pl = split_plan(c.M, c.N, c.K, t, wg_per_cu(c.layout, t))
    cap = (need if scratch is None else scratch) - al4(auto.tiles)
    return pl.nsplit > 1 and pl.slab_floats <= cap and pl.tiles <= auto.tiles


def path(c, hint=None):
    """The dispatch class a case reaches: (loader, epilogue, split, tile)."""
    t = tile_used(c, hint)
    return ("float4" if vec4(c) else "scalar", "vector" if evec(c) else "element", takes_split(c, hint), t)
