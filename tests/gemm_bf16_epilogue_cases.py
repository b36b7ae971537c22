"""The bf16 GEMM epilogue matrix: case table, operands, fp64 reference, bounds and the dispatch of csrc/gemm_bf16.hip restated.

Shared by tests/test_gemm_bf16_epilogue_matrix_host.py (CPU: the reference, the bounds and the table are checked against themselves
and the refusals against the library's host checks) and tests/test_gpu_gemm_bf16_epilogues.py (the kernels against the reference).
Nothing here touches a GPU.

dgvit_gemm_bf16 computes C = A B^T (A (M, K), B (N, K), bf16, k contiguous, fp32 accumulation) with six epilogues:
  0  C (bf16) = acc + bias                  1  C (bf16) = gelu(acc + bias)
  2  C (fp32) = acc + bias + res            3  C (bf16) = acc * gelu'(aux)
  4  C (fp32) = acc                         5  C (bf16) = gelu(acc + bias), C2 (bf16) = acc + bias
Epilogues 0, 1 and 5 run with and without a bias ("b", ""), epilogue 2 in four variants ("br", "b", "r", "").

Two operand regimes:
  * "int"   - A and B are integers in [-3, 3], bias and residual integers in [-8, 8]: every fp32 partial sum is an integer below 2^24
              (asserted on the CPU), so the result does not depend on the accumulation order or the path and the fp32 outputs (2, 4) and
              the bf16 stores (0, C2 of 5) are compared with torch.equal against the fp64 result, rounded once to bf16 where stored so.
              Sums of zero-mean small integers stay below 256, where bf16 holds every integer: rows 0 and M - 1 of A are planted with -3
              and +3 and the odd rows of B made non-negative, so that for K >= 72 these two rows of the output pass 256 and their odd
              values need the rounding.
  * "gauss" - the regime of helpers.bf16_epilogue_bound (A ~ N(0, 1), B ~ N(0, 1) / sqrt(K), bias, residual and aux ~ N(0, 1); A, B and
              aux bf16-rounded before the reference sees them), all six epilogues, under that function's bounds unchanged; epilogue 2,
              whose B is scaled here, takes its "f32" bound (the two additions of O(1) terms cost at most an fp32 ulp of a value below
              16, 1e-6, against 2e-5 sqrt(K) >= 5.6e-5).

What catches what (MUTANTS below): every wrong evaluation is rejected by every case it applies to, in both regimes - the gauss
bounds are tight enough for all of them, truncation included (a truncated bf16 store is off by up to 2^-7 |ref|, twice the bound,
and any matrix of a few hundred elements has one near enough a power of two).  What the bounds cannot see by nature is anything
below 2^-8 |ref|: a wrong last bit of the accumulator or of the rounding.  The int cases catch that, bit for bit.  The stride
mutants (c2_with_ldc, aux_with_ldc) exist only where the strides differ: the "pad" and "persistent" classes.
"""
import functools
import math
from collections import namedtuple

import torch

EPILOGUES = (0, 1, 2, 3, 4, 5)
VARIANTS = {0: ("b", ""), 1: ("b", ""), 2: ("br", "b", "r", ""), 3: ("",), 4: ("",), 5: ("b", "")}
EPI_VARIANTS = [(e, v) for e in EPILOGUES for v in VARIANTS[e]]
INT_EPILOGUES = (0, 2, 4, 5)                      # epilogue 5: its C2 only

# A path: (name, tile hint for dgvit_set_gemm_bf16_tile, dgvit_set_gemm_bf16_mfma16).  The MFMA shape matters to the ring kernel only.
Path = namedtuple("Path", "name hint m16")
PATHS = [Path("tile64", 64064, 1), Path("tile128", 128128, 1), Path("ring256x128", 256128, 1), Path("ring256x128-m32", 256128, 0),
         Path("ring256", 256256, 1), Path("ring256-m32", 256256, 0), Path("stream", 256257, 1)]
AUTO = Path("auto", 0, 1)                          # the product library's own choice
CLASSES = ("ragged", "n4", "tiny", "short-k", "long-k", "pad", "persistent")
PERSISTENT_PATHS = ("ring256x128", "ring256x128-m32", "ring256", "ring256-m32", "stream")     # the kernels that walk several tiles
KERNELS = ("tile64", "tile128", "ring256x128", "ring256x128-m32", "ring256", "ring256-m32", "stream")

# A case: one dgvit_gemm_bf16 call.  Leading dimensions are in elements and given whether or not the epilogue uses them.
Case = namedtuple("Case", "cls path regime epi variant M N K lda ldb ldc ldr ldc2 ldaux")


def has_bias(c):
    return "b" in c.variant


def has_res(c):
    return c.epi == 2 and "r" in c.variant


def has_aux(c):
    return c.epi == 3


def has_c2(c):
    return c.epi == 5


def out_f32(c):
    return c.epi in (2, 4)


def outputs(c):
    """name -> kind of helpers.bf16_epilogue_bound"""
    return {0: {"C": "bf16"}, 1: {"C": "gelu"}, 2: {"C": "f32"}, 3: {"C": "dgelu"}, 4: {"C": "f32"}, 5: {"C": "gelu", "C2": "bf16"}}[c.epi]


def exact_outputs(c):
    """The outputs an int case compares bit for bit."""
    return {0: ("C",), 2: ("C",), 4: ("C",), 5: ("C2",)}[c.epi] if c.regime == "int" else ()


def problem(c):
    """What the operands and the reference depend on: the case without its path."""
    return c._replace(path=None)


# ------------------------------------------------------------------------------------------------ csrc/gemm_bf16*.hip's dispatch, restated
def stream_supports(c):
    """gemm_bf16_stream_supports for a dgvit_gemm_bf16 call (no TN, no split-K, no row maps): no residual; epilogues 0, 1, 5 and 4;
    the bf16 outputs in 16-byte pieces (N, ldc and epilogue 5's ldc2 multiples of 8), the fp32 output of epilogue 4 at N % 4."""
    if has_res(c) or c.epi not in (0, 1, 5, 4):
        return False
    if c.epi != 4 and (c.N % 8 or c.ldc % 8 or (c.epi == 5 and c.ldc2 % 8)):
        return False
    return c.K % 8 == 0 and c.N % 4 == 0


def kernel_reached(c, path=None):
    """The kernel a case runs on under its path's hint: hint 256257 falls back to the 256 x 256 ring kernel where the stream kernel
    does not apply; the MFMA shape distinguishes ring kernels only."""
    p = c.path if path is None else path
    if p.hint == 0:
        return kernel_reached(c, Path("", auto_path(c.epi, c), p.m16))
    if p.hint == 64064:
        return "tile64"
    if p.hint == 128128:
        return "tile128"
    if p.hint == 256257 and stream_supports(c):
        return "stream"
    return ("ring256x128" if p.hint == 256128 else "ring256") + ("" if p.m16 else "-m32")


def tiles(c, t):
    return -(-c.M // t) * -(-c.N // t)


def auto_path(epi, c):
    """The `tile == 0` branch of dispatch<EPI> (no split-K, no TN through dgvit_gemm_bf16): the 256 x 256 ring kernel when its grid fills
    the chip (512 tiles), else 128 x 128 tiles, else - fewer than 128 of those - 64 x 64 tiles; the stream kernel where it applies."""
    assert epi == c.epi
    tile = 256256 if (c.M >= 256 and c.N >= 256 and tiles(c, 256) >= 512) else 128128
    if tile == 128128 and tiles(c, 128) < 128:
        tile = 64064
    if tile == 256256 and stream_supports(c):
        tile = 256257
    return tile


def ldc2_may_differ(path):
    """The per-tile kernel addresses C2 with its own stride; the ring kernel (launch<>) and the stream kernel (launch_stream) refuse
    epilogue 5 with ldc2 != ldc: both store C2 at C's tile-relative offset."""
    return path.hint in (64064, 128128)


# ------------------------------------------------------------------------------------------------ the table
_PAD = dict(dlda=8, dldb=16, dldc=16, dldr=4, dldc2=24, dldaux=8)


def _case(cls, path, regime, epi, variant, M, N, K, dlda=0, dldb=0, dldc=0, dldr=0, dldc2=0, dldaux=0):
    if not ldc2_may_differ(path):   # (automatic dispatch included: whichever kernel runs must accept the call)
        dldc2 = dldc
    return Case(cls, path, regime, epi, variant, M, N, K, K + dlda, K + dldb, N + dldc, N + dldr, N + dldc2, N + dldaux)


def regimes(epi):
    return ("int", "gauss") if epi in INT_EPILOGUES else ("gauss",)


def class_shapes(cls):
    return {"ragged": [(300, 264, 72)], "n4": [(300, 268, 72)], "tiny": [(1, 8, 8), (1, 4, 128)], "short-k": [(70, 72, 8), (70, 72, 40)],
            "long-k": [(70, 72, 520)], "pad": [(300, 264, 72)], "persistent": [(4357, 4104, 40)]}[cls]


def class_epi_variants(cls):
    return [(0, "b"), (2, "br"), (5, "b")] if cls == "persistent" else EPI_VARIANTS


def class_cases(cls, path):
    """Every case of class ``cls`` on ``path``: all epilogues, variants and regimes of the class, all its shapes."""
    if cls == "persistent" and path.name not in PERSISTENT_PATHS:
        return []
    pad = _PAD if cls in ("pad", "persistent") else {}
    return [_case(cls, path, regime, epi, v, M, N, K, **pad)
            for (epi, v) in class_epi_variants(cls) for regime in regimes(epi) for (M, N, K) in class_shapes(cls)]


def all_cases():
    return [c for cls in CLASSES for path in PATHS for c in class_cases(cls, path)]


# One shape per arm of auto_path, run on the product library: gauss operands.  The large shape is checked on helpers.sampled_rows.
AUTO_SHAPES = {"small": (300, 264, 72), "mid": (1500, 1544, 40), "large": (5900, 5640, 40)}
AUTO_EPI_VARIANTS = [(0, "b"), (1, "b"), (2, "br"), (3, ""), (4, ""), (5, "b")]
AUTO_ARMS = {"small": {64064}, "mid": {128128}, "large": {256256, 256257}}


def auto_cases(name):
    M, N, K = AUTO_SHAPES[name]
    return [_case("auto-" + name, AUTO, "gauss", epi, v, M, N, K, **_PAD) for (epi, v) in AUTO_EPI_VARIANTS]


# ------------------------------------------------------------------------------------------------ bounds
def bf16_epilogue_bound(kind, ref, K):
    """helpers.bf16_epilogue_bound, unchanged (imported late: helpers pulls in the oracle)."""
    from helpers import bf16_epilogue_bound as b
    return b(kind, ref, K)


def worst_ratio(c, got, ref):
    """max over the bounded outputs and elements of error / bound; inf where an element is NaN or was not written."""
    worst = 0.0
    if c.regime == "int":           # compared with exact_mismatches; the activation beside an exact C2 is the gauss cases' business
        return worst
    for name, kind in outputs(c).items():
        r = ref[name].double()
        ratio = (got[name].double() - r).abs() / bf16_epilogue_bound(kind, r, c.K)
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        worst = max(worst, float(ratio.max()))
    return worst


def exact_mismatches(c, got, ref):
    """Number of elements of the exact outputs that differ from the reference (NaN differs from everything)."""
    return sum(int((got[name].double() != ref[name].double()).sum()) for name in exact_outputs(c))


def rejected(c, got, ref):
    """Whether the comparison the GPU test makes fails on ``got``."""
    return exact_mismatches(c, got, ref) > 0 if c.regime == "int" else worst_ratio(c, got, ref) > 1.0


# ------------------------------------------------------------------------------------------------ reference arithmetic (any dtype)
def gelu(t):
    return t * 0.5 * (1 + torch.erf(t / math.sqrt(2)))


def gelu_grad(t):
    return 0.5 * (1 + torch.erf(t / math.sqrt(2))) + t * torch.exp(-0.5 * t * t) / math.sqrt(2 * math.pi)


def round_bf16(t):
    """One round-to-nearest-even fp32 -> bf16, returned as float64."""
    return t.float().bfloat16().double()


def truncate_bf16(t):
    """fp32 -> bf16 by dropping the low 16 bits (the wrong store), returned as float64."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).double()


# ------------------------------------------------------------------------------------------------ operands
def _seed(c):
    return (c.epi * 7 + len(c.variant)) * 1000003 + c.M * 10007 + c.N * 101 + c.K + (c.regime == "int") * 17


@functools.lru_cache(maxsize=None)
def _operands(p):
    g = torch.Generator().manual_seed(_seed(p))
    ops = {}
    if p.regime == "int":
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
        A, B = ri(-3, 3, p.M, p.K), ri(-3, 3, p.N, p.K)
        B[1::2] = B[1::2].abs()
        if p.M >= 2:
            A[0], A[p.M - 1] = -3.0, 3.0
        side = lambda *shape: ri(-8, 8, *shape)
    else:
        rb = lambda *shape: torch.randn(*shape, generator=g).bfloat16().float()
        A, B = rb(p.M, p.K), (torch.randn(p.N, p.K, generator=g) / math.sqrt(p.K)).bfloat16().float()
        side = lambda *shape: torch.randn(*shape, generator=g)
    ops["A"], ops["B"] = A, B
    if has_bias(p):
        ops["bias"] = side(p.N)
    if has_res(p):
        ops["res"] = side(p.M, p.N)
    if has_aux(p):
        ops["aux"] = side(p.M, p.N).bfloat16().float()
    return ops


def operands(c):
    """CPU operands of a case as float32 tensors, logical shapes (no padding); A, B and aux hold bf16-representable values.  Cases
    that differ in path only share them.  Treat the tensors as read-only."""
    return _operands(problem(c))


def partial_sum_limit(c, ops):
    """An upper bound on |any partial sum| of the int regime, in any order: sum_k |a| |b| + |bias| + |res|."""
    s = float((ops["A"].abs().double() @ ops["B"].abs().double().T).max())
    return s + (float(ops["bias"].abs().max()) if "bias" in ops else 0.0) + (float(ops["res"].abs().max()) if "res" in ops else 0.0)


# ------------------------------------------------------------------------------------------------ evaluation
def evaluate(c, ops, mode="ref", mutant=None, rows=None):
    """The case's outputs {"C": ..., "C2": ...} as float64 tensors.
      mode "ref":  fp64 throughout; in the int regime a bf16 output is the exact result rounded once (torch's fp32 -> bf16 cast), in
                   the gauss regime it is left unrounded (the bound carries the rounding);
      mode "emul": the plain emulation the bounds must admit - bf16 operands, fp32 accumulation, the epilogue in fp32, one bf16 rounding.
    ``mutant`` names a deliberately wrong evaluation (MUTANTS) the comparison must reject; ``rows`` restricts the result to those rows."""
    dt = torch.float64 if mode == "ref" else torch.float32
    A, B = ops["A"].to(dt), ops["B"].to(dt)
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    if mutant == "k_chunk_dropped":
        A, B = A[:, :c.K - 8], B[:, :c.K - 8]
    acc = sel(A) @ B.T
    zero = torch.zeros((), dtype=dt)
    bias = ops["bias"].to(dt) if "bias" in ops else zero
    if mutant == "bias_shifted_4":
        bias = torch.roll(bias, 4)
    store = truncate_bf16 if mutant == "bf16_store_truncates" else round_bf16
    if mode == "ref" and c.regime == "gauss" and mutant != "bf16_store_truncates":
        store = lambda t: t.double()
    out = {}
    if c.epi == 0:
        out["C"] = store(acc + bias)
    elif c.epi == 1:
        out["C"] = store(gelu(acc + bias))
    elif c.epi == 2:
        res = zero
        if "res" in ops:
            res = sel(torch.roll(ops["res"], -1, 0) if mutant == "res_next_row" else ops["res"]).to(dt)
        out["C"] = (acc + bias + res).double()
    elif c.epi == 3:
        aux = ops["aux"]
        if mutant == "aux_with_ldc":
            aux = _restride(aux, c.N, pitch_write=c.ldaux, pitch_read=c.ldc)
        out["C"] = store(acc * gelu_grad(acc if mutant == "dgelu_at_acc" else sel(aux).to(dt)))
    elif c.epi == 4:
        out["C"] = acc.double()
    elif c.epi == 5:
        out["C"] = store(gelu(acc + bias))
        out["C2"] = store(gelu(acc + bias) if mutant == "c2_activation" else acc + bias)
        if mutant == "c2_with_ldc":
            out["C2"] = _restride(out["C2"], c.N, pitch_write=c.ldc, pitch_read=c.ldc2)
    else:
        raise ValueError(c.epi)
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
def _reference(p):
    return evaluate(p, _operands(p))


def reference(c):
    """The reference of a case: computed once per problem, shared by the paths; read-only."""
    return _reference(problem(c))


def clear_caches():
    _operands.cache_clear()
    _reference.cache_clear()


# The wrong evaluations the comparison must reject, with the cases each applies to.  A rule depends on the case's description only,
# never on values.  Where a mutant changes nothing by construction it does not apply:
#  * k_chunk_dropped: the last 8 of K; a problem of a handful of elements (tiny) can lose an all-zero chunk in the int regime;
#  * bias_shifted_4 needs more than one 4-column group; res_next_row a second row;
#  * c2_with_ldc / aux_with_ldc need a stride that differs from ldc (pad: per-tile paths for C2, every path for aux);
#  * c2_activation and bf16_store_truncates in the int regime need values that the wrong form changes: gelu(n) rounds to n for n >= 3, and
#    every integer below 256 is a bf16 value - the planted rows pass 256 from K = 72 (see the module docstring), tiny problems have none.
# The persistent class repeats the pad class's strides at 18 M elements and is left out to keep the CPU test quick.
_BF16_OUT = lambda c: not out_f32(c)
MUTANTS = {
    "k_chunk_dropped": lambda c: c.M * c.N >= 64,
    "bias_shifted_4": lambda c: has_bias(c) and c.N > 4,
    "res_next_row": lambda c: has_res(c) and c.M > 1,
    "dgelu_at_acc": lambda c: c.epi == 3,
    "c2_activation": lambda c: c.epi == 5 and c.M * c.N >= 64,
    "c2_with_ldc": lambda c: c.epi == 5 and c.ldc2 != c.ldc,
    "aux_with_ldc": lambda c: c.epi == 3 and c.ldaux != c.ldc,
    "bf16_store_truncates": lambda c: _BF16_OUT(c) and c.M * c.N >= 64 and (c.regime == "gauss" or c.K >= 72),
}


def mutant_applies(mutant, c):
    return c.cls != "persistent" and MUTANTS[mutant](c)


# ------------------------------------------------------------------------------------------------ refusals
# Calls that gemm_bf16 / launch<> / launch_stream must refuse with DGVIT_ERR_ARG before anything touches the device.  The base call is a
# legal 16 x 16 x 16 problem with every stride 16 and every optional operand present; each entry overrides some arguments.  ``hint`` is
# the tile hint the call needs (0: any library), ``msg`` a fragment of the message.
Refusal = namedtuple("Refusal", "what epi over drop misalign hint msg")


def refusals():
    r = []
    add = lambda what, epi, msg, over=None, drop=(), misalign=None, hint=0: r.append(Refusal(what, epi, over or {}, drop, misalign, hint, msg))
    add("epilogue 3 without aux", 3, "epilogue 3 needs aux", drop=("aux",))
    add("epilogue 5 without C2", 5, "epilogue 5 needs C2", drop=("C2",))
    add("epilogue -1", -1, "unknown epilogue")
    add("epilogue 6", 6, "unknown epilogue")
    add("K % 8", 0, "multiples of 8", over=dict(K=12))
    add("lda % 8", 0, "multiples of 8", over=dict(lda=20))
    add("ldb % 8", 0, "multiples of 8", over=dict(ldb=20))
    add("N % 4", 0, "N and ldc must be multiples of 4", over=dict(N=14))
    add("ldc % 4", 0, "N and ldc must be multiples of 4", over=dict(ldc=18))
    add("ldr % 4", 2, "bad residual / aux", over=dict(ldr=18))
    add("ldaux % 4", 3, "bad residual / aux", over=dict(ldaux=18))
    add("ldc2 % 4", 5, "epilogue 5 needs C2", over=dict(ldc2=18))
    for name in ("A", "B", "C", "bias", "res", "C2", "aux"):
        add(f"{name} misaligned", 2 if name == "res" else 5, "16-byte aligned", misalign=name)
    for hint in (256256, 256128, 256257):
        add(f"hint {hint}: epilogue 5 with ldc2 != ldc", 5, "needs ldc2 == ldc", over=dict(ldc2=24), drop=("res",), hint=hint)
    return r


def refusal_arguments(r, ptr, stream=None):
    """The argument list of dgvit_gemm_bf16 for refusal ``r``; ``ptr(name)`` gives the address of an operand."""
    a = dict(M=16, N=16, K=16, lda=16, ldb=16, ldc=16, ldr=16, ldc2=16, ldaux=16)
    a.update(r.over)
    p = lambda name: None if name in r.drop else ptr(name) + (2 if r.misalign == name else 0)
    return (r.epi, p("A"), a["lda"], p("B"), a["ldb"], p("C"), a["ldc"], a["M"], a["N"], a["K"], p("bias"), p("res"), a["ldr"], p("C2"),
            a["ldc2"], p("aux"), a["ldaux"], stream)
