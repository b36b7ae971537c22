"""GPU: every epilogue of dgvit_gemm_bf16 on every dispatch path of csrc/gemm_bf16.hip and csrc/gemm_bf16_stream.hip, exactly and against fp64.

The case table, operands, reference, bounds and the restated dispatch live in tests/gemm_bf16_epilogue_cases.py and are checked on the
CPU by tests/test_gemm_bf16_epilogue_matrix_host.py.  Here each case is one dgvit_gemm_bf16 call through ctypes with every leading
dimension explicit:
  * inputs with a padded stride carry NaN in the padding (a read past the logical width poisons the row);
  * C and C2 are windows inside canary buffers whose logical elements are NaN before the call: every one of them must be written, and the
    columns between N and the leading dimension, two spare rows past M and the guard zones must keep the canary (520: a bf16 value);
  * "int" cases (small-integer operands, every fp32 partial sum exact) are compared with torch.equal - epilogues 0, 2, 4 and the C2 of 5;
  * "gauss" cases are held to helpers.bf16_epilogue_bound, element-wise, all six epilogues.
The paths: the per-tile kernel at 64 x 64 and 128 x 128, the ring kernel at 256 x 128 and 256 x 256 in both MFMA shapes, the stream
kernel (hint 256257, which hands epilogues 2 and 3 and N % 8 == 4 back to the ring kernel), the product library's automatic choice,
and the TN split-K form behind dgvit_wgrad_bf16.

Worst error / bound, gauss cases (int cases are exact or fail), bf16 outputs / fp32 outputs, with this file's cases on 6ee6c33.  A
bf16 store alone reaches 2^-8 |ref| just above a power of two, so the bf16 figure sits just under 1 by nature, on the CPU and on
every path alike (the same element decides it); the fp32 figure is decided by the last fp32 addition of epilogue 2.
CPU emulation (bf16 operands, fp32 accumulation, fp32 epilogue, one bf16 rounding; it does not depend on the path), per class: ragged
0.9934 / 0.0047, n4 0.9934 / 0.0044, tiny 0.8349 / 0.0021, short-k 0.9913 / 0.0072, long-k 0.9909 / 0.0019, pad 0.9934 / 0.0047,
persistent 0.9954 / 0.0083.  Per epilogue: 0: 0.9934, 1: 0.9875, 2: 0.0072, 3: 0.9878, 4: 0.0042, 5: 0.9934.
Kernels on an MI355X, per class, the same on each of the seven forced paths (tile64, tile128, ring256x128, ring256x128-m32, ring256,
ring256-m32, stream; persistent on the last five): ragged 0.9934 / 0.0040, n4 0.9934 / 0.0038, tiny 0.8349 / 0.0021, short-k 0.9913 /
0.0072, long-k 0.9909 / 0.0029, pad 0.9934 / 0.0040, persistent 0.9954 / 0.0067.  Automatic dispatch: small 0.9921 / 0.0037, mid
0.9951 / 0.0070, large (sampled rows) 0.9954 / 0.0057.  dgvit_wgrad_bf16 and every int case: exact.
"""
import functools

import pytest
import torch

import gemm_bf16_epilogue_cases as G
from helpers import knobs, sampled_rows

pytestmark = pytest.mark.gpu

CANARY = 520.0        # exactly representable in bf16
GUARD = 2048          # elements on each side of an output window (the window stays 16-byte aligned in both element sizes)
SPARE_ROWS = 2        # canary rows past M inside the window


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_tensors():
    """The operands and references are computed once and shared by the tests of this file; nothing of them outlives it."""
    yield
    _device_inputs_of.cache_clear()
    G.clear_caches()
    torch.cuda.empty_cache()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _padded(x, ld, dtype):
    """(R, W) logical matrix -> device buffer of R rows ``ld`` elements apart, NaN between W and ld."""
    buf = torch.full((x.shape[0], ld), float("nan"), dtype=dtype)
    buf[:, :x.shape[1]] = x.to(dtype)
    return buf.cuda()


@functools.lru_cache(maxsize=None)
def _device_inputs_of(p):
    ops = G.operands(p)
    bf = torch.bfloat16
    d = {"A": _padded(ops["A"], p.lda, bf), "B": _padded(ops["B"], p.ldb, bf)}
    assert torch.equal(d["A"][:, :p.K].float().cpu(), ops["A"]) and torch.equal(d["B"][:, :p.K].float().cpu(), ops["B"])   # bf16 holds them
    if "bias" in ops:
        d["bias"] = ops["bias"].cuda()
    if "res" in ops:
        d["res"] = _padded(ops["res"], p.ldr, torch.float32)
    if "aux" in ops:
        d["aux"] = _padded(ops["aux"], p.ldaux, bf)
    for t in d.values():
        assert t.data_ptr() % 16 == 0
    return d


def _device_inputs(c):
    return _device_inputs_of(G.problem(c))


class _Window:
    """An (M, N) output with leading dimension ld inside a canary buffer; the logical elements start as NaN."""

    def __init__(self, M, N, ld, dtype):
        self.M, self.N, self.ld = M, N, ld
        self.buf = torch.full((GUARD + (M + SPARE_ROWS) * ld + GUARD,), CANARY, device="cuda", dtype=dtype)
        self.win = self.buf[GUARD:GUARD + (M + SPARE_ROWS) * ld].view(M + SPARE_ROWS, ld)
        self.win[:M, :N] = float("nan")
        assert self.win.data_ptr() % 16 == 0

    def ptr(self):
        return self.win.data_ptr()

    def logical(self):
        return self.win[:self.M, :self.N]

    def assert_written(self, what):
        assert not bool(torch.isnan(self.logical()).any()), f"{what}: logical elements were left unwritten (or are NaN)"

    def assert_untouched_outside(self, what):
        keep = self.logical().clone()
        self.win[:self.M, :self.N] = CANARY
        ok = bool((self.buf == CANARY).all())
        self.win[:self.M, :self.N] = keep
        assert ok, f"{what}: wrote outside the logical window (padding columns, rows past M or the guard zones)"

    def assert_untouched(self, what):
        assert bool(torch.isnan(self.logical()).all()), f"{what}: a refused call wrote into the window"
        self.assert_untouched_outside(what)


def _call(lib, c, d, C, C2):
    p = lambda t: None if t is None else t.data_ptr()
    return lib.dgvit_gemm_bf16(c.epi, p(d["A"]), c.lda, p(d["B"]), c.ldb, C.ptr(), c.ldc, c.M, c.N, c.K, p(d.get("bias")), p(d.get("res")),
                               c.ldr if "res" in d else 0, None if C2 is None else C2.ptr(), c.ldc2 if C2 is not None else 0, p(d.get("aux")),
                               c.ldaux if "aux" in d else 0, _stream())


def _run(lib, c):
    """One call: the outputs as device tensors (views of their windows), after the written and canary checks."""
    d = _device_inputs(c)
    C = _Window(c.M, c.N, c.ldc, torch.float32 if G.out_f32(c) else torch.bfloat16)
    C2 = _Window(c.M, c.N, c.ldc2, torch.bfloat16) if G.has_c2(c) else None
    rc = _call(lib, c, d, C, C2)
    assert rc == 0, f"dgvit_gemm_bf16 {c}: code {rc}: {lib.dgvit_last_error()}"
    torch.cuda.synchronize()
    out = {"C": C}
    if C2 is not None:
        out["C2"] = C2
    for name, w in out.items():
        w.assert_written(f"{name} of {c}")
        w.assert_untouched_outside(f"{name} of {c}")
    return {name: w.logical() for name, w in out.items()}


def _compare(c, got, rows=None):
    """Exact (int) or bounded (gauss) comparison on the device; returns worst error / bound (0 for an int case)."""
    if rows is None:
        ref = {k: v.cuda() for k, v in G.reference(c).items()}
    else:
        ref = {k: v.cuda() for k, v in G.evaluate(c, G.operands(c), rows=rows).items()}
        got = {k: v[rows.cuda()] for k, v in got.items()}
    if c.regime == "int":
        bad = G.exact_mismatches(c, got, ref)
        assert bad == 0, f"{c}: {bad} elements of {G.exact_outputs(c)} differ from the exact result"
        return 0.0
    r = G.worst_ratio(c, got, ref)
    assert r <= 1.0, f"{c}: worst error / bound = {r:.4g}"
    return r


class _Worst:
    """Worst error / bound of the gauss cases, bf16 and fp32 outputs apart: a bf16 store alone comes close to its bound, whatever the
    path, while the fp32 figure shows the accumulation."""

    def __init__(self):
        self.w = {"bf16": 0.0, "fp32": 0.0}

    def add(self, c, r):
        k = "fp32" if G.out_f32(c) else "bf16"
        self.w[k] = max(self.w[k], r)

    def __str__(self):
        return f"bf16 outputs {self.w['bf16']:.4f}, fp32 outputs {self.w['fp32']:.4f}"


# ------------------------------------------------------------------------------------------------ 1. forced paths (diagnostic library)
_FORCED = [(path, cls) for cls in G.CLASSES for path in G.PATHS if G.class_cases(cls, path)]


@pytest.mark.parametrize("path,cls", _FORCED, ids=[f"{p.name}-{cls}" for (p, cls) in _FORCED])
def test_every_epilogue_on_a_forced_path(amd, path, cls):
    """dgvit_set_gemm_bf16_tile / dgvit_set_gemm_bf16_mfma16 on the diagnostic library (same sources): every epilogue, variant and
    regime of the class.  Poison and canaries first, then torch.equal (int) or the project's bound (gauss)."""
    worst, n = _Worst(), 0
    with knobs(force_diag=True, gemm_bf16_tile=path.hint, gemm_bf16_mfma16=path.m16) as dlib:
        for c in G.class_cases(cls, path):
            worst.add(c, _compare(c, _run(dlib, c)))
            n += 1
    print(f"bf16 gemm epilogue matrix: path {path.name} class {cls}: {n} cases, worst error / bound {worst}")


# ------------------------------------------------------------------------------------------------ 2. automatic dispatch (product library)
@pytest.mark.parametrize("name", list(G.AUTO_SHAPES))
def test_automatic_dispatch_takes_the_path_meant_for_the_shape(amd, name):
    """libdgvit_hip.so with no hint: the result is within the bound of the reference and bit-identical to the same call on the
    diagnostic library with the hint the restated dispatch predicts (same sources, same kernel).  The large shape is compared on
    helpers.sampled_rows; the canaries are checked around the whole window."""
    lib = amd.load_library()
    M = G.AUTO_SHAPES[name][0]
    rows = sampled_rows(M) if name == "large" else None
    worst = _Worst()
    for c in G.auto_cases(name):
        hint = G.auto_path(c.epi, c)
        assert hint in G.AUTO_ARMS[name]
        got = _run(lib, c)
        worst.add(c, _compare(c, got, rows))
        with knobs(force_diag=True, gemm_bf16_tile=hint) as dlib:
            forced = _run(dlib, c)
        for k in got:
            assert torch.equal(got[k], forced[k]), f"{c}: {k} of the automatic dispatch differs from hint {hint}"
        del got, forced
    _device_inputs_of.cache_clear()
    torch.cuda.empty_cache()
    print(f"bf16 gemm epilogue matrix: automatic dispatch, shape {name}: worst error / bound {worst}")


# ------------------------------------------------------------------------------------------------ 3. dgvit_wgrad_bf16
WGRAD_SHAPES = [(1, 8, 8), (33, 264, 520), (4095, 8, 16), (4096, 8, 16), (16383, 8, 8), (16384, 8, 8), (1000, 256, 256)]


@functools.lru_cache(maxsize=None)
def _wgrad_operands(T, Mo, Ko):
    """Integers in [-3, 3]: |any partial sum| <= 9 T < 2^24, so dW = dY^T X and db = column sums of dY are exact in fp32 in any order."""
    assert 9 * T < 2 ** 24
    g = torch.Generator().manual_seed(T * 1009 + Mo * 31 + Ko)
    dy = torch.randint(-3, 4, (T, Mo), generator=g).float()
    x = torch.randint(-3, 4, (T, Ko), generator=g).float()
    return dy, x, (dy.double().T @ x.double()).float(), dy.double().sum(0).float()


@pytest.mark.parametrize("m16", [1, 0])
@pytest.mark.parametrize("T,Mo,Ko", WGRAD_SHAPES)
def test_wgrad_bf16_is_exact_and_stays_inside_its_outputs_and_scratch(amd, T, Mo, Ko, m16):
    """dW (Mo x Ko) = dY^T X and db = sum over tokens, on the TN split-K ring kernel and colsum_bf16: exact on integer operands; dW, db
    and a scratch of exactly dgvit_wgrad_bf16_scratch_floats floats (NaN before the call) sit in canary buffers that must survive; a
    second call on the same scratch gives the same bits; db = NULL leaves db alone; one float too little scratch is refused."""
    dy, x, dw_ref, db_ref = _wgrad_operands(T, Mo, Ko)
    dyd, xd = dy.bfloat16().cuda(), x.bfloat16().cuda()
    with knobs(gemm_bf16_mfma16=m16) as lib:
        ns = int(lib.dgvit_wgrad_bf16_scratch_floats(Mo, Ko, T))
        assert ns > 0
        scratch = _Window(1, ns, ns, torch.float32)

        def call(dW, db, floats):
            return lib.dgvit_wgrad_bf16(dyd.data_ptr(), xd.data_ptr(), dW.ptr(), None if db is None else db.ptr(), scratch.ptr(), floats, T, Mo,
                                        Ko, _stream())

        results = []
        for attempt in range(2):             # the second call finds the first one's partial sums in the scratch
            dW, db = _Window(Mo, Ko, Ko, torch.float32), _Window(1, Mo, Mo, torch.float32)
            rc = call(dW, db, ns)
            assert rc == 0, f"dgvit_wgrad_bf16: code {rc}: {lib.dgvit_last_error()}"
            torch.cuda.synchronize()
            for w, what in ((dW, "dW"), (db, "db")):
                w.assert_written(what)
                w.assert_untouched_outside(what)
            scratch.assert_untouched_outside("scratch")
            assert torch.equal(dW.logical().cpu(), dw_ref), f"dW differs in {int((dW.logical().cpu() != dw_ref).sum())} elements"
            assert torch.equal(db.logical().cpu()[0], db_ref)
            results.append((dW.logical().clone(), db.logical().clone()))
        assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
        # without a bias gradient
        dW, db = _Window(Mo, Ko, Ko, torch.float32), _Window(1, Mo, Mo, torch.float32)
        assert call(dW, None, ns) == 0
        torch.cuda.synchronize()
        dW.assert_written("dW (db = NULL)")
        dW.assert_untouched_outside("dW (db = NULL)")
        db.assert_untouched("db of a call without db")
        scratch.assert_untouched_outside("scratch (db = NULL)")
        assert torch.equal(dW.logical().cpu(), dw_ref)
        # one float too little
        scratch.win[:1, :ns] = float("nan")
        dW = _Window(Mo, Ko, Ko, torch.float32)
        rc = call(dW, db, ns - 1)
        torch.cuda.synchronize()
        assert rc == -4 and lib.dgvit_last_error(), rc            # DGVIT_ERR_WORKSPACE
        for w, what in ((dW, "dW"), (db, "db"), (scratch, "scratch")):
            w.assert_untouched(f"{what} of a call refused for its scratch")


# ------------------------------------------------------------------------------------------------ 4. refusals leave C and C2 alone
def test_refused_calls_write_nothing(amd):
    """The refusals of the CPU test (all of them precede any device call) again with real windows: DGVIT_ERR_ARG, and C and C2 keep
    their NaN and their canaries."""
    bufs = {n: torch.zeros(1 << 16, device="cuda") for n in ("A", "B", "bias", "res", "aux")}
    for r in G.refusals():
        C, C2 = _Window(16, 16, 24, torch.float32), _Window(16, 16, 24, torch.bfloat16)
        ptr = lambda n: C.ptr() if n == "C" else C2.ptr() if n == "C2" else bufs[n].data_ptr()
        with knobs(gemm_bf16_tile=r.hint) as lib:
            rc = lib.dgvit_gemm_bf16(*G.refusal_arguments(r, ptr, _stream()))
            msg = lib.dgvit_last_error()
        torch.cuda.synchronize()
        assert rc == -1 and msg and r.msg.encode() in msg, f"{r.what}: {rc} {msg}"
        C.assert_untouched(f"C of {r.what}")
        C2.assert_untouched(f"C2 of {r.what}")
