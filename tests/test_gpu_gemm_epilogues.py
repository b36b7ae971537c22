"""GPU: every (layout, epilogue) pair of dgvit_gemm on every dispatch path of csrc/gemm.hip, against an fp64 reference.

The case table, operands, reference, bound and the restated dispatch predicates live in tests/gemm_epilogue_cases.py and are checked
on the CPU by tests/test_gemm_epilogue_matrix_host.py.  Here each case is one dgvit_gemm call through ctypes with every leading
dimension explicit:
  * inputs with a padded stride carry NaN in the padding (a read past the logical width poisons the row);
  * C and C2 are windows inside canary buffers whose logical elements are NaN before the call: every one of them must be written, and the
    columns between N and the leading dimension, the rows past M and the guard zones must keep the canary;
  * |got - ref| <= tol(K) * max(1, |f|) element-wise, tol(K) = 1e-4 * max(1, sqrt(K / 256)) (the bound test_gemm_epilogues already asserts,
    grown like the project's sqrt(K) accumulation bounds), f the multiplier of epilogues 2 and 7.  No relative term.

Worst error / bound per class, kernels on an MI355X at 6ee6c33 (this file is unchanged since 58772b7): product library 0.0458 (vec),
0.0465 (pad), 0.0513 (elem), 0.0357 (scalar), 0.0152 (tiny), 0.0311 (split), 0.0340 (split-wide), 0.0489 (TN); the sweep over the eight
tiles 0.0458 (vec), 0.0456 (split).  For comparison, from tests/test_gemm_epilogue_matrix_host.py at 58772b7: a plain fp32 CPU
evaluation of the same cases reaches 0.043 (vec), 0.047 (pad), 0.061 (elem), 0.036 (scalar), 0.013 (tiny), 0.042 (split), 0.091
(split-wide) and 0.075 (TN) of the bound.
"""
import functools

import pytest
import torch

import gemm_epilogue_cases as G
from helpers import knobs

pytestmark = pytest.mark.gpu

CANARY = 555.0
GUARD = 2048          # floats on each side of an output window (a multiple of 4: the window stays 16-byte aligned)
SPARE_ROWS = 2        # canary rows past M inside the window
LAYOUT_NAME = ("NT", "NN", "TN")


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


def _padded(x, ld):
    """(R, W) logical matrix -> device buffer of R rows ``ld`` floats apart, NaN between W and ld."""
    buf = torch.full((x.shape[0], ld), float("nan"))
    buf[:, :x.shape[1]] = x
    return buf.cuda()


@functools.lru_cache(maxsize=None)
def _device_inputs(c):
    ops = G.operands(c)
    d = {"A": _padded(ops["A"], c.lda), "B": _padded(ops["B"], c.ldb)}
    if "bias" in ops:
        d["bias"] = ops["bias"].cuda()
    if "res" in ops:
        d["res"] = _padded(ops["res"], c.ldr)
    if "aux" in ops:
        d["aux"] = _padded(ops["aux"], c.ldaux)
    for t in d.values():
        assert t.data_ptr() % 16 == 0
    return d


class _Window:
    """An (M, N) output with leading dimension ld inside a canary buffer; the logical elements start as NaN."""

    def __init__(self, M, N, ld):
        self.M, self.N, self.ld = M, N, ld
        self.buf = torch.full((GUARD + (M + SPARE_ROWS) * ld + GUARD,), CANARY, device="cuda")
        self.win = self.buf[GUARD:GUARD + (M + SPARE_ROWS) * ld].view(M + SPARE_ROWS, ld)
        self.win[:M, :N] = float("nan")
        assert self.win.data_ptr() % 16 == 0

    def ptr(self):
        return self.win.data_ptr()

    def logical(self):
        return self.win[:self.M, :self.N].cpu()

    def assert_untouched_outside(self, what):
        rest = self.buf.clone()
        rest[GUARD:GUARD + (self.M + SPARE_ROWS) * self.ld].view(self.M + SPARE_ROWS, self.ld)[:self.M, :self.N] = CANARY
        assert bool((rest == CANARY).all()), f"{what}: wrote outside the logical window (padding columns, rows past M or the guard zones)"

    def assert_untouched(self, what):
        assert bool(torch.isnan(self.win[:self.M, :self.N]).all()), f"{what}: a refused call wrote into C"
        self.assert_untouched_outside(what)


def _call(lib, c, d, C, C2, scratch, epi=None, bias="case", aux="case", c2="case", ldc=None):
    """dgvit_gemm with the case's arguments; the keyword overrides are for the refusal test."""
    p = lambda t: None if t is None else t.data_ptr()
    bias_t = d.get("bias") if bias == "case" else bias
    aux_t = d.get("aux") if aux == "case" else aux
    c2_w = C2 if c2 == "case" else c2
    return lib.dgvit_gemm(c.layout, c.epi if epi is None else epi, p(d["A"]), c.lda, p(d["B"]), c.ldb, C.ptr(), c.ldc if ldc is None else ldc,
                          c.M, c.N, c.K, p(bias_t), p(d.get("res")), c.ldr if "res" in d else 0, None if c2_w is None else c2_w.ptr(),
                          c.ldc2 if c2_w is not None else 0, p(aux_t), c.ldaux if aux_t is not None else 0,
                          p(scratch), 0 if scratch is None else scratch.numel(), torch.cuda.current_stream().cuda_stream)


def _scratch(lib, c, floats=None):
    """NaN-filled scratch of dgvit_gemm_scratch_floats (or ``floats``); dgvit_gemm clears the arrival counters itself."""
    n = int(lib.dgvit_gemm_scratch_floats(c.layout, c.M, c.N, c.K)) if floats is None else floats
    return torch.full((max(n, 4),), float("nan"), device="cuda")


def _run(lib, c, scratch):
    """One call: outputs as CPU tensors, after the canary checks."""
    from dgvit_amd import _lib
    d = _device_inputs(c)
    C = _Window(c.M, c.N, c.ldc)
    C2 = _Window(c.M, c.N, c.ldc2) if G.has_c2(c) else None
    _lib.check(_call(lib, c, d, C, C2, scratch), f"dgvit_gemm {c}")
    torch.cuda.synchronize()
    out = {"C": C.logical()}
    C.assert_untouched_outside(f"C of {c}")
    if C2 is not None:
        out["C2"] = C2.logical()
        C2.assert_untouched_outside(f"C2 of {c}")
    return out


def _ratio(c, got, ref=None):
    return G.worst_ratio(c, G.operands(c), got, G.reference(c) if ref is None else ref)


def _check(c, got, what):
    r = _ratio(c, got)
    assert r <= 1.0, f"{what} {c}: worst error / bound = {r:.3g} (bound {G.tol(c.K):.3g} x max(1, |factor|))"
    return r


# ------------------------------------------------------------------------------------------------ product library, automatic tile
@pytest.mark.parametrize("layout,epi", G.PAIRS)
@pytest.mark.parametrize("cls", G.CLASSES)
def test_pair_on_every_path_product_library(amd, cls, layout, epi):
    """Every case of the class for this pair on libdgvit_hip.so with the automatic tile.  The library's scratch query announces a
    split exactly when the restated dispatch predicts one; the split classes also give the same bits from a second call on the same
    scratch (the arrival counters were left at zero) and stay within the bound of the unsplit kernel (diagnostic library, gemm_split = 0)."""
    lib = amd.load_library()
    worst = 0.0
    for c in G.class_cases(cls, layout, epi):
        nsc = int(lib.dgvit_gemm_scratch_floats(c.layout, c.M, c.N, c.K))
        assert (nsc > 0) == G.takes_split(c), f"{c}: scratch query {nsc}, restated dispatch {G.path(c)}"
        assert nsc == G.scratch_floats(c.layout, c.M, c.N, c.K)
        scratch = _scratch(lib, c)
        got = _run(lib, c, scratch)
        worst = max(worst, _check(c, got, "product"))
        if cls in ("split", "split-wide"):
            assert nsc > 0, f"{c} is supposed to take the split path"
            again = _run(lib, c, scratch)
            for k in got:
                assert torch.equal(got[k], again[k]), f"{c}: {k} of a second call on the same scratch differs"
            with knobs(gemm_split=0) as dlib:
                unsplit = _run(dlib, c, _scratch(dlib, c))
            _check(c, unsplit, "unsplit (diagnostic library)")
            r = _ratio(c, got, unsplit)
            assert r <= 1.0, f"{c}: split against unsplit, worst difference / bound = {r:.3g}"
    print(f"gemm epilogue matrix: {LAYOUT_NAME[layout]} epilogue {epi} class {cls}: worst error / bound {worst:.4f}")


def test_weight_gradient_form_with_padded_operands(amd):
    """TN, A (K x M) and B (K x N) with padded strides, dense C: the float4 loader (72 x 68) and the scalar one (70 x 66)."""
    lib = amd.load_library()
    worst = 0.0
    for c in G.tn_cases():
        assert int(lib.dgvit_gemm_scratch_floats(c.layout, c.M, c.N, c.K)) > 0
        worst = max(worst, _check(c, _run(lib, c, _scratch(lib, c)), "product"))
    print(f"gemm epilogue matrix: TN epilogue 0 class TN: worst error / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------------ all eight tiles (diagnostic library)
@pytest.mark.parametrize("tile", G.TILES, ids=lambda t: "x".join(str(v) for v in t))
@pytest.mark.parametrize("cls", ["vec", "split"])
def test_every_pair_on_every_tile(amd, cls, tile):
    """dgvit_set_gemm_tile on the diagnostic library (same sources): all nine pairs on "vec" (direct-from-registers or LDS-image
    vector epilogue, whichever the tile takes) and on "split" (a tile whose plan does not split is an unsplit case here).  The scratch
    has room for the slabs of any tile's plan."""
    code = tile[0] * 1000000 + tile[1] * 1000 + tile[2]
    worst = 0.0
    with knobs(force_diag=True, gemm_tile=code) as dlib:
        for (layout, epi) in G.PAIRS:
            for c in G.class_cases(cls, layout, epi):
                got = _run(dlib, c, _scratch(dlib, c, 1 << 20))
                worst = max(worst, _check(c, got, f"tile {tile}"))
    print(f"gemm epilogue matrix: tile {tile} class {cls}: worst error / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------------ refusals
def test_illegal_calls_are_refused_and_leave_c_untouched(amd):
    """Epilogues 5 and 9 (internal forms), a two-output epilogue without C2, an aux epilogue without aux, a (layout, epilogue) pair that
    is not among the nine, TN with a bias or a padded C: DGVIT_ERR_ARG, and nothing is written."""
    lib = amd.load_library()
    nt, nn, tn = G.class_cases("vec", G.NT, 1)[0], G.class_cases("vec", G.NN, 2)[0], G.tn_cases()[0]
    # one set of operands per layout that satisfies every epilogue: bias, C2 and aux are all there unless a call leaves one out
    aux = torch.randn(nt.M, nt.N, generator=torch.Generator().manual_seed(1)).cuda()
    bias = torch.zeros(nt.N, device="cuda")

    def refused(c, what, **kw):
        d = dict(_device_inputs(c))
        d.setdefault("aux", aux)
        d.setdefault("bias", bias)
        C, C2 = _Window(c.M, c.N, c.ldc), _Window(c.M, c.N, c.ldc2)
        if c.layout == G.TN:
            d.pop("aux"), d.pop("bias")
            kw.setdefault("c2", None)
        rc = _call(lib, c, d, C, C2, _scratch(lib, c), **kw)
        torch.cuda.synchronize()
        assert rc == -1, f"{what}: returned {rc}"
        assert lib.dgvit_last_error(), what
        C.assert_untouched(what)
        C2.assert_untouched(what)

    for c in (nt, nn):
        for epi in (5, 9, -1, 10):
            refused(c, f"{LAYOUT_NAME[c.layout]} epilogue {epi}", epi=epi)
    for epi in (1, 6):
        refused(nt, f"epilogue {epi} without C2", epi=epi, c2=None)
    for epi in (2, 4, 7):
        refused(nn, f"epilogue {epi} without aux", epi=epi, aux=None)
    for epi in (2, 7, 4):
        refused(nt, f"NT with epilogue {epi}", epi=epi)
    for epi in (1, 6, 8, 3):
        refused(nn, f"NN with epilogue {epi}", epi=epi)
    refused(tn, "TN with a bias", bias=torch.zeros(tn.M, device="cuda"))
    refused(tn, "TN with epilogue 3", epi=3)
    C = _Window(tn.M, tn.N, tn.N + 4)
    rc = _call(lib, tn, _device_inputs(tn), C, None, _scratch(lib, tn), ldc=tn.N + 4)
    torch.cuda.synchronize()
    assert rc == -1 and b"ldc == N" in lib.dgvit_last_error()
    C.assert_untouched("TN with ldc != N")
