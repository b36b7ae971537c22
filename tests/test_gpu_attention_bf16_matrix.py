"""GPU: the bf16 attention kernels of csrc/attention_bf16.hip and csrc/attention_bf16_long.hip on every dispatch path, against fp64.

The case table, the dispatch restated, the data classes, the fp64 reference, the masses, the CPU yardstick, the rule and its floor live in
tests/attention_bf16_cases.py and are checked on the CPU by tests/test_attention_bf16_matrix_host.py.  Here every case runs through the C
ABI (dgvit_attention_forward_bf16 / _backward_bf16, the _tiled and _tiled_drop entry points; with a knob set or nq < N on the fused
kernels through the diagnostic library and its dgvit_attention_forward_bf16_queries) with
  * qkv, dout and the backward's out / lse inside larger allocations whose every other element is NaN;
  * out, lse, dqkv and delta poisoned with NaN inside canary-filled allocations: afterwards every element that must be written is finite,
    the canaries are intact, and with nq < N the rows >= nq still hold their poison, bit for bit;
  * the rule: |got - fp64| <= max(2 Y mass, floor) for every element, Y the yardstick of the CPU restatement for the same operands;
  * the exact classes: select (out == V[pi], lse == fp32(2^14 sc), dv == dout[pi^-1] bit for bit, dq == dk == 0) and tie
    (out == RN_bf16((V_a + V_b) / 2) bit for bit);
  * nq < N: rows < nq equal the nq = N run bit for bit; lse NULL: out equals the lse run bit for bit; keep = 1 _drop entries equal the
    plain tiled ones; token0: dq rows >= 1 are 0; N = 1: dq and dk are 0 up to the fp32 part of the mass and exactly 0 in select
    (dP and delta are two fp32 sums of the same 64 products in two orders: exact zeros are unprovable elsewhere);
  * a NaN frame or a NaN head beside clean items changes no bit of them; a frame alone equals the frame in its batch; the persistent
    kernels equal the per-item ones, eight waves equal nine, a launch equals the next;
  * refusals return DGVIT_ERR_ARG and leave the outputs' canaries.
The many-item problems (>= 511 items) take their fp64 reference and masses from torch on the device; test_device_reference_is_the_cpu_one
compares one of them with the CPU result.

Measured on an MI355X (the lines test_zz_report prints): per class and output the narrowest pass, as the largest |got - fp64| /
max(2 Y mass, floor) over the class's cases (<= 1 passes), with the kernel's largest distance and the case's Y in units of the mass.
  class       out                   lse                   dq                    dk                    dv
  gauss       0.76 (0.383 / 0.250)  0.54 (0.585 / 0.484)  0.50 (0.130 / 0.130)  0.50 (0.073 / 0.073)  0.50 (0.426 / 0.426)
  moving-max  0.52 (0.739 / 0.711)  0.57 (0.567 / 0.441)  0.50 (0.269 / 0.269)  0.50 (0.373 / 0.373)  0.50 (0.895 / 0.895)
  flat        0.53 (0.191 / 0.179)  0.51 (0.453 / 0.233)  0.50 (0.033 / 0.033)  0.50 (0.035 / 0.035)  0.50 (0.153 / 0.153)
  tie         0.48 (0.483 / 0.483)  0.04 (0.056 / 0.056)  0.00 (0.000 / 0.000)  0.42 (0.125 / 0.125)  0.00 (0.000 / 0.000)
  near-tie    0.50 (0.038 / 0.038)  0.37 (0.932 / 0.372)  0.50 (0.134 / 0.134)  0.50 (0.006 / 0.006)  0.50 (0.290 / 0.290)
  offset-v    0.60 (0.483 / 0.402)  0.55 (0.611 / 0.451)  0.50 (0.040 / 0.040)  0.50 (0.032 / 0.032)  0.50 (0.275 / 0.275)
  select      0.00 (0.000 / 0.000)  0.04 (0.056 / 0.056)  0.00 (0.000 / 0.000)  0.00 (0.000 / 0.000)  0.00 (0.000 / 0.000)
  token0                                                  0.50 (0.032 / 0.032)  0.50 (0.366 / 0.366)  0.50 (0.927 / 0.927)
The narrowest pass is the forward out of gauss at 513 tokens on the tiled kernels (0.764 of the bound).  A backward cell of 0.50 with
distance = Y: kernel and restatement have the same worst element with the same error.  N = 1: |dq|, |dk| up to 9.9e-7 (moving-max), at
most 0.063 of the fp32 part of the mass (flat).  The fused and the tiled kernels agree bit for bit, forward and backward, at 33, 128,
129, 256, 257 and 288 tokens.
"""
import contextlib
import ctypes
import functools

import pytest
import torch

import attention_bf16_cases as A
from test_attention_bf16_matrix_host import call_refused, refusals

pytestmark = pytest.mark.gpu

DH = A.DH
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
CASES = A.all_cases(CUS)
FWD = [c for c in CASES if c.op == "fwd"]
BWD = [c for c in CASES if c.op == "bwd"]
GUARD = 4096           # elements on each side of a buffer: payloads stay 16-byte aligned
CANARY = 555.0
NAN = float("nan")
ERR_ARG = -1
WORST = {}             # (op, cls, output) -> (tightness, distance, Y, case id)


@pytest.fixture(scope="module", autouse=True)
def _module():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    yield
    A.clear_caches()
    _device_reference.cache_clear()
    _yard.cache_clear()
    torch.cuda.empty_cache()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Buf:
    """a payload of `shape` between two guard zones.  Inputs: data in the payload, NaN in the guards (reading them poisons a result).
    Outputs: NaN in the payload (an element left unwritten shows), the canary in the guards."""

    def __init__(self, shape, dtype, data=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((2 * GUARD + n,), NAN if data is not None else CANARY, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if data is not None:
            self.t.copy_(data.to(dtype))
        else:
            self.t.fill_(NAN)
        self.before = self.buf.clone()
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def _bits(self, x):
        return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)

    def check(self, what, written=None):
        """written: boolean tensor of the payload's shape (default: everything) -- those are finite, everything else holds its bits"""
        same = self._bits(self.buf) == self._bits(self.before)
        assert bool(same[:GUARD].all()) and bool(same[-GUARD:].all()), f"{what}: wrote outside its extent"
        if written is None:
            assert bool(torch.isfinite(self.t).all()), f"{what}: an element was left unwritten, or is not finite"
        else:
            w = written.to(self.t.device).expand(self.t.shape)
            assert bool(torch.isfinite(self.t[w]).all()), f"{what}: an element that must be written is not finite"
            assert bool(same[GUARD:-GUARD].view(self.t.shape)[~w].all()), f"{what}: wrote an element it must leave alone"

    def untouched(self, what):
        assert bool((self._bits(self.buf) == self._bits(self.before)).all()), f"{what}: a refused call wrote"


def _null():
    return ctypes.c_void_p(0)


@contextlib.contextmanager
def library_for(c):
    """the product library for what it can run; the diagnostic one, with the case's knobs set and restored, for the rest"""
    import dgvit_amd
    if c.long is None and c.waves is None and not (c.op == "fwd" and c.entry == "short" and c.nq < c.N):
        yield dgvit_amd.load_library()
        return
    with dgvit_amd.diagnostic_library() as lib:
        try:
            if c.long is not None:
                lib.dgvit_set_attention_bf16_long(c.long)
            if c.waves is not None:
                lib.dgvit_set_attention_bf16_tiled_waves(c.waves)
            yield lib
        finally:
            lib.dgvit_set_attention_bf16_long(-1)
            lib.dgvit_set_attention_bf16_tiled_waves(-1)


def _ok(lib, rc, what):
    assert rc == 0, f"{what}: code {rc}: {lib.dgvit_last_error()}"


def run_fwd(c, qkv=None):
    """-> {"out": CPU bf16 (B, N, I), "lse": CPU fp32 (B, H, N) or absent} after the canary checks"""
    B, N, H, I = c.B, c.N, c.H, c.H * DH
    x = Buf((B, N, 3 * I), torch.bfloat16, data=A.operands(A.problem(c)).qkv if qkv is None else qkv)
    out = Buf((B, N, I), torch.bfloat16)
    lse = Buf((B, H, N), torch.float32) if c.lse else None
    lp = lse.ptr if lse else _null()
    with library_for(c) as lib:
        if c.entry == "short" and c.nq == N:
            rc = lib.dgvit_attention_forward_bf16(x.ptr, out.ptr, lp, B, N, H, DH, _st())
        elif c.entry == "short":
            rc = lib.dgvit_attention_forward_bf16_queries(x.ptr, out.ptr, lp, B, N, H, DH, c.nq, _st())
        elif c.entry == "tiled":
            rc = lib.dgvit_attention_forward_bf16_tiled(x.ptr, out.ptr, lp, B, N, H, DH, c.nq, _st())
        else:
            rc = lib.dgvit_attention_forward_bf16_tiled_drop(x.ptr, out.ptr, lp, B, N, H, DH, c.nq, 1.0, 1234, None, 3, _st())
        _ok(lib, rc, A.case_id(c))
        torch.cuda.synchronize()
    what = A.case_id(c)
    x.untouched(what + " qkv")
    rows = torch.arange(N) < c.nq
    out.check(what + " out", None if c.nq == N else rows[None, :, None])
    res = {"out": out.t.cpu()}
    if lse:
        lse.check(what + " lse", None if c.nq == N else rows[None, None, :])
        res["lse"] = lse.t.cpu()
    return res


def run_bwd(c, qkv=None, out=None, lse=None, dout=None):
    """-> {"dq", "dk", "dv": CPU bf16 (B, N, I), "delta": CPU fp32 (B, H, N)} after the canary checks"""
    B, N, H, I = c.B, c.N, c.H, c.H * DH
    p = A.problem(c)
    ops = A.operands(p)
    o_in, l_in = A.backward_inputs(p) if out is None else (out, lse)
    x = Buf((B, N, 3 * I), torch.bfloat16, data=ops.qkv if qkv is None else qkv)
    o = Buf((B, N, I), torch.bfloat16, data=o_in)
    d = Buf((B, N, I), torch.bfloat16, data=ops.dout if dout is None else dout)
    l = Buf((B, H, N), torch.float32, data=l_in)
    dqkv, delta = Buf((B, N, 3 * I), torch.bfloat16), Buf((B, H, N), torch.float32)
    with library_for(c) as lib:
        args = (x.ptr, o.ptr, d.ptr, l.ptr, dqkv.ptr, delta.ptr, B, N, H, DH)
        if c.entry == "short":
            rc = lib.dgvit_attention_backward_bf16(*args, _st())
        elif c.entry == "tiled":
            rc = lib.dgvit_attention_backward_bf16_tiled(*args, _st())
        else:
            rc = lib.dgvit_attention_backward_bf16_tiled_drop(*args, 1.0, 1234, None, 3, _st())
        _ok(lib, rc, A.case_id(c))
        torch.cuda.synchronize()
    what = A.case_id(c)
    for b, name in ((x, "qkv"), (o, "out"), (d, "dout"), (l, "lse")):
        b.untouched(f"{what} {name}")
    dqkv.check(what + " dqkv")
    delta.check(what + " delta")
    return {**A.split_dqkv(dqkv.t.cpu(), H), "delta": delta.t.cpu()}


# ------------------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=3)
def _device_reference(p):
    return A.reference(A.operands(p), device="cuda")


def _reference(p):
    return _device_reference(p) if p.B * p.H >= 511 else A.cpu_reference(p)


@functools.lru_cache(maxsize=64)
def _yard(p, nq):
    return A.yardsticks(p, _reference(p), nq)


def _judge(c, got, outputs):
    p = A.problem(c)
    j = A.judge(p, {k: got[k] for k in outputs if k in got}, ref=_reference(p), Y=_yard(p, c.nq), nq=c.nq)
    for k, (t, d, y) in j.items():
        key = (c.op, c.cls, k)
        if t >= WORST.get(key, (-1.0,))[0]:
            WORST[key] = (t, d, y, A.case_id(c))
    line = "; ".join(f"{k} {t:.3f} of the bound (distance {d:.3f}, Y {y:.3f})" for k, (t, d, y) in j.items())
    print(f"{A.case_id(c)} [{A.kernel_reached(c)}]: {line}")
    bad = {k: v for k, v in j.items() if v[0] > 1.0}
    assert not bad, f"{A.case_id(c)} [{A.kernel_reached(c)}] breaks the rule: " + "; ".join(
        f"{k}: {t:.3f} x the bound, distance {d:.4f} against Y {y:.4f}" for k, (t, d, y) in bad.items())
    broken = A.exact_violations(p, got, c.nq)
    assert not broken, f"{A.case_id(c)} [{A.kernel_reached(c)}]: not bit-exact in {broken}"


# ------------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize("c", FWD, ids=A.case_id)
def test_forward(c):
    got = run_fwd(c)
    _judge(c, got, A.FWD_OUTPUTS)
    if c.nq < c.N:
        dense = run_fwd(c._replace(nq=c.N))
        for k in got:
            assert A.same_bits(A.rows(got[k], k, c.nq), A.rows(dense[k], k, c.nq)), f"{k}: rows < nq differ from the nq = N run"
    if not c.lse:
        assert A.same_bits(got["out"], run_fwd(c._replace(lse=True))["out"]), "out depends on whether lse is asked for"
    if c.entry == "tiled_drop":
        plain = run_fwd(c._replace(entry="tiled"))
        assert all(A.same_bits(got[k], plain[k]) for k in got), "keep = 1 differs from the plain tiled kernel"


@pytest.mark.parametrize("c", BWD, ids=A.case_id)
def test_backward(c):
    p = A.problem(c)
    got = run_bwd(c)
    _judge(c, got, A.BWD_OUTPUTS)
    # delta = rowsum(dout o out) of the `out` it was given: a 64-term fp32 sum, within 64 * 2^-24 of the sum of absolute products
    ops, (o_in, _) = A.operands(p), A.backward_inputs(p)
    prod = A.heads(ops.dout.double(), c.H) * A.heads(o_in.double(), c.H)
    err = (got["delta"].double() - prod.sum(-1)).abs()
    assert bool((err <= 64 * A.V32 * prod.abs().sum(-1)).all()), f"delta: {float(err.max()):.3e}"
    if c.N == 1:
        # dq = dk = 0 in exact arithmetic.  dP and delta are two fp32 sums of the same 64 products in two orders, so the kernels leave
        # fp32 noise (a few 1e-7, printed below) unless the sums are exact, as in select, which exact_violations holds to 0 above.
        # Nothing of bf16 size may appear: the fp32 part of the mass, 1e-4 of the mass, bounds every element.
        ref = _reference(p)
        for k in ("dq", "dk"):
            g = got[k].double().abs()
            print(f"N = 1 {A.case_id(c)} {k}: max |{k}| {float(g.max()):.2e}, {float((g / ref[k][2].clamp_min(1e-300)).max()):.3f} of the fp32 part of the mass")
            assert bool((ref[k][0] == 0).all()) and bool((g <= ref[k][2]).all()), f"N = 1: {k} is not zero up to fp32 rounding"
    if c.cls == "token0":
        assert bool((got["dq"][:, 1:].float() == 0).all()), "token0: dq rows >= 1 are exactly zero"
    if c.entry == "tiled_drop":
        plain = run_bwd(c._replace(entry="tiled"))
        assert all(A.same_bits(got[k], plain[k]) for k in got), "keep = 1 differs from the plain tiled kernels"


def test_device_reference_is_the_cpu_one():
    """the many-item references come from torch fp64 on the device: for the 512-item problem at 129 tokens they are the CPU's to 1e-12 of
    the mass-free scale, and the masses to 1e-9"""
    p = A.Problem("fwd", "gauss", 128, 129, 4)
    dev, cpu = A.reference(A.operands(p), device="cuda"), A.reference(A.operands(p))
    for k in cpu:
        torch.testing.assert_close(dev[k][0].cpu(), cpu[k][0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(dev[k][1].cpu(), cpu[k][1], rtol=1e-9, atol=0)
        torch.testing.assert_close(dev[k][2].cpu(), cpu[k][2], rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------ neighbours cannot leak
def _case(op, entry, N, B, H, long=None, waves=None):
    return A.Case(op, entry, "gauss", B, N, H, N, True, long, waves)


LEAK = [_case("fwd", "short", 33, 3, 3), _case("fwd", "short", 197, 3, 3), _case("fwd", "short", 288, 3, 3), _case("fwd", "short", 288, 3, 3, long=0),
        _case("fwd", "short", 197, 171, 3), _case("fwd", "short", 257, 171, 3), _case("fwd", "tiled", 321, 3, 3, waves=8),
        _case("fwd", "tiled", 321, 3, 3, waves=4), _case("bwd", "short", 197, 3, 3), _case("bwd", "short", 288, 3, 3),
        _case("bwd", "short", 288, 3, 3, long=0), _case("bwd", "tiled", 321, 3, 3, waves=8), _case("bwd", "tiled", 321, 3, 3, waves=4)]


@pytest.mark.parametrize("what", ["frame", "head"])
@pytest.mark.parametrize("c", LEAK, ids=lambda c: f"{A.case_id(c)}-{A.kernel_reached(c)}")
def test_a_poisoned_neighbour_changes_no_bit(c, what):
    """the middle frame (of three, or of 171) or the middle head all NaN in every input: the other items equal the clean run bit for bit"""
    p = A.problem(c)
    ops = A.operands(p)
    B, H, I = c.B, c.H, c.H * DH
    mid = B // 2

    def poison(t, thirds):
        t = t.clone()
        if what == "frame":
            t[mid] = NAN
        else:
            for j in range(thirds):
                t[..., j * I + DH:j * I + 2 * DH] = NAN
        return t

    def clean(t, lse=False):
        if what == "frame":
            return torch.cat([t[:mid], t[mid + 1:]])
        return torch.cat([t[:, :1], t[:, 2:]], 1) if lse else torch.cat([t[..., :DH], t[..., 2 * DH:]], -1)

    if c.op == "fwd":
        a, b = run_fwd(c), _run_poisoned_fwd(c, poison(ops.qkv, 3))
        assert A.same_bits(clean(a["out"]), clean(b["out"])) and A.same_bits(clean(a["lse"], True), clean(b["lse"], True))
        return
    o_in, l_in = A.backward_inputs(p)
    l_p = l_in.clone()
    if what == "frame":
        l_p[mid] = NAN
    else:
        l_p[:, 1] = NAN
    a = run_bwd(c)
    b = _run_poisoned_bwd(c, poison(ops.qkv, 3), poison(o_in, 1), l_p, poison(ops.dout, 1))
    for k in A.BWD_OUTPUTS:
        assert A.same_bits(clean(a[k]), clean(b[k])), k
    assert A.same_bits(clean(a["delta"], True), clean(b["delta"], True))


def _run_poisoned_fwd(c, qkv):
    """run_fwd without the finiteness check of the poisoned item's outputs"""
    B, N, H, I = c.B, c.N, c.H, c.H * DH
    x, out, lse = Buf((B, N, 3 * I), torch.bfloat16, data=qkv), Buf((B, N, I), torch.bfloat16), Buf((B, H, N), torch.float32)
    with library_for(c) as lib:
        f = lib.dgvit_attention_forward_bf16_tiled if c.entry == "tiled" else None
        rc = f(x.ptr, out.ptr, lse.ptr, B, N, H, DH, N, _st()) if f else lib.dgvit_attention_forward_bf16(x.ptr, out.ptr, lse.ptr, B, N, H, DH, _st())
        _ok(lib, rc, A.case_id(c))
        torch.cuda.synchronize()
    for b in (out, lse):
        same = b._bits(b.buf) == b._bits(b.before)
        assert bool(same[:GUARD].all()) and bool(same[-GUARD:].all()), "wrote outside its extent"
    return {"out": out.t.cpu(), "lse": lse.t.cpu()}


def _run_poisoned_bwd(c, qkv, o_in, l_in, dout):
    B, N, H, I = c.B, c.N, c.H, c.H * DH
    x, o, d, l = (Buf((B, N, 3 * I), torch.bfloat16, data=qkv), Buf((B, N, I), torch.bfloat16, data=o_in), Buf((B, N, I), torch.bfloat16, data=dout),
                  Buf((B, H, N), torch.float32, data=l_in))
    dqkv, delta = Buf((B, N, 3 * I), torch.bfloat16), Buf((B, H, N), torch.float32)
    with library_for(c) as lib:
        f = lib.dgvit_attention_backward_bf16_tiled if c.entry == "tiled" else lib.dgvit_attention_backward_bf16
        _ok(lib, f(x.ptr, o.ptr, d.ptr, l.ptr, dqkv.ptr, delta.ptr, B, N, H, DH, _st()), A.case_id(c))
        torch.cuda.synchronize()
    for b in (dqkv, delta):
        same = b._bits(b.buf) == b._bits(b.before)
        assert bool(same[:GUARD].all()) and bool(same[-GUARD:].all()), "wrote outside its extent"
    return {**A.split_dqkv(dqkv.t.cpu(), H), "delta": delta.t.cpu()}


# ------------------------------------------------------------------------------------------------ the same bits on every path
@pytest.mark.parametrize("N", A.STREAM_N + A.STREAM288_N)
def test_persistent_equals_per_item_and_itself(N):
    """512 items on the persistent kernel, launch to launch; frame 77 alone (4 items: a per-item kernel) and, from 225 tokens, the whole
    batch on the per-item kernels (knob bit 0 off)"""
    c = _case("fwd", "short", N, 128, 4)
    assert A.kernel_reached(c) in ("stream", "stream288")
    qkv = A.operands(A.problem(c)).qkv
    a, b = run_fwd(c), run_fwd(c)
    assert A.same_bits(a["out"], b["out"]) and A.same_bits(a["lse"], b["lse"]), "not reproducible from launch to launch"
    one = c._replace(B=1)
    assert A.kernel_reached(one) in ("item8", "item9")
    f = run_fwd(one, qkv=qkv[77:78])
    assert A.same_bits(f["out"], a["out"][77:78]) and A.same_bits(f["lse"], a["lse"][77:78]), "per-item and persistent kernels differ"
    if N > 224:
        for bits in (2, 0):
            v = c._replace(long=bits)
            assert A.kernel_reached(v) in ("item8", "item9")
            g = run_fwd(v)
            assert A.same_bits(g["out"], a["out"]) and A.same_bits(g["lse"], a["lse"]), f"knob {bits} differs from the persistent kernel"


@pytest.mark.parametrize("N", A.ITEM9_N)
def test_eight_waves_equal_nine(N):
    f8, f9 = _case("fwd", "short", N, 2, 3, long=0), _case("fwd", "short", N, 2, 3, long=2)
    assert (A.kernel_reached(f8), A.kernel_reached(f9)) == ("item8", "item9")
    a, b = run_fwd(f8), run_fwd(f9)
    assert A.same_bits(a["out"], b["out"]) and A.same_bits(a["lse"], b["lse"])
    b8, b9 = f8._replace(op="bwd"), f9._replace(op="bwd")
    assert (A.kernel_reached(b8), A.kernel_reached(b9)) == ("dq8+dkv", "dq9+dkv")
    a, b = run_bwd(b8), run_bwd(b9)
    assert all(A.same_bits(a[k], b[k]) for k in a)


ALONE = [_case("fwd", "short", N, 2, 3) for N in A.ITEM4_N + A.ITEM8_N + A.ITEM9_N] + \
        [_case("bwd", "short", N, 2, 3) for N in A.BWD_SHORT_N + A.ITEM9_N] + \
        [_case(op, "tiled", N, 2, 2, waves=w) for op in ("fwd", "bwd") for w in (8, 4) for N in A.TILED_N]


@pytest.mark.parametrize("c", ALONE, ids=A.case_id)
def test_a_frame_alone_equals_the_frame_in_its_batch_and_a_launch_the_next(c):
    p = A.problem(c)
    ops = A.operands(p)
    one = c._replace(B=1)
    if c.op == "fwd":
        a, b, f = run_fwd(c), run_fwd(c), run_fwd(one, qkv=ops.qkv[1:2])
    else:
        o, l = A.backward_inputs(p)
        a, b, f = run_bwd(c), run_bwd(c), run_bwd(one, qkv=ops.qkv[1:2], out=o[1:2], lse=l[1:2], dout=ops.dout[1:2])
    for k in a:
        assert A.same_bits(a[k], b[k]), f"{k}: not reproducible from launch to launch"
        assert A.same_bits(f[k], a[k][1:2]), f"{k}: depends on the batch"


@pytest.mark.parametrize("N", [33, 128, 129, 256, 257, 288])
def test_tiled_and_fused_kernels_meet_the_same_rule(N):
    """the relation of test_tiled_kernels_agree_with_the_fused_ones, at the boundaries: both within the rule of the same reference (each
    asserted); whether they are bitwise equal is reported"""
    fused, tiled = _case("fwd", "short", N, 2, 3), _case("fwd", "tiled", N, 2, 3, waves=8)
    a, b = run_fwd(fused), run_fwd(tiled)
    _judge(fused, a, A.FWD_OUTPUTS)
    _judge(tiled, b, A.FWD_OUTPUTS)
    ga, gb = run_bwd(fused._replace(op="bwd")), run_bwd(tiled._replace(op="bwd"))
    _judge(fused._replace(op="bwd"), ga, A.BWD_OUTPUTS)
    _judge(tiled._replace(op="bwd"), gb, A.BWD_OUTPUTS)
    print(f"N={N}: forward bitwise equal {all(A.same_bits(a[k], b[k]) for k in a)}, backward bitwise equal {all(A.same_bits(ga[k], gb[k]) for k in ga)}")


# ------------------------------------------------------------------------------------------------ refusals, the wrapper
def test_refused_calls_leave_the_canaries():
    import dgvit_amd
    B, N, H = 2, 289, 3            # buffers that cover the largest refused problem
    I = H * DH
    bufs = {"qkv": Buf((B, N, 3 * I), torch.bfloat16, data=torch.zeros(B, N, 3 * I)), "dout": Buf((B, N, I), torch.bfloat16, data=torch.zeros(B, N, I)),
            "out": Buf((B, N, I), torch.bfloat16), "lse": Buf((B, H, N), torch.float32), "dqkv": Buf((B, N, 3 * I), torch.bfloat16),
            "delta": Buf((B, H, N), torch.float32)}
    with dgvit_amd.diagnostic_library() as lib:
        for r in refusals():
            rc = call_refused(lib, r, lambda n: bufs[n].t.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == ERR_ARG, f"{r[0]} {r[1]}: returned {rc}"
        torch.cuda.synchronize()
    for k in ("out", "lse", "dqkv", "delta"):
        bufs[k].untouched(k)


def test_queries_wrapper_uses_the_buffers_it_is_given():
    import dgvit_amd
    F = dgvit_amd.functional
    c = A.Case("fwd", "short", "gauss", 2, 197, 3, 33, True, None, None)
    qkv = A.operands(A.problem(c)).qkv.cuda()
    out, lse = Buf((2, 197, 192), torch.bfloat16), Buf((2, 3, 197), torch.float32)
    with pytest.raises(dgvit_amd.DgvitError):
        F.op_attention_bf16_queries(qkv, 3, 33, out=out.t, lse=lse.t)            # the product library has no such entry point
    with dgvit_amd.diagnostic_library():
        o, l = F.op_attention_bf16_queries(qkv, 3, 33, out=out.t, lse=lse.t)
        assert o.data_ptr() == out.t.data_ptr() and l.data_ptr() == lse.t.data_ptr()
        with pytest.raises(dgvit_amd.DgvitError):
            F.op_attention_bf16_queries(qkv, 3, 33, out=out.t[:, :, :64], lse=None)
        with pytest.raises(dgvit_amd.DgvitError):
            F.op_attention_bf16_queries(qkv, 3, 0, out=out.t, lse=None)
    torch.cuda.synchronize()
    rows = torch.arange(197) < 33
    out.check("out", rows[None, :, None])
    lse.check("lse", rows[None, None, :])
    ref = run_fwd(c)
    assert A.same_bits(out.t.cpu(), ref["out"]) and A.same_bits(lse.t.cpu(), ref["lse"])


def test_zz_report():
    """the table of the docstring: per class and output the narrowest pass over the cases run in this session"""
    print()
    for op, classes, outs in (("fwd", A.FWD_CLASSES, A.FWD_OUTPUTS), ("bwd", A.BWD_CLASSES, A.BWD_OUTPUTS)):
        for cls in classes:
            cells = [f"{k} {WORST[(op, cls, k)][0]:.2f} ({WORST[(op, cls, k)][1]:.3f} / {WORST[(op, cls, k)][2]:.3f})" for k in outs if (op, cls, k) in WORST]
            print(f"attention bf16: {op} {cls:10s} " + "; ".join(cells))
    if WORST:
        k = max(WORST, key=lambda k: WORST[k][0])
        print(f"attention bf16: narrowest pass {k}: {WORST[k][0]:.3f} of the bound in {WORST[k][3]}")
