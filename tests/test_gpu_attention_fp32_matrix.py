"""GPU: the fp32 attention kernels of csrc/attention.hip and csrc/attention_long.hip on every dispatch path, against fp64.

The case table, the dispatch restated, the data classes, the fp64 reference, the masses, the CPU yardstick, the rule and its floor live in
tests/attention_fp32_cases.py and are checked on the CPU by tests/test_attention_fp32_matrix_host.py.  Here every case runs through the C
ABI (dgvit_attention_forward / _backward, the _tiled entry points; with a knob set, nq < N on the fused kernels or keep < 1 through the
diagnostic library: dgvit_attention_forward_queries / _backward_queries and the four _drop entry points) with
  * qkv, dout and the backward's out / lse inside larger allocations whose every other element is NaN; with nq < N the rows >= nq of the
    backward's out, dout and lse are NaN too (the comment of attention_bwd promises they are not read);
  * out, lse, dqkv and the tiled backward's scratch poisoned with NaN inside canary-filled allocations: afterwards every element that must
    be written is finite, the canaries are intact, the inputs hold their bits, and with nq < N the rows >= nq of out, lse and dq still hold
    their poison, bit for bit, while dk and dv are written in every row;
  * the rule: |got - fp64| <= max(2 Y mass, floor) for every element, Y the yardstick of the CPU restatement for the same operands;
  * the exact classes: select (out == V[pi], lse == fp32(32768 qscale) bit for bit, dv == dout[pi^-1], dq == dk == 0) and tie
    (out == RN_fp32(V_a + V_b) / 2 bit for bit);
  * the kernel the restated dispatch names is the one that ran, as far as the ABI shows it: test_zz_report asserts that every kernel name
    was reached at every listed token count for both head sizes;
  * nq < N: rows < nq equal the nq = N run bit for bit on the tile and tiled kernels; the one-query kernels meet the rule of the tile
    kernels (their bitwise relation is reported); lse NULL: out equals the lse run bit for bit; dropout: lse equals the undropped run's,
    keep = 1 through the _drop entries equals the plain kernels, a second seed gives another out, seed_dev overrides seed;
  * a NaN frame or a NaN head beside clean items changes no bit of them; a frame alone equals the frame in its batch; the pipelined kernel
    equals tile2 bit for bit; a launch equals the next; bwd64 and the two-phase kernel both meet the rule (bitwise relation reported);
  * refusals return DGVIT_ERR_ARG (short scratch: DGVIT_ERR_WORKSPACE) and leave the outputs' canaries.
The many-item problems (>= 2047 items) take their fp64 reference and masses from torch on the device; test_device_reference_is_the_cpu_one
compares one of them with the CPU result.

Measured on an MI355X (the lines test_zz_report prints; 1889 tests, 1576 table cases, 95 s): per class and output the narrowest
pass, as the largest |got - fp64| / max(2 Y mass, floor) over the class's cases (<= 1 passes), with the kernel's largest distance and the
case's Y in units of the mass.
  class                 out                   lse                   dq                    dk                    dv
  gauss                 0.56 (0.853 / 0.758)  0.50 (0.519 / 0.519)  0.17 (0.174 / 0.174)  0.40 (0.413 / 0.413)  0.53 (0.591 / 0.557)
  moving-max            0.50 (2.114 / 2.105)  0.50 (1.564 / 1.564)  0.40 (0.430 / 0.543)  0.99 (0.988 / 0.450)  0.58 (1.132 / 0.980)
  flat                  0.50 (1.172 / 1.172)  0.50 (1.246 / 1.246)  0.22 (0.227 / 0.192)  0.41 (0.431 / 0.446)  0.50 (0.599 / 0.599)
  tie                   0.00                  0.06 (0.110 / 0.110)  0.00                  0.00                  0.00
  offset-v              0.52 (0.932 / 0.894)  0.50 (0.614 / 0.614)  0.10 (0.099 / 0.099)  0.20 (0.196 / 0.202)  0.50 (0.787 / 0.787)
  select                0.00                  0.06 (0.110 / 0.110)  0.00                  0.00                  0.00
  token0                                                            0.12 (0.121 / 0.138)  0.33 (0.336 / 0.304)  0.56 (0.602 / 0.524)
  gauss (dropped)       0.54 (0.865 / 0.801)  0.50 (0.395 / 0.395)  0.25 (0.251 / 0.238)  0.26 (0.269 / 0.269)  0.47 (0.495 / 0.521)
  moving-max (dropped)  0.50 (2.564 / 2.561)  0.50 (1.475 / 1.475)  0.50 (0.515 / 0.515)  0.51 (0.811 / 0.796)  0.51 (0.889 / 0.869)
  flat (dropped)        0.50 (0.903 / 0.903)  0.40 (0.831 / 0.707)  0.19 (0.191 / 0.191)  0.20 (0.206 / 0.206)  0.22 (0.224 / 0.224)
  offset-v (dropped)    0.50 (0.916 / 0.916)  0.50 (0.395 / 0.395)  0.09 (0.096 / 0.096)  0.14 (0.140 / 0.132)  0.39 (0.400 / 0.302)
The narrowest pass is dk of moving-max in bwd-fused-moving-max-B10H13N50d64-nq1-q1.0 (0.988 of the bound, through the floor).  A forward cell of
0.50 with distance = Y: the kernel and the chained-fma step order of the restatement have the same worst element with the same error (a
32x32x2 matrix-core step is fma(a1, b1, fma(a0, b0, c)): DESIGN 3.44).  With Y from the whole-row and the online forms alone, five of the
1576 table cases missed the rule (lse at N = 1 at 1.81 and 1.25 times the bound, out of offset-v at 288 and flat at 321 tokens at 1.10, of
dropped moving-max at 33 tokens at 1.15): none by a defect, all by the order of the matrix cores' steps, which the restatement now has.
Teeth: a build with the fused dropped forward's mask row stride N / 4 and the tiled forward's `key < N` guard removed fails 148 tests here
(test_forward, test_tiled_and_fused_kernels_meet_the_same_rule).
"""
import contextlib
import ctypes
import functools

import pytest
import torch

import attention_fp32_cases as A
from test_attention_fp32_matrix_host import ERR_ARG, call_refused, refusals

pytestmark = pytest.mark.gpu

CASES = A.all_cases()
FWD = [c for c in CASES if c.op == "fwd"]
BWD = [c for c in CASES if c.op == "bwd"]
GUARD = 4096           # elements on each side of a buffer: payloads stay 16-byte aligned
CANARY = 555.0
NAN = float("nan")
ERR_HIP = -2
MANY = 2000            # items from which the reference is computed on the device
WORST = {}             # (op, cls, output, dropped) -> (tightness, distance, Y, case id)
REACHED = set()        # (op, kernel, N, dh) of the table's cases that were judged
JUDGED = set()


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
    """a payload of `shape` fp32 between two guard zones.  Inputs: data in the payload, NaN in the guards (reading them poisons a result).
    Outputs: NaN in the payload (an element left unwritten shows), the canary in the guards."""

    def __init__(self, shape, data=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((2 * GUARD + n,), NAN if data is not None else CANARY, dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if data is not None:
            self.t.copy_(data)
        else:
            self.t.fill_(NAN)
        self.before = self.buf.clone()
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def _same(self):
        return self.buf.view(torch.int32) == self.before.view(torch.int32)

    def guards(self, what):
        same = self._same()
        assert bool(same[:GUARD].all()) and bool(same[-GUARD:].all()), f"{what}: wrote outside its extent"

    def check(self, what, written=None, finite=True):
        """written: boolean tensor broadcastable to the payload (default: everything) -- those are finite, everything else holds its bits"""
        self.guards(what)
        if written is None:
            assert not finite or bool(torch.isfinite(self.t).all()), f"{what}: an element was left unwritten, or is not finite"
            return
        w = written.to(self.t.device).expand(self.t.shape)
        assert not finite or bool(torch.isfinite(self.t[w]).all()), f"{what}: an element that must be written is not finite"
        assert bool(self._same()[GUARD:-GUARD].view(self.t.shape)[~w].all()), f"{what}: wrote an element it must leave alone"

    def untouched(self, what):
        assert bool(self._same().all()), f"{what}: an input changed, or a refused call wrote"


def _null():
    return ctypes.c_void_p(0)


def needs_diag(c):
    return c.q1 is not None or c.bwd64 is not None or c.keep < 1 or (c.entry == "fused" and c.nq < c.N)


@contextlib.contextmanager
def library_for(c, diag=False):
    """the product library for what it can run; the diagnostic one, with the case's knobs set and restored, for the rest"""
    import dgvit_amd
    if not (diag or needs_diag(c)):
        yield dgvit_amd.load_library()
        return
    with dgvit_amd.diagnostic_library() as lib:
        try:
            if c.q1 is not None:
                lib.dgvit_set_attention_single_query(c.q1)
            if c.bwd64 is not None:
                lib.dgvit_set_attention_bwd_single_pass(c.bwd64)
            yield lib
        finally:
            lib.dgvit_set_attention_single_query(1)
            lib.dgvit_set_attention_bwd_single_pass(1)


def _ok(lib, rc, what):
    """the call succeeded and its kernels ran to their end; a device error ends the session (nothing more is started on a faulted GPU)"""
    if rc == ERR_HIP:
        pytest.exit(f"{what}: device error: {lib.dgvit_last_error()}", returncode=3)
    assert rc == 0, f"{what}: code {rc}: {lib.dgvit_last_error()}"
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: device error: {e}", returncode=3)


def _drop_args(c, seed, seed_dev, drop_entry):
    """None: the plain entry; else (keep, seed, seed_dev pointer, layer) of the _drop entry"""
    if c.keep >= 1 and not drop_entry:
        return None
    return (c.keep, A.DROP_SEED if seed is None else seed, ctypes.c_void_p(seed_dev.data_ptr()) if seed_dev is not None else None, A.DROP_LAYER)


def run_fwd(c, qkv=None, finite=True, seed=None, seed_dev=None, drop_entry=False):
    """-> {"out": CPU (B, N, I), "lse": CPU (B, H, N) or absent} after the canary checks"""
    B, N, H, dh, I = c.B, c.N, c.H, c.dh, c.H * c.dh
    x = Buf((B, N, 3 * I), data=A.operands(A.problem(c)).qkv if qkv is None else qkv)
    out = Buf((B, N, I))
    lse = Buf((B, H, N)) if c.lse else None
    lp = lse.ptr if lse else _null()
    drop = _drop_args(c, seed, seed_dev, drop_entry)
    what = A.case_id(c)
    with library_for(c, diag=drop is not None) as lib:
        if drop is not None:
            f = lib.dgvit_attention_forward_drop if c.entry == "fused" else lib.dgvit_attention_forward_tiled_drop
            rc = f(x.ptr, out.ptr, lp, B, N, H, dh, c.nq, *drop, _st())
        elif c.entry == "tiled":
            rc = lib.dgvit_attention_forward_tiled(x.ptr, out.ptr, lp, B, N, H, dh, c.nq, _st())
        elif needs_diag(c):
            rc = lib.dgvit_attention_forward_queries(x.ptr, out.ptr, lp, B, N, H, dh, c.nq, _st())
        else:
            rc = lib.dgvit_attention_forward(x.ptr, out.ptr, lp, B, N, H, dh, _st())
        _ok(lib, rc, what)
    x.untouched(what + " qkv")
    rows = torch.arange(N) < c.nq
    out.check(what + " out", None if c.nq == N else rows[None, :, None], finite)
    res = {"out": out.t.cpu()}
    if lse:
        lse.check(what + " lse", None if c.nq == N else rows[None, None, :], finite)
        res["lse"] = lse.t.cpu()
    return res


def run_bwd(c, qkv=None, out=None, lse=None, dout=None, finite=True, poison_rows=True, seed=None, drop_entry=False):
    """-> {"dq", "dk", "dv": CPU (B, N, I)} after the canary checks.  With nq < N the rows >= nq of out, dout and lse are NaN
    (poison_rows), and dq keeps its poison there."""
    B, N, H, dh, I, nq = c.B, c.N, c.H, c.dh, c.H * c.dh, c.nq
    p = A.problem(c)
    ops = A.operands(p)
    o_in, l_in = A.backward_inputs(p) if out is None else (out, lse)
    d_in = ops.dout if dout is None else dout
    if nq < N and poison_rows:
        o_in, l_in, d_in = o_in.clone(), l_in.clone(), d_in.clone()
        o_in[:, nq:], d_in[:, nq:], l_in[..., nq:] = NAN, NAN, NAN
    x, o, d, l = Buf((B, N, 3 * I), data=ops.qkv if qkv is None else qkv), Buf((B, N, I), data=o_in), Buf((B, N, I), data=d_in), Buf((B, H, N), data=l_in)
    dqkv = Buf((B, N, 3 * I))
    scratch = Buf((B * H * N,)) if c.entry == "tiled" else None
    drop = _drop_args(c, seed, None, drop_entry)
    what = A.case_id(c)
    with library_for(c, diag=drop is not None) as lib:
        args = (x.ptr, o.ptr, d.ptr, l.ptr, dqkv.ptr)
        if c.entry == "tiled":
            args += (scratch.ptr, B * H * N)
        if drop is not None:
            f = lib.dgvit_attention_backward_drop if c.entry == "fused" else lib.dgvit_attention_backward_tiled_drop
            rc = f(*args, B, N, H, dh, nq, *drop, _st())
        elif c.entry == "tiled":
            rc = lib.dgvit_attention_backward_tiled(*args, B, N, H, dh, nq, _st())
        elif needs_diag(c):
            rc = lib.dgvit_attention_backward_queries(*args, B, N, H, dh, nq, _st())
        else:
            rc = lib.dgvit_attention_backward(*args, B, N, H, dh, _st())
        _ok(lib, rc, what)
    for b, name in ((x, "qkv"), (o, "out"), (d, "dout"), (l, "lse")):
        b.untouched(f"{what} {name}")
    written = torch.ones(N, 3 * I, dtype=torch.bool)
    written[nq:, :I] = False                       # dq rows >= nq are left alone; dk and dv are written in every row
    dqkv.check(what + " dqkv", None if nq == N else written[None], finite)
    if scratch:
        scratch.guards(what + " scratch")
    return A.split_dqkv(dqkv.t.cpu(), H)


# ------------------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=2)
def _device_reference(p):
    return A.reference(A.operands(p), device="cuda")


def _reference(p):
    return _device_reference(p) if p.B * p.H >= MANY else A.cpu_reference(p)


@functools.lru_cache(maxsize=64)
def _yard(p, nq):
    return A.yardsticks(p, _reference(p), nq)


def _judge(c, got, outputs, table=False):
    p = A.problem(c)
    kern = A.kernel_reached(c)
    j = A.judge(p, {k: got[k] for k in outputs if k in got}, ref=_reference(p), Y=_yard(p, c.nq), nq=c.nq)
    for k, (t, d, y) in j.items():
        key = (c.op, c.cls, k, c.keep < 1)
        if t >= WORST.get(key, (-1.0,))[0]:
            WORST[key] = (t, d, y, A.case_id(c))
    line = "; ".join(f"{k} {t:.3f} of the bound (distance {d:.3f}, Y {y:.3f})" for k, (t, d, y) in j.items())
    print(f"{A.case_id(c)} [{kern}]: {line}")
    bad = {k: v for k, v in j.items() if v[0] > 1.0}
    assert not bad, f"{A.case_id(c)} [{kern}] breaks the rule: " + "; ".join(
        f"{k}: {t:.3f} x the bound, distance {d:.4f} against Y {y:.4f}" for k, (t, d, y) in bad.items())
    broken = A.exact_violations(p, got, c.nq)
    assert not broken, f"{A.case_id(c)} [{kern}]: not exact in {broken}"
    if table:
        JUDGED.add(c)
        if c.nq == c.N or kern == "q1":
            REACHED.add((c.op, kern, c.N, c.dh))


def _bits_equal(a, b, nq=None):
    return all(A.same_bits(a[k] if nq is None else A.rows(a[k], k, nq), b[k] if nq is None else A.rows(b[k], k, nq)) for k in a)


# ------------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize("c", FWD, ids=A.case_id)
def test_forward(c):
    got = run_fwd(c)
    _judge(c, got, A.FWD_OUTPUTS, table=True)
    kern = A.kernel_reached(c)
    if c.nq < c.N and kern != "q1":
        dense = run_fwd(c._replace(nq=c.N))
        assert A.kernel_reached(c._replace(nq=c.N)) in (kern, "pipe", "bwd64")
        assert _bits_equal(got, dense, c.nq), "rows < nq differ from the nq = N run"
    if kern == "q1":
        tile = run_fwd(c._replace(q1=0))
        _judge(c._replace(q1=0), tile, A.FWD_OUTPUTS)
        print(f"{A.case_id(c)}: one-query kernel bitwise equal to {A.kernel_reached(c._replace(q1=0))}: {_bits_equal(got, tile, 1)}")
    if not c.lse:
        assert A.same_bits(got["out"], run_fwd(c._replace(lse=True))["out"]), "out depends on whether lse is asked for"
    if c.keep < 1 and c.lse:
        plain = run_fwd(c._replace(keep=1.0, q1=0))       # the same general kernel without the mask
        assert A.same_bits(A.rows(got["lse"], "lse", c.nq), A.rows(plain["lse"], "lse", c.nq)), "lse is not the undropped softmax's"
        assert not A.same_bits(got["out"], plain["out"]), "the mask changed nothing"


@pytest.mark.parametrize("c", BWD, ids=A.case_id)
def test_backward(c):
    got = run_bwd(c)
    _judge(c, got, A.BWD_OUTPUTS, table=True)
    kern = A.kernel_reached(c)
    if c.nq < c.N:
        clean = run_bwd(c, poison_rows=False)             # rows >= nq of out / dout / lse hold numbers: nothing may change
        for k in A.BWD_OUTPUTS:
            assert A.same_bits(A.rows(got[k], k, c.nq), A.rows(clean[k], k, c.nq)), f"{k} depends on rows >= nq of out / dout / lse"
    if kern == "q1":
        tile = run_bwd(c._replace(q1=0))
        _judge(c._replace(q1=0), tile, A.BWD_OUTPUTS)
        print(f"{A.case_id(c)}: one-query kernel bitwise equal to {A.kernel_reached(c._replace(q1=0))}: {_bits_equal(got, tile, 1)}")
    if c.N == 1:
        ref = _reference(A.problem(c))
        for k in ("dq", "dk"):
            g = got[k].double().abs()
            print(f"N = 1 {A.case_id(c)} {k}: max |{k}| {float(g.max()):.2e}, {float((g / ref[k][1].clamp_min(1e-300)).max()):.3f} of the mass")
            assert bool((ref[k][0].abs() <= 1e-13).all()) and bool((g <= ref[k][1]).all()), f"N = 1: {k} is not zero up to the mass"
    if c.cls == "token0":
        assert bool((got["dq"][:, 1:c.nq] == 0).all()), "token0: dq rows >= 1 are exactly zero"


def test_device_reference_is_the_cpu_one():
    """the many-item references come from torch fp64 on the device: for a 2048-item problem at 50 tokens they are the CPU's to 1e-12
    and the masses to 1e-9"""
    p = A.Problem("fwd", "gauss", 512, 50, 4, 64, 50, 1.0)
    dev, cpu = A.reference(A.operands(p), device="cuda"), A.reference(A.operands(p))
    for k in cpu:
        torch.testing.assert_close(dev[k][0].cpu(), cpu[k][0], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(dev[k][1].cpu(), cpu[k][1], rtol=1e-9, atol=0)


# ------------------------------------------------------------------------------------------------ neighbours cannot leak
def _case(op, entry, N, B=3, H=3, dh=64, nq=None, q1=None, bwd64=None, keep=1.0, cls="gauss"):
    return A.Case(op, entry, cls, B, N, H, dh, N if nq is None else nq, True, q1, bwd64, keep)


LEAK = [_case(op, e, N, dh=dh, **kw) for dh in A.DHS for op in ("fwd", "bwd") for e, N, kw in (
    ("fused", 32, {}), ("fused", 50, {}), ("fused", 50, dict(bwd64=0)), ("fused", 197, {}), ("fused", 50, dict(nq=1)), ("tiled", 321, {}),
    ("fused", 50, dict(keep=0.5)), ("fused", 197, dict(keep=0.5)), ("tiled", 321, dict(keep=0.5))) if not (op == "fwd" and "bwd64" in kw)]
LEAK += [_case("fwd", "fused", 50, B=683, H=3, dh=dh) for dh in A.DHS]          # the pipelined walk: 2049 items


@pytest.mark.parametrize("what", ["frame", "head"])
@pytest.mark.parametrize("c", LEAK, ids=lambda c: f"{A.case_id(c)}-{A.kernel_reached(c)}")
def test_a_poisoned_neighbour_changes_no_bit(c, what):
    """the middle frame or the middle head all NaN in every input: the other items equal the clean run bit for bit"""
    p = A.problem(c)
    ops = A.operands(p)
    B, H, dh, I = c.B, c.H, c.dh, c.H * c.dh
    mid = B // 2

    def poison(t, thirds):
        t = t.clone()
        if what == "frame":
            t[mid] = NAN
        else:
            for j in range(thirds):
                t[..., j * I + dh:j * I + 2 * dh] = NAN
        return t

    def clean(t, lse=False):
        if what == "frame":
            return torch.cat([t[:mid], t[mid + 1:]])
        return torch.cat([t[:, :1], t[:, 2:]], 1) if lse else torch.cat([t[..., :dh], t[..., 2 * dh:]], -1)

    if c.op == "fwd":
        a, b = run_fwd(c), run_fwd(c, qkv=poison(ops.qkv, 3), finite=False)
        assert A.same_bits(clean(a["out"]), clean(b["out"])) and A.same_bits(clean(a["lse"], True), clean(b["lse"], True))
        assert bool(torch.isfinite(clean(b["out"])[:, :c.nq]).all())
        return
    o_in, l_in = A.backward_inputs(p)
    l_p = l_in.clone()
    if what == "frame":
        l_p[mid] = NAN
    else:
        l_p[:, 1] = NAN
    a = run_bwd(c)
    b = run_bwd(c, qkv=poison(ops.qkv, 3), out=poison(o_in, 1), lse=l_p, dout=poison(ops.dout, 1), finite=False)
    for k in A.BWD_OUTPUTS:
        assert A.same_bits(clean(A.rows(a[k], k, c.nq)), clean(A.rows(b[k], k, c.nq))), k
        assert bool(torch.isfinite(clean(A.rows(b[k], k, c.nq))).all()), k


# ------------------------------------------------------------------------------------------------ the same bits on every path
@pytest.mark.parametrize("dh", A.DHS)
@pytest.mark.parametrize("shape", A.PIPE_SHAPES, ids=lambda s: f"{s[0] * s[1]}items")
@pytest.mark.parametrize("N", [33, 41, 50, 64])
def test_pipelined_equals_tile2_and_itself(N, shape, dh):
    """2048, 2049 and 3071 items on the pipelined kernel, launch to launch; one frame alone, and the first frames that stay under 2048
    items as their own call (both reach tile2): the same bits"""
    B, H = shape
    c = _case("fwd", "fused", N, B=B, H=H, dh=dh)
    assert A.kernel_reached(c) == "pipe"
    qkv = A.operands(A.problem(c)).qkv
    a, b = run_fwd(c), run_fwd(c)
    assert _bits_equal(a, b), "not reproducible from launch to launch"
    f = B // 2 + 1
    one = c._replace(B=1)
    assert A.kernel_reached(one) == "tile2"
    g = run_fwd(one, qkv=qkv[f:f + 1])
    assert A.same_bits(g["out"], a["out"][f:f + 1]) and A.same_bits(g["lse"], a["lse"][f:f + 1]), "tile2 and the pipelined kernel differ"
    nb = 2047 // H
    first = c._replace(B=nb)
    assert A.kernel_reached(first) == "tile2" and (nb + 1) * H > 2047
    g = run_fwd(first, qkv=qkv[:nb])
    assert A.same_bits(g["out"], a["out"][:nb]) and A.same_bits(g["lse"], a["lse"][:nb]), "tile2 and the pipelined kernel differ"


@pytest.mark.parametrize("dh", A.DHS)
@pytest.mark.parametrize("N", A.TILE2_N)
def test_single_pass_and_two_phase_backward_meet_the_same_rule(N, dh):
    one, two = _case("bwd", "fused", N, B=2, dh=dh), _case("bwd", "fused", N, B=2, dh=dh, bwd64=0)
    assert (A.kernel_reached(one), A.kernel_reached(two)) == ("bwd64", "two-phase2")
    a, b = run_bwd(one), run_bwd(two)
    _judge(one, a, A.BWD_OUTPUTS)
    _judge(two, b, A.BWD_OUTPUTS)
    print(f"N={N} dh={dh}: bwd64 bitwise equal to two-phase: " + ", ".join(f"{k} {A.same_bits(a[k], b[k])}" for k in a))


ALONE = [_case(op, "fused", N, B=2, dh=64, **kw) for op in ("fwd", "bwd") for N in A.TILE1_N + A.TILE2_N + A.TILE4_N
         for kw in (({}, dict(bwd64=0)) if op == "bwd" and 32 < N <= 64 else ({},))] + \
        [_case(op, "tiled", N, B=2, H=2, dh=64) for op in ("fwd", "bwd") for N in A.TILED_N] + \
        [_case(op, e, N, B=2, dh=32) for op in ("fwd", "bwd") for e, N in (("fused", 32), ("fused", 50), ("fused", 197), ("tiled", 321))] + \
        [_case(op, e, N, B=2, dh=dh, keep=0.5) for op in ("fwd", "bwd") for dh in A.DHS for e, N in (("fused", 50), ("fused", 197), ("tiled", 321))] + \
        [_case(op, "fused", N, B=2, dh=dh, nq=1) for op in ("fwd", "bwd") for dh in A.DHS for N in (17, 50)]


@pytest.mark.parametrize("c", ALONE, ids=A.case_id)
def test_a_frame_alone_equals_the_frame_in_its_batch_and_a_launch_the_next(c):
    """(with dropout the frame alone is frame 0: the mask's counter holds the frame index)"""
    p = A.problem(c)
    ops = A.operands(p)
    f = 0 if c.keep < 1 else 1
    one = c._replace(B=1)
    if c.op == "fwd":
        a, b, g = run_fwd(c), run_fwd(c), run_fwd(one, qkv=ops.qkv[f:f + 1])
    else:
        o, l = A.backward_inputs(p)
        a, b, g = run_bwd(c), run_bwd(c), run_bwd(one, qkv=ops.qkv[f:f + 1], out=o[f:f + 1], lse=l[f:f + 1], dout=ops.dout[f:f + 1])
    for k in a:
        assert A.same_bits(a[k], b[k]), f"{k}: not reproducible from launch to launch"
        assert A.same_bits(A.rows(g[k], k, c.nq), A.rows(a[k][f:f + 1], k, c.nq)), f"{k}: depends on the batch"


@pytest.mark.parametrize("dh", A.DHS)
@pytest.mark.parametrize("N", [33, 64, 65, 128, 129, 256, 257, 288])
def test_tiled_and_fused_kernels_meet_the_same_rule(N, dh):
    """both within the rule of the same reference (each asserted); whether they are bitwise equal is reported"""
    fused, tiled = _case("fwd", "fused", N, B=2, dh=dh, bwd64=0), _case("fwd", "tiled", N, B=2, dh=dh)
    a, b = run_fwd(fused), run_fwd(tiled)
    _judge(fused, a, A.FWD_OUTPUTS)
    _judge(tiled, b, A.FWD_OUTPUTS)
    ga, gb = run_bwd(fused._replace(op="bwd")), run_bwd(tiled._replace(op="bwd"))
    _judge(fused._replace(op="bwd"), ga, A.BWD_OUTPUTS)
    _judge(tiled._replace(op="bwd"), gb, A.BWD_OUTPUTS)
    print(f"N={N} dh={dh}: forward bitwise equal {_bits_equal(a, b)}, backward (two-phase) bitwise equal {_bits_equal(ga, gb)}")


# ------------------------------------------------------------------------------------------------ dropout
DROPPED = [_case("fwd", e, N, B=2, dh=dh, keep=keep, nq=nq) for dh in A.DHS for keep in A.DROP_KEEPS
           for e, N, nq in (("fused", 7, None), ("fused", 50, None), ("fused", 197, None), ("fused", 50, 1), ("tiled", 321, None), ("tiled", 65, 33))]


@pytest.mark.parametrize("c", DROPPED, ids=A.case_id)
def test_dropout_seeds(c):
    """a second seed gives another out and the same lse; seed_dev overrides seed, in the forward and (through the gradient it gives) in
    the backward's regenerated mask"""
    a = run_fwd(c)
    other = run_fwd(c, seed=A.DROP_SEED + 1)
    assert not A.same_bits(a["out"], other["out"]) and A.same_bits(A.rows(a["lse"], "lse", c.nq), A.rows(other["lse"], "lse", c.nq))
    dev = torch.tensor([A.DROP_SEED], dtype=torch.int64, device="cuda")
    over = run_fwd(c, seed=A.DROP_SEED + 1, seed_dev=dev)
    assert _bits_equal(a, over, c.nq), "seed_dev does not override seed"
    cb = c._replace(op="bwd")
    ga, gb = run_bwd(cb), run_bwd(cb, seed=A.DROP_SEED + 1)
    assert not A.same_bits(ga["dv"], gb["dv"]), "the backward's mask does not depend on the seed"


KEEP1 = [_case(op, e, N, B=2, dh=dh, nq=nq) for op in ("fwd", "bwd") for dh in A.DHS
         for e, N, nq in (("fused", 32, None), ("fused", 50, None), ("fused", 197, None), ("fused", 197, 33), ("tiled", 321, None), ("tiled", 129, 33))]


@pytest.mark.parametrize("c", KEEP1, ids=A.case_id)
def test_keep_one_through_the_drop_entries_is_the_plain_kernel(c):
    run = run_fwd if c.op == "fwd" else run_bwd
    a, b = run(c), run(c, drop_entry=True)
    assert _bits_equal(a, b, c.nq), "keep = 1 differs from the plain kernels"


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_calls_leave_the_canaries():
    import dgvit_amd
    B, N, H = 2, 289, 3            # buffers that cover the largest refused problem
    I = H * 64
    bufs = {"qkv": Buf((B, N, 3 * I), data=torch.zeros(B, N, 3 * I)), "dout": Buf((B, N, I), data=torch.zeros(B, N, I)),
            "out": Buf((B, N, I)), "lse": Buf((B, H, N)), "dqkv": Buf((B, N, 3 * I)), "scratch": Buf((B * H * N,))}
    with dgvit_amd.diagnostic_library() as lib:
        for r in refusals():
            rc = call_refused(lib, r, lambda n: bufs[n].t.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == r.code, f"{r.entry} {r.what}: returned {rc}"
        torch.cuda.synchronize()
    assert ERR_ARG == -1
    for k in ("out", "lse", "dqkv", "scratch"):
        bufs[k].untouched(k)


def test_zz_report():
    """the table of the docstring: per class and output the narrowest pass over the cases run in this session; and, when the whole table
    ran, that every kernel name of the restated dispatch was reached at every listed token count for both head sizes"""
    print()
    for drop in (False, True):
        for op, classes, outs in (("fwd", A.FWD_CLASSES, A.FWD_OUTPUTS), ("bwd", A.BWD_CLASSES, A.BWD_OUTPUTS)):
            for cls in classes:
                cells = [f"{k} {WORST[(op, cls, k, drop)][0]:.2f} ({WORST[(op, cls, k, drop)][1]:.3f} / {WORST[(op, cls, k, drop)][2]:.3f})"
                         for k in outs if (op, cls, k, drop) in WORST]
                if cells:
                    print(f"attention fp32: {op} {'dropped ' if drop else ''}{cls:10s} " + "; ".join(cells))
    if WORST:
        k = max(WORST, key=lambda k: WORST[k][0])
        print(f"attention fp32: narrowest pass {k}: {WORST[k][0]:.3f} of the bound in {WORST[k][3]}")
    print(f"attention fp32: {len(JUDGED)} of the table's {len(CASES)} cases judged")
    if len(JUDGED) == len(CASES):
        for dh in A.DHS:
            for (op, kern), ns in A.LISTED_N.items():
                missing = [n for n in ns if (op, kern, n, dh) not in REACHED]
                assert not missing, f"{op} {kern} at dim_head {dh}: not reached at {missing}"
        print("attention fp32: every kernel reached at every listed token count, dim_head 64 and 32")
