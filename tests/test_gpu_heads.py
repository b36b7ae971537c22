"""GPU: the fused SAC heads of csrc/heads.hip on every dispatch path, against fp64.

The case tables, data classes, references, masses, yardsticks and the rule live in tests/head_cases.py and are checked on the CPU by
tests/test_head_matrix_host.py.  Here every case runs through the product C ABI (dgvit_mlp_head_forward / _backward,
dgvit_tanh_gaussian_forward / _backward) with
  * NaN in everything a kernel must not read: the padding behind a row of a strided input, the floats before an unaligned base;
  * every output and the scratch inside canary guard zones: NULL slots, the third layer of a NULL dy and everything outside the logical
    extents must keep the canary;
  * the rule: distance to fp64 in units of the mass <= max(2 Y, 8 * 2^-24), Y the fp32 yardstick of the (family, output, class) from
    the CPU alone;
  * the exact conditions: the `exact` class equals fp64 bit for bit; two runs give the same bits; a twin head equals its two single
    towers (dx = dx_t0 + dx_t1 in fp32); rows of one block do not depend on the other blocks; the partial path equals the sum of the
    direct results of its blocks; strided = contiguous; a NULL slot changes no other output; tanh_mean does not depend on log_std or
    eps; eps = 0 gives action = tanh_mean; log_std beyond a clamp bound gives the bits of the bound and a dlog_std of exactly 0;
    refusals return an error and leave the canaries.

Measured on an MI355X (the lines every test prints; `kernel distance / yardstick Y` in units of 2^-24 of the mass, largest over the cases
of the class).  The bound is max(2 Y, 8): the floor everywhere but for h1, whose Y was 4.20 and 4.75 in two classes.  torch's fp32 matmul
sums in an order that depends on the CPU and its thread count, so Y moves by a few tenths between machines, which only the bounds of h1
can feel.  The narrowest pass is h1 of the `dead` class, 4.84 against 8; the saturated and deep tanh-Gaussian rows, which the earlier
test could only ask to be finite, are within 0.80.
  family class     output kernel / Y
  mlp normal      h1 4.14 / 4.20; h2 1.19 / 1.41; y 0.15 / 0.18; dw3 0.95 / 1.24; db3 1.90 / 1.90; dw2 2.82 / 3.23; db2 2.24 / 2.24; dw1 1.83 / 2.21; db1 1.11 / 1.11; dx 1.12 / 1.00
  mlp rowscale    h1 3.19 / 3.32; h2 1.27 / 1.27; y 0.16 / 0.36; dw3 0.37 / 0.38; db3 0.76 / 0.76; dw2 2.43 / 2.53; db2 1.27 / 1.51; dw1 3.78 / 3.39; db1 0.62 / 0.98; dx 1.50 / 1.62
  mlp dead        h1 4.84 / 3.49; h2 0.54 / 0.54; y 0.05 / 0.04; dw3 0.06 / 0.06; db3 0.78 / 0.86; dw2 1.70 / 1.32; db2 1.40 / 1.48; dw1 0.70 / 0.81; db1 0.34 / 0.58; dx 0.59 / 0.60
  mlp one_row     h1 4.75 / 4.75; h2 1.24 / 1.24; y 0.11 / 0.19; dw3 0.62 / 0.39; db3 0.59 / 1.24; dw2 2.86 / 2.37; db2 1.41 / 1.46; dw1 1.80 / 2.17; db1 1.04 / 1.57; dx 0.62 / 0.62
  mlp exact       h1 0.00 / 0.00; h2 0.00 / 0.00; y 0.00 / 0.00; dw3 0.00 / 0.00; db3 0.00 / 0.00; dw2 0.00 / 0.00; db2 0.00 / 0.00; dw1 0.00 / 0.00; db1 0.00 / 0.00; dx 0.00 / 0.00
  tg  normal      action 0.86 / 1.67; tanh_mean 1.08 / 1.35; log_prob 0.45 / 0.73; dmean 0.62 / 1.31; dlog_std 0.97 / 0.97
  tg  shoulder    action 0.86 / 1.79; tanh_mean 1.06 / 1.26; log_prob 0.54 / 0.77; dmean 0.61 / 1.54; dlog_std 0.99 / 1.24
  tg  saturated   action 0.79 / 1.07; tanh_mean 0.68 / 1.08; log_prob 0.34 / 0.63; dmean 0.80 / 0.66; dlog_std 0.77 / 0.66
  tg  deep        action 0.57 / 1.26; tanh_mean 0.48 / 0.48; log_prob 0.26 / 0.51; dmean 0.36 / 0.68; dlog_std 0.36 / 0.68
  tg  tiny_scale  action 0.48 / 0.48; tanh_mean 0.48 / 0.48; log_prob 1.08 / 0.70; dmean 0.91 / 1.58; dlog_std 0.98 / 1.19
  tg  clamp_edges action 0.84 / 1.27; tanh_mean 1.10 / 1.31; log_prob 0.72 / 0.76; dmean 0.62 / 1.35; dlog_std 0.93 / 0.93
  tg  zero_eps    action 0.90 / 0.99; tanh_mean 1.22 / 1.26; log_prob 0.45 / 0.53; dmean 0.64 / 0.67; dlog_std 0.00 / 0.00
  through the wrappers:
  mlp normal      h1 2.40 / 4.20; h2 0.37 / 1.41; y 0.04 / 0.18; dw3 0.08 / 1.24; db3 0.12 / 1.90; dw2 0.69 / 3.23; db2 0.72 / 2.24; dw1 1.36 / 2.21; dx 0.67 / 1.00
  tg  saturated   action 0.53 / 1.07; tanh_mean 0.52 / 1.08; log_prob 0.33 / 0.63; dmean 0.36 / 0.66; dlog_std 0.36 / 0.66
"""
import ctypes

import numpy as np
import pytest
import torch

import head_cases as H

pytestmark = pytest.mark.gpu

CANARY = 555.0
GUARD = 64            # floats on each side of a buffer (256 bytes: payloads stay 16-byte aligned)
NAN = float("nan")
ERR_ARG = -1          # DGVIT_ERR_ARG


@pytest.fixture(scope="module")
def lib():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    from dgvit_amd import _lib
    return _lib.load()


def _ok(rc, what):
    from dgvit_amd import _lib
    _lib.check(rc, what)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tab(bufs):
    return (ctypes.c_void_p * len(bufs))(*[0 if b is None else (b if isinstance(b, int) else b.ptr) for b in bufs])


def _p(b):
    return ctypes.c_void_p(0 if b is None else b.ptr)


class Buf:
    """n floats that start `off` floats behind a 16-byte boundary, inside guard zones.  Everything but the payload holds ``fill`` (NaN for
    inputs: reading it poisons the result; the canary for outputs)."""

    def __init__(self, n=None, data=None, off=0, fill=CANARY):
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
            n = data.size
        self.n, self.off, self.fill = n, off, fill
        self.buf = torch.full((GUARD + off + n + GUARD,), fill, dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD + off:GUARD + off + n]
        self.ptr = self.t.data_ptr()
        assert self.ptr % 16 == 4 * (off % 4)
        if data is not None:
            self.t.copy_(torch.from_numpy(data))

    def numpy(self, *shape):
        return self.t.cpu().numpy().reshape(*shape)

    def check(self, what, written=True):
        rest = self.buf.clone()
        if written:
            rest[GUARD + self.off:GUARD + self.off + self.n] = self.fill
        assert bool((rest == self.fill).all()), f"{what}: wrote " + ("outside its extent" if written else "into a slot it must leave alone")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_same(a, b, what, keys=None):
    for k in (keys if keys is not None else a):
        assert same_bits(a[k], b[k]), f"{what}: {k} differs, max |diff| {float(np.abs(a[k].astype(np.float64) - b[k]).max()):.3e}"


class Worst:
    """largest kernel distance per output over the cases of a (family, class), beside its yardstick"""

    def __init__(self, fam, cls):
        self.fam, self.cls, self.d = fam, cls, {}

    def check(self, c, got, what=""):
        for k, v in H.distances(self.fam, c, got).items():
            self.d[k] = max(self.d.get(k, 0.0), v)
        bad = H.violations(self.fam, c, got)
        assert not bad, f"{what}{c}: " + ", ".join(f"{k}: distance {v:.3e} > bound {b:.3e}" for k, v, b in bad)

    def report(self):
        Y = H.yardsticks(self.fam, self.cls)
        print(f"heads: {self.fam:3s} {self.cls:11s} " + "; ".join(f"{k} {v / H.U:.2f} / {Y[k] / H.U:.2f}" for k, v in self.d.items()))


# ------------------------------------------------------------------------------------------------ the MLP head through the C ABI
def _desc(c):
    from dgvit_amd import _lib
    d = _lib.dgvit_mlp_desc()
    d.batch, d.nseg, d.n1, d.n2, d.n3, d.towers, d.heads3 = c.B, len(c.ks), c.n1, c.n2, c.n3, c.towers, c.heads3
    for s, k in enumerate(c.ks):
        d.kx[s], d.ldx[s] = k, k + c.pad[s]
    return d


def run_mlp(lib, c, inp=None, backward=True):
    """forward (and backward on the forward's h1 / h2) -> outputs by the names of H.mlp_eval, after the canary checks"""
    inp = H.mlp_inputs(c) if inp is None else inp
    d, B = _desc(c), c.B
    xs = [Buf(data=H.padded_input(c, inp, s), off=c.x_off if s == 0 else 0, fill=NAN) for s in range(len(c.ks))]
    params = [Buf(data=q, off=c.w1_off[t] // 4 if i == 0 else 0, fill=NAN) for t in range(c.towers) for i, q in enumerate(inp["params"][t])]
    h1, h2, y = Buf(c.towers * B * c.n1), Buf(c.towers * B * c.n2), Buf(c.towers * c.heads3 * B * c.n3)
    _ok(lib.dgvit_mlp_head_forward(ctypes.byref(d), _tab(xs), _tab(params), _p(h1), _p(h2), _p(y), _st()), f"forward {c.name}")
    torch.cuda.synchronize()
    for b, what in ((h1, "h1"), (h2, "h2"), (y, "y")):
        b.check(f"{c.name} {what}")
    H1, H2, Y = h1.numpy(c.towers, B, c.n1), h2.numpy(c.towers, B, c.n2), y.numpy(c.towers, c.heads3, B, c.n3)
    out = {}
    for t in range(c.towers):
        out[f"h1.{t}"], out[f"h2.{t}"] = H1[t], H2[t]
        for j in range(c.heads3):
            out[f"y.{t}.{j}"] = Y[t, j]
    if not backward:
        return out
    nsc = lib.dgvit_mlp_head_backward_scratch_floats(ctypes.byref(d))
    assert nsc > 0
    sc = Buf(nsc)
    dys = [None if f"dy.{t}.{j}" in c.nulls else Buf(data=inp["dy"][t][j], fill=NAN) for t in range(c.towers) for j in range(c.heads3)]
    dins = [None if f"din.{s}" in c.nulls else Buf(B * k) for s, k in enumerate(c.ks)]
    shapes = H.param_shapes(c)
    dpars = [None if f"dpar.{t}.{i}" in c.nulls else Buf(int(np.prod(s)), off=c.g_off) for t in range(c.towers) for i, s in enumerate(shapes)]
    _ok(lib.dgvit_mlp_head_backward(ctypes.byref(d), _tab(xs), _tab(params), _p(h1), _p(h2), _tab(dys), _tab(dins), _tab(dpars), _p(sc), nsc,
                                    _st()), f"backward {c.name}")
    torch.cuda.synchronize()
    sc.check(f"{c.name} scratch")
    for b, what in ((h1, "h1"), (h2, "h2"), (y, "y")):
        b.check(f"{c.name} {what} (backward)")
    for s, b in enumerate(dins):
        if b is not None:
            b.check(f"{c.name} dx.{s}")
            out[f"dx.{s}"] = b.numpy(B, c.ks[s])
    for n, b in enumerate(dpars):
        t, i = divmod(n, len(shapes))
        name = f"{H.PARAM_KINDS[i]}.{t}" if i < 4 else f"{H.PARAM_KINDS[i]}.{t}.{(i - 4) // 2}"
        if b is None:
            continue
        unused = i >= 4 and f"dy.{t}.{(i - 4) // 2}" in c.nulls        # the third layer of a NULL dy gets no gradient
        b.check(f"{c.name} {name}", written=not unused)
        if not unused:
            out[name] = b.numpy(*shapes[i])
    return out


def _dense(c):
    return c._replace(pad=(0,) * len(c.ks), x_off=0)


@pytest.mark.parametrize("cls", H.MLP_CLASSES)
def test_mlp_head(lib, cls):
    w = Worst("mlp", cls)
    for c in H.mlp_cases(cls):
        if not H.admitted(c):
            continue
        got = run_mlp(lib, c)
        w.check(c, got)
        assert_same(got, run_mlp(lib, c), f"{c.name}: two runs")
        if cls == "exact":
            ref, _ = H.mlp_reference(c)
            for k, v in ref.items():
                assert np.array_equal(got[k].astype(np.float64), v), f"{c.name} {k}: not the fp64 result"
        if any(c.pad) or c.x_off:
            assert_same(got, run_mlp(lib, _dense(c)), f"{c.name}: strided against contiguous")
        if c.nulls:
            base = run_mlp(lib, c._replace(nulls=()))
            keys = [k for k in got if H.kind_of(k) in ("y", "h1", "h2")] if any(n.startswith("dy.") for n in c.nulls) else list(got)
            assert_same(got, base, f"{c.name}: NULL slots against none", keys)
    w.report()


def _tower(c, inp, t):
    return (c._replace(towers=1, w1_off=(c.w1_off[t],), nulls=()),
            {"x": inp["x"], "params": [inp["params"][t]], "dy": [inp["dy"][t]]})


def test_twin_head_equals_its_two_towers(lib):
    for c in [c for c in H.mlp_cases("normal") if c.towers == 2 and not c.nulls]:
        inp, twin = H.mlp_inputs(c), run_mlp(lib, c)
        single = [run_mlp(lib, *_tower(c, inp, t)) for t in range(2)]
        for k, v in twin.items():
            parts = k.split(".")
            if parts[0] == "dx":
                want = (torch.from_numpy(single[0][k]) + torch.from_numpy(single[1][k])).numpy()
            else:
                want = single[int(parts[1])][".".join([parts[0], "0"] + parts[2:])]
            assert same_bits(v, want), f"{c.name} {k}: twin differs from its towers"


def test_rows_do_not_depend_on_other_blocks(lib):
    c70 = H._c("blocks", 70, (20, 12, 1), 32, 64, 3, 2, 2)
    inp = H._draw(c70, 0)

    def rows(n):
        sub = {"x": [x[:n] for x in inp["x"]], "params": inp["params"], "dy": [[d[:n] for d in r] for r in inp["dy"]]}
        return run_mlp(lib, c70._replace(B=n), sub, backward=False)
    o70, o33, o32 = rows(70), rows(33), rows(32)
    for k in o70:
        assert same_bits(o70[k][:32], o32[k]), f"{k}: rows [0, 32) of B = 70 against B = 32"
        assert same_bits(o70[k][32], o33[k][32]), f"{k}: row 32 of B = 70 against B = 33"


@pytest.mark.parametrize("g_off", [0, 1], ids=["vector", "scalar"])
def test_partial_path_is_the_sum_of_its_blocks(lib, g_off):
    c = next(c for c in H.mlp_cases("normal") if H.nwg(c.B) == 2 and H.last_rows(c.B) == "32")._replace(g_off=g_off)
    inp, got = H.mlp_inputs(c), run_mlp(lib, c)
    halves = []
    for r0 in (0, 32):
        sub = {"x": [x[r0:r0 + 32] for x in inp["x"]], "params": inp["params"], "dy": [[d[r0:r0 + 32] for d in r] for r in inp["dy"]]}
        halves.append(run_mlp(lib, c._replace(B=32), sub))
    for k, v in got.items():
        if H.kind_of(k) in H.PARAM_KINDS:
            want = (torch.from_numpy(halves[0][k]) + torch.from_numpy(halves[1][k])).numpy()
            assert same_bits(v, want), f"{k}: partial path differs from direct(rows 0..31) + direct(rows 32..63)"
        else:
            assert same_bits(v, np.concatenate([halves[0][k], halves[1][k]])), k


# ------------------------------------------------------------------------------------------------ tanh-Gaussian through the C ABI
def run_tg(lib, c, i):
    B, A = c.B, c.A
    mean, raw, eps = (Buf(data=i[k], fill=NAN) for k in ("mean", "raw", "eps"))
    scale, bias = Buf(data=i["scale"], fill=NAN), Buf(data=i["bias"], fill=NAN)
    action, logp, tmean, dmean, dls = Buf(B * A), Buf(B), Buf(B * A), Buf(B * A), Buf(B * A)
    _ok(lib.dgvit_tanh_gaussian_forward(_p(mean), _p(raw), _p(eps), _p(scale), _p(bias), c.scale_n, i["lo"], i["hi"], _p(action), _p(logp),
                                        _p(tmean), B, A, _st()), "tanh_gaussian_forward")
    ups = [None if i[k] is None else Buf(data=i[k], fill=NAN) for k in ("d_action", "d_log_prob", "d_tanh_mean")]
    _ok(lib.dgvit_tanh_gaussian_backward(_p(mean), _p(raw), _p(eps), _p(scale), c.scale_n, i["lo"], i["hi"], _p(ups[0]), _p(ups[1]), _p(ups[2]),
                                         _p(dmean), _p(dls), B, A, _st()), "tanh_gaussian_backward")
    torch.cuda.synchronize()
    for b, what in ((action, "action"), (logp, "log_prob"), (tmean, "tanh_mean"), (dmean, "dmean"), (dls, "dlog_std")):
        b.check(f"{c} {what}")
    return {"action": action.numpy(B, A), "log_prob": logp.numpy(B), "tanh_mean": tmean.numpy(B, A), "dmean": dmean.numpy(B, A),
            "dlog_std": dls.numpy(B, A)}


FWD = ("action", "log_prob", "tanh_mean")


@pytest.mark.parametrize("cls", H.TG_CLASSES)
def test_tanh_gaussian(lib, cls):
    w = Worst("tg", cls)
    for n, c in enumerate(H.tg_cases(cls)):
        i = H.tg_inputs(c)
        got = run_tg(lib, c, i)
        w.check(c, got)
        assert_same(got, run_tg(lib, c, i), f"{c}: two runs")
        lo, hi = np.float32(i["lo"]), np.float32(i["hi"])
        outside = (i["raw"] < lo) | (i["raw"] > hi)
        assert (got["dlog_std"][outside] == 0).all(), f"{c}: a gradient passed the clamp"
        if not all(c.ups):         # a NULL upstream gradient is a zero tensor
            zeros = dict(i, **{k: np.zeros(s, np.float32) for k, s in (("d_action", (c.B, c.A)), ("d_log_prob", (c.B,)),
                                                                       ("d_tanh_mean", (c.B, c.A))) if i[k] is None})
            assert_same(got, run_tg(lib, c, zeros), f"{c}: NULL upstream against zeros")
        if n % 3 == 0 or cls == "clamp_edges":
            # log_std beyond a bound gives the forward bits of the bound; tanh_mean depends on neither log_std nor eps
            assert_same(got, run_tg(lib, c, dict(i, raw=np.clip(i["raw"], lo, hi))), f"{c}: clamped on the host", FWD)
            other = run_tg(lib, c, dict(i, raw=i["raw"][::-1].copy(), eps=i["eps"] * np.float32(-3)))
            assert same_bits(got["tanh_mean"], other["tanh_mean"]), f"{c}: tanh_mean depends on log_std or eps"
        if cls == "zero_eps":
            assert same_bits(got["action"], got["tanh_mean"]), f"{c}: eps = 0 must give action = tanh_mean"
    w.report()


# ------------------------------------------------------------------------------------------------ refusals
class _Args:
    """a valid small twin call whose every pointer has room for any of the refused shapes; `change` edits it"""
    N = 1 << 17

    def __init__(self, towers=2, nseg=2):
        from dgvit_amd import _lib
        self.d = _lib.dgvit_mlp_desc()
        self.d.batch, self.d.nseg, self.d.n1, self.d.n2, self.d.n3, self.d.towers, self.d.heads3 = 5, nseg, 32, 32, 2, towers, 2
        for s in range(3):
            self.d.kx[s], self.d.ldx[s] = 8, 8
        self.xs = [Buf(self.N, fill=0.0) for _ in range(4)]
        self.params = [Buf(self.N, fill=0.0) for _ in range(24)]
        self.outs = {k: Buf(self.N) for k in ("h1", "h2", "y", "scratch")}
        self.dys = [Buf(self.N, fill=0.0) for _ in range(6)]
        self.dins = [Buf(self.N) for _ in range(4)]
        self.dpars = [Buf(self.N) for _ in range(24)]
        self.param_ptrs = [b.ptr for b in self.params]
        self.short = 0

    def call(self, lib):
        o, pp = self.outs, self.param_ptrs
        rf = lib.dgvit_mlp_head_forward(ctypes.byref(self.d), _tab(self.xs), _tab(pp), _p(o["h1"]), _p(o["h2"]), _p(o["y"]), _st())
        nsc = lib.dgvit_mlp_head_backward_scratch_floats(ctypes.byref(self.d))
        nsc = min(max(nsc, 4), self.N) - self.short
        rb = lib.dgvit_mlp_head_backward(ctypes.byref(self.d), _tab(self.xs), _tab(pp), _p(o["h1"]), _p(o["h2"]), _tab(self.dys), _tab(self.dins),
                                         _tab(self.dpars), _p(o["scratch"]), nsc, _st())
        torch.cuda.synchronize()
        return rf, rb

    def untouched(self, what, forward_too=True):
        for k, b in list(self.outs.items()) + [(f"din{n}", b) for n, b in enumerate(self.dins)] + [(f"dpar{n}", b) for n, b in enumerate(self.dpars)]:
            if forward_too or k not in ("h1", "h2", "y"):
                b.check(f"refused call ({what}) {k}", written=False)


def _set(a, **kw):
    for k, v in kw.items():
        setattr(a.d, k, v)


def _kx0(v, ld=None):
    def f(a):
        a.d.kx[0], a.d.ldx[0] = v, v if ld is None else ld
    return f


def _misalign(n):
    def f(a):
        a.param_ptrs[n] += 4
    return f


REFUSALS = {
    "K0=513": _kx0(505), "n1=48": lambda a: _set(a, n1=48), "n1=160": lambda a: _set(a, n1=160), "n3=5": lambda a: _set(a, n3=5),
    "nseg=0": lambda a: _set(a, nseg=0), "nseg=4": lambda a: _set(a, nseg=4), "towers=3": lambda a: _set(a, towers=3),
    "ldx<kx": _kx0(8, 7), "W2 of tower 1 4-byte aligned": _misalign(8 + 2), "second W3 of tower 0 4-byte aligned": _misalign(6),
}


def test_refusals_leave_everything_alone(lib):
    for what, change in REFUSALS.items():
        a = _Args()
        change(a)
        rf, rb = a.call(lib)
        assert rf == ERR_ARG and rb == ERR_ARG, f"{what}: forward {rf}, backward {rb}"
        a.untouched(what)
    a = _Args()
    a.short = 1
    rf, rb = a.call(lib)                  # (the forward is valid here and runs)
    assert rf == 0 and rb == ERR_ARG, f"scratch one float short: forward {rf}, backward {rb}"
    a.untouched("scratch one float short", forward_too=False)
    a.short = 0
    assert a.call(lib) == (0, 0)
    # tanh_gaussian: A = 17, scale_n not in {1, A}, lo > hi
    ins, outs = [Buf(1024, fill=0.0) for _ in range(8)], [Buf(1024) for _ in range(5)]
    for what, (B, A, sn, lo, hi) in {"A=17": (4, 17, 1, -20.0, 2.0), "scale_n=2, A=3": (4, 3, 2, -20.0, 2.0), "scale_n=0": (4, 3, 0, -20.0, 2.0),
                                     "lo>hi": (4, 3, 3, 2.0, -20.0)}.items():
        rf = lib.dgvit_tanh_gaussian_forward(_p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), _p(ins[4]), sn, lo, hi, _p(outs[0]), _p(outs[1]),
                                             _p(outs[2]), B, A, _st())
        rb = lib.dgvit_tanh_gaussian_backward(_p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), sn, lo, hi, _p(ins[5]), _p(ins[6]), _p(ins[7]),
                                              _p(outs[3]), _p(outs[4]), B, A, _st())
        torch.cuda.synchronize()
        assert rf == ERR_ARG and rb == ERR_ARG, f"tanh_gaussian {what}: forward {rf}, backward {rb}"
        for b in outs:
            b.check(f"refused tanh_gaussian call ({what})", written=False)


# ------------------------------------------------------------------------------------------------ through the autograd wrappers
def test_through_the_wrappers(lib):
    from dgvit_amd import functional as F
    c = H.WRAPPER_CASE
    inp = H.mlp_inputs(c)

    def lin(w, b):
        m = torch.nn.Linear(w.shape[1], w.shape[0])
        m.weight.data.copy_(torch.from_numpy(w))
        m.bias.data.copy_(torch.from_numpy(b))
        return m.cuda()
    p = inp["params"][0]
    l1, l2, mean_l, log_std_l = lin(p[0], p[1]), lin(p[2], p[3]), lin(p[4], p[5]), lin(p[6], p[7])
    l1.bias.requires_grad_(False)                                        # frozen parameter
    wide = torch.full((c.B, c.ks[0] + c.pad[0]), NAN, device="cuda")
    wide[:, :c.ks[0]] = torch.from_numpy(inp["x"][0])
    wide.requires_grad_(True)
    x0, x1 = wide[:, :c.ks[0]], torch.from_numpy(inp["x"][1]).cuda()      # a column slice: ldx > kx; x1 without requires_grad
    assert x0.stride(0) == c.ks[0] + c.pad[0] and F.mlp_head_supported([x0, x1], [(l1, l2, [mean_l, log_std_l])])
    (mean, log_std), = F.mlp_head([x0, x1], [(l1, l2, [mean_l, log_std_l])])
    (mean * torch.from_numpy(inp["dy"][0][0]).cuda()).sum().backward()    # a loss on the mean only
    assert log_std_l.weight.grad is None and log_std_l.bias.grad is None and l1.bias.grad is None
    ref, _ = H.mlp_reference(c)
    got = {"y.0.0": mean, "y.0.1": log_std, "dx.0": wide.grad[:, :c.ks[0]], "dw1.0": l1.weight.grad, "dw2.0": l2.weight.grad, "db2.0": l2.bias.grad,
           "dw3.0.0": mean_l.weight.grad, "db3.0.0": mean_l.bias.grad}
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    assert bool((wide.grad[:, c.ks[0]:] == 0).all())
    keys = set(got)
    full = run_mlp(lib, c)
    assert keys | {"h1.0", "h2.0"} == set(ref) == set(full)
    assert_same(got, full, "wrapper against the C ABI", keys)
    w = Worst("mlp", "normal")
    w.check(c, dict(full, **got), "wrapper ")
    w.report()
    # tanh_gaussian_sample: saturated rows, per-action scale, tanh_mean unused
    t = H.TgCase("saturated", 257, 3, 3, (True, True, False))
    i = H.tg_inputs(t)
    dev = lambda a: torch.from_numpy(a).cuda()
    m, r = dev(i["mean"]).requires_grad_(True), dev(i["raw"]).requires_grad_(True)
    act, lp, tm = F.tanh_gaussian_sample(m, r, dev(i["eps"]), dev(i["scale"]), dev(i["bias"]), i["lo"], i["hi"])
    assert lp.shape == (t.B, 1)
    ((act * dev(i["d_action"])).sum() + (lp[:, 0] * dev(i["d_log_prob"])).sum()).backward()
    got = {"action": act, "log_prob": lp[:, 0], "tanh_mean": tm, "dmean": m.grad, "dlog_std": r.grad}
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    w = Worst("tg", "saturated")
    w.check(t, got, "wrapper ")
    assert_same(got, run_tg(lib, t, i), "tanh_gaussian_sample against the C ABI")
    w.report()
