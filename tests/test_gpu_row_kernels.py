"""GPU: the row kernels of csrc/norm.hip and csrc/misc_bf16.hip on every dispatch path and on ill-conditioned rows, against fp64.

The case tables, row classes, references, yardsticks and the rule live in tests/row_kernel_cases.py and are checked on the CPU by
tests/test_row_kernel_matrix_host.py.  Here every case runs through the diagnostic library's row-kernel entry points (RMSNorm through
the product ABI, which already takes every argument) with
  * NaN in everything a kernel must not read: the rows a row step skips, the padding behind a row of a padded matrix, the rows the
    column sum's row map skips, the floats before an unaligned base;
  * outputs inside canary buffers: the skipped rows, the padding and the guard zones must keep the canary;
  * the rule: distance to fp64 <= max(2 Y, floor), Y the fp32 yardstick of the (family, output, class) from the CPU alone;
  * the bit-exact conditions: xout == (x + delta) [+ delta2] in torch fp32; y of an add variant == y of the plain kernel on that sum;
    strided == contiguous on the gathered rows; dxb == bf16(dx); queued == direct reduction; a NULL dgamma / dbeta / dg / dxb / mean leaves
    every other output unchanged; residual_add and transpose == torch; constant rows give y = beta; two runs give the same bits;
    refusals return an error and leave the canaries.

Measured on an MI355X (the lines every test prints; `kernel distance / yardstick Y`, largest over the admitted cases of the class; the bound
is max(2 Y, floor), floor 4.8e-7 for row outputs and (T + 8) 2^-24 for sums).  The narrowest pass is dgamma of the fp32 backward on
1000 + N(0, 1) rows, 7.32e-5 against 2 Y = 7.36e-5; the RMSNorm dx figures equal Y because the worst cases are rows of three elements (dx is what
is left of u after a projection that removes most of it), where the kernel and its numpy restatement round alike.
  family   class      output kernel / Y
  ln       normal     y 2.17e-07 / 2.32e-07; dx 2.03e-07 / 2.53e-07; rstd 1.50e-07 / 1.81e-07; mean 3.35e-08 / 5.43e-08; dgamma 1.21e-07 / 1.28e-07; dbeta 7.10e-08 / 1.02e-07
  ln       offset     y 7.02e-05 / 6.53e-05; dx 2.18e-05 / 3.62e-05; rstd 1.38e-07 / 1.56e-05; mean 1.20e-07 / 1.31e-07; dgamma 7.32e-05 / 3.68e-05; dbeta 9.91e-08 / 1.08e-07
  ln       tight      y 1.30e-05 / 2.07e-05; dx 1.22e-06 / 2.56e-06; rstd 9.43e-08 / 1.16e-06; mean 1.87e-07 / 2.14e-07; dgamma 2.20e-05 / 1.40e-05; dbeta 7.80e-08 / 9.94e-08
  ln       spike      y 2.07e-07 / 3.17e-07; dx 5.90e-08 / 5.90e-08; rstd 1.90e-07 / 2.58e-07; mean 1.45e-08 / 1.99e-08; dgamma 9.21e-08 / 5.59e-07; dbeta 7.44e-08 / 1.06e-07
  ln       scaled     y 2.33e-07 / 2.55e-07; dx 2.29e-07 / 3.46e-07; rstd 1.36e-07 / 1.72e-07; mean 2.40e-08 / 4.75e-08; dgamma 1.06e-07 / 1.45e-07; dbeta 6.93e-08 / 8.77e-08
  ln       const      y 0.00e+00 / 0.00e+00; dx 2.19e-07 / 2.96e-07; rstd 5.48e-08 / 4.17e-08; mean 0.00e+00 / 0.00e+00; dgamma 0.00e+00 / 6.10e-05; dbeta 7.41e-08 / 1.05e-07
  lnb_fwd  normal     y 2.44e-08 / 2.44e-08; rstd 1.00e-07 / 1.25e-07; mean 2.53e-08 / 5.43e-08
  lnb_fwd  offset     y 2.52e-05 / 2.20e-05; rstd 8.54e-08 / 2.29e-05; mean 9.59e-08 / 1.07e-07
  lnb_fwd  tight      y 3.85e-06 / 3.87e-06; rstd 9.91e-08 / 8.02e-07; mean 1.30e-07 / 1.52e-07
  lnb_fwd  spike      y 5.18e-13 / 0.00e+00; rstd 1.20e-07 / 1.81e-07; mean 1.99e-08 / 1.99e-08
  lnb_fwd  scaled     y 8.58e-10 / 0.00e+00; rstd 1.05e-07 / 1.13e-07; mean 2.10e-08 / 4.75e-08
  lnb_fwd  const      y 1.81e-08 / 1.61e-08; rstd 8.51e-08 / 1.26e-07; mean 4.63e-08 / 4.76e-08
  lnb_bwd  normal     dx 2.31e-07 / 2.45e-07; dgamma 9.71e-08 / 1.43e-07; dbeta 2.26e-09 / 7.32e-09
  lnb_bwd  offset     dx 3.30e-05 / 6.87e-05; dgamma 3.13e-05 / 3.67e-05; dbeta 4.88e-09 / 2.79e-09
  lnb_bwd  tight      dx 1.62e-06 / 1.98e-06; dgamma 2.20e-05 / 1.41e-05; dbeta 2.23e-09 / 4.43e-09
  lnb_bwd  spike      dx 5.90e-08 / 5.90e-08; dgamma 1.23e-07 / 3.70e-07; dbeta 1.40e-08 / 1.40e-08
  lnb_bwd  scaled     dx 2.72e-07 / 2.92e-07; dgamma 1.27e-07 / 1.02e-07; dbeta 4.49e-09 / 5.19e-09
  lnb_bwd  const      dx 2.47e-07 / 2.56e-07; dgamma 0.00e+00 / 6.10e-05; dbeta 4.40e-09 / 4.40e-09
  rms      normal     y 1.89e-07 / 2.76e-07; dx 1.19e-06 / 1.19e-06; dg 1.15e-07 / 1.80e-07
  rms      zero_rows  y 1.63e-07 / 2.64e-07; dx 3.87e-06 / 3.87e-06; dg 9.19e-08 / 1.79e-07
  rms      tiny       y 1.41e-07 / 1.41e-07; dx 1.40e-07 / 1.40e-07; dg 9.40e-08 / 1.88e-07
  rms      scaled     y 1.83e-07 / 2.37e-07; dx 1.33e-06 / 1.33e-06; dg 9.54e-08 / 1.90e-07
  rms      spike      y 5.75e-08 / 5.75e-08; dx 1.09e-06 / 1.09e-06; dg 1.62e-07 / 8.29e-07
  rms      huge       y 1.89e-07 / 3.19e-07; dx 1.68e-06 / 1.68e-06; dg 9.45e-08 / 1.99e-07
  colsum   normal     sum 5.18e-08 / 1.82e-07
(bf16 y distances are what is left after half a bf16 ulp of the reference.)
"""
import ctypes

import numpy as np
import pytest
import torch

import row_kernel_cases as R

pytestmark = pytest.mark.gpu

CANARY = 555.0
GUARD = 256           # elements on each side of a buffer (a multiple of 8: fp32 and bf16 payloads stay 16-byte aligned)
NAN = float("nan")


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


@pytest.fixture
def F(amd):
    with amd.diagnostic_library():
        yield amd.functional


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(dtype).cuda()


class Rows:
    """T logical rows of D elements, logical row r at physical row r * rs, inside guard zones.  Everything but the logical rows holds
    ``fill`` (NaN for inputs: reading it poisons the result; the canary for outputs); ``t`` is the flat payload the library gets."""

    def __init__(self, T, D, rs=1, data=None, fill=CANARY, dtype=torch.float32):
        self.T, self.D, self.rs, self.fill = T, D, rs, fill
        n = ((T - 1) * rs + 1) * D
        self.buf = torch.full((GUARD + n + GUARD,), fill, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()
        if data is not None:
            self.t.view(-1, D)[::rs] = data.reshape(T, D)

    def logical(self):
        return self.t.view(-1, self.D)[::self.rs].clone()

    def numpy(self):
        r = self.logical().float().cpu().numpy()
        return r.reshape(-1) if self.T == 1 else r

    def assert_rest_untouched(self, what, logical_too=False):
        rest = self.buf.clone()
        if not logical_too:
            rest[GUARD:GUARD + self.t.numel()].view(-1, self.D)[::self.rs] = self.fill
        ok = torch.isnan(rest).all() if self.fill != self.fill else (rest == torch.full_like(rest, self.fill)).all()
        assert bool(ok), f"{what}: wrote outside its rows" + (" (a refused call wrote)" if logical_too else "")


def vec(n, dtype=torch.float32):
    return Rows(1, n, 1, dtype=dtype)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Worst:
    """largest kernel distance per output over the admitted cases of a (family, class), beside its yardstick"""

    def __init__(self, fam, cls):
        self.fam, self.cls, self.d = fam, cls, {}

    def check(self, c, got, what=""):
        if not R.admitted(self.fam, c):
            return
        for k, v in R.distances(self.fam, c, got).items():
            self.d[k] = max(self.d.get(k, 0.0), v)
        bad = R.violations(self.fam, c, got)
        assert not bad, f"{what}{c}: " + ", ".join(f"{k}: distance {v:.3e} > bound {b:.3e}" for k, v, b in bad)

    def report(self):
        Y = R.yardsticks(self.fam, self.cls)
        for k, v in self.d.items():
            ratio = f"{v / Y[k]:.2f}" if Y[k] > 0 else ("0" if v == 0 else "inf")
            print(f"row kernels: {self.fam:8s} {self.cls:10s} {k:7s} hip {v:.2e}  Y {Y[k]:.2e}  hip/Y {ratio}")


# ------------------------------------------------------------------------------------------------ fp32 LayerNorm
def _ln_run(F, i, T, D, rs, *, backward=True, grouped=False, dgamma=True, dbeta=True):
    """forward, then the backward on the forward's statistics; every output as numpy after the canary checks"""
    x = Rows(T, D, rs, dev(i["x"]), fill=NAN)
    gamma, beta = dev(i["gamma"]), dev(i["beta"])
    y, mean, rstd = Rows(T, D, rs), vec(T), vec(T)
    F.op_diag_layernorm_fwd(x.t, gamma, beta, T, D, rs, y=y.t, mean=mean.t, rstd=rstd.t)
    out = {"y": y, "mean": mean, "rstd": rstd}
    if backward:
        dy, dres = Rows(T, D, rs, dev(i["dy"]), fill=NAN), Rows(T, D, rs, dev(i["dres"]), fill=NAN)
        dx, dg, db = Rows(T, D, rs), vec(D), vec(D)
        F.op_diag_layernorm_bwd(dy.t, x.t, mean.t, rstd.t, gamma, T, D, rs, dres=dres.t, dx=dx.t, dgamma=dg.t if dgamma else None,
                                dbeta=db.t if dbeta else None, grouped=grouped)
        out.update(dx=dx, dgamma=dg, dbeta=db)
    torch.cuda.synchronize()
    for k, r in out.items():
        r.assert_rest_untouched(f"{k} (T {T}, D {D}, row step {rs})", logical_too=(k == "dgamma" and not dgamma) or (k == "dbeta" and not dbeta))
    return {k: r.numpy() for k, r in out.items() if not ((k == "dgamma" and not dgamma) or (k == "dbeta" and not dbeta))}


@pytest.mark.parametrize("cls", R.LN_CLASSES)
def test_layernorm_fp32(F, cls):
    w = Worst("ln", cls)
    dense = {}
    for c in R.ln_cases(cls):
        i = R.ln_inputs(c.cls, c.T, c.D)
        got = _ln_run(F, i, c.T, c.D, c.rs)
        w.check(c, got)
        again = _ln_run(F, i, c.T, c.D, c.rs)
        assert all(same_bits(got[k], again[k]) for k in got), f"{c}: two runs differ"
        if c.rs == 1:
            dense[(c.T, c.D)] = got
        else:
            assert all(same_bits(got[k], dense[(c.T, c.D)][k]) for k in got), f"{c}: strided and contiguous rows differ"
        queued = _ln_run(F, i, c.T, c.D, c.rs, grouped=True)
        assert all(same_bits(got[k], queued[k]) for k in got), f"{c}: queued and direct reduction differ"
        for frozen in ("dgamma", "dbeta"):
            part = _ln_run(F, i, c.T, c.D, c.rs, **{frozen: False})
            assert frozen not in part and all(same_bits(got[k], part[k]) for k in part), f"{c}: NULL {frozen} changed another output"
        if cls == "const":
            assert same_bits(got["y"], np.broadcast_to(i["beta"], got["y"].shape).copy()), f"{c}: constant rows must give y = beta"
            assert (got["mean"] == 3.75).all()
    # D = 1028: the forward takes it (rows of five chunks), the backward refuses it
    Y = R.yardsticks("ln", cls)
    for rs in (1, 5):
        x = R.ln_rows(cls, 5, R.LN_D_FWD_ONLY, 7)
        i = {"x": x, "gamma": np.linspace(0.5, 1.5, x.shape[1], dtype=R.F32), "beta": np.linspace(-1, 1, x.shape[1], dtype=R.F32)}
        got = _ln_run(F, i, 5, x.shape[1], rs, backward=False)
        for k, v in R.ln_distances(got, R.ln_ref64(i["x"], i["gamma"], i["beta"])).items():
            assert v <= R.bound(Y[k], R.ROW_FLOOR), f"D = 1028 forward, row step {rs}, {cls}: {k} {v:.3e}"
    w.report()


def test_layernorm_backward_refuses_wide_rows(amd, F):
    """D = 1028 (fp32 and bf16 backward, bf16 forward): an error, nothing written"""
    T, D = 5, R.LN_D_FWD_ONLY
    g = torch.Generator().manual_seed(3)
    x, dy = torch.randn(T, D, generator=g).cuda(), torch.randn(T, D, generator=g).cuda()
    gamma, stat = torch.ones(D, device="cuda"), torch.ones(T, device="cuda")
    dx, dxb, dg, db, y = Rows(T, D), Rows(T, D, dtype=torch.bfloat16), vec(D), vec(D), Rows(T, D, dtype=torch.bfloat16)
    with pytest.raises(amd.DgvitError, match="1028"):
        F.op_diag_layernorm_bwd(dy.view(-1), x.view(-1), stat, stat, gamma, T, D, dx=dx.t, dgamma=dg.t, dbeta=db.t)
    with pytest.raises(amd.DgvitError, match="1028"):
        F.op_diag_layernorm_bwd_bf16(dy.to(torch.bfloat16).view(-1), x.view(-1), stat, stat, gamma, T, D, dx=dx.t, dxb=dxb.t, dgamma=dg.t, dbeta=db.t)
    with pytest.raises(amd.DgvitError, match="1028"):
        F.op_diag_layernorm_fwd_bf16(x.view(-1), gamma, gamma, T, D, y=y.t)
    with pytest.raises(amd.DgvitError):        # the joint form has no row step
        F.op_diag_layernorm_fwd_bf16(x.view(-1)[:T * 64], gamma[:64], gamma[:64], 2, 64, 2, delta=dy.to(torch.bfloat16).view(-1), y=y.t)
    torch.cuda.synchronize()
    for name, r in (("dx", dx), ("dxb", dxb), ("dgamma", dg), ("dbeta", db), ("y", y)):
        r.assert_rest_untouched(name, logical_too=True)


# ------------------------------------------------------------------------------------------------ bf16 LayerNorm forward
def _lnb_fwd_run(F, i, x_np, T, D, rs, nadd, has_xout, has_stat):
    bf = torch.bfloat16
    x = Rows(T, D, rs, dev(x_np), fill=NAN)
    delta = Rows(T, D, rs, dev(i["delta"], bf), fill=NAN, dtype=bf) if nadd >= 1 else None
    delta2 = Rows(T, D, rs, dev(i["delta2"], bf), fill=NAN, dtype=bf) if nadd == 2 else None
    out = {"y": Rows(T, D, rs, dtype=bf)}
    if has_xout:
        out["xout"] = Rows(T, D, rs)
    if has_stat:
        out["mean"], out["rstd"] = vec(T), vec(T)
    F.op_diag_layernorm_fwd_bf16(x.t, dev(i["gamma"]), dev(i["beta"]), T, D, rs, delta=delta and delta.t, delta2=delta2 and delta2.t,
                                 xout=out["xout"].t if has_xout else None, y=out["y"].t, mean=out["mean"].t if has_stat else None,
                                 rstd=out["rstd"].t if has_stat else None)
    torch.cuda.synchronize()
    for k, r in out.items():
        r.assert_rest_untouched(f"{k} (T {T}, D {D}, row step {rs}, ADD {nadd})")
    return {k: r.numpy() for k, r in out.items()}


@pytest.mark.parametrize("cls", R.LN_CLASSES)
def test_layernorm_bf16_forward_variants(F, cls):
    w = Worst("lnb_fwd", cls)
    plain = {}
    for c in R.lnb_fwd_cases(cls):
        i = R.lnb_inputs(c.cls, c.T, c.D)
        nadd, has_xout, has_stat = R.LNB_VARIANTS[c.variant]
        row_in = R.lnb_row_input(c)
        key = (c.T, c.D, nadd)
        if key not in plain:          # the plain kernel, contiguous, on the fp32 sum an add variant must form
            plain[key] = _lnb_fwd_run(F, i, row_in, c.T, c.D, 1, 0, False, True)
        got = _lnb_fwd_run(F, i, i["x"], c.T, c.D, c.rs, nadd, has_xout, has_stat)
        w.check(c, {k: v for k, v in got.items() if k != "xout"})
        if has_xout:
            assert same_bits(got["xout"], row_in), f"{c}: xout != (x + delta) [+ delta2] in fp32"
        for k in ("y", "mean", "rstd"):
            if k in got:
                assert same_bits(got[k], plain[key][k]), f"{c}: {k} differs from the plain contiguous kernel on the same rows"
        again = _lnb_fwd_run(F, i, i["x"], c.T, c.D, c.rs, nadd, has_xout, has_stat)
        assert all(same_bits(got[k], again[k]) for k in got), f"{c}: two runs differ"
        if cls == "const" and nadd == 0:
            want = torch.from_numpy(np.array(i["beta"])).to(torch.bfloat16).float().numpy()
            assert same_bits(got["y"], np.broadcast_to(want, got["y"].shape).copy()), f"{c}: constant rows must give y = bf16(beta)"
    w.report()


# ------------------------------------------------------------------------------------------------ bf16 LayerNorm backward
def _lnb_bwd_run(F, i, T, D, rs, stats, *, dxb=True, params=True):
    bf = torch.bfloat16
    x, dres = Rows(T, D, rs, dev(i["x"]), fill=NAN), Rows(T, D, rs, dev(i["dres"]), fill=NAN)
    dy = Rows(T, D, rs, dev(i["dy"], bf), fill=NAN, dtype=bf)
    out = {"dx": Rows(T, D, rs), "dxb": Rows(T, D, rs, dtype=bf), "dgamma": vec(D), "dbeta": vec(D)}
    F.op_diag_layernorm_bwd_bf16(dy.t, x.t, stats[0], stats[1], dev(i["gamma"]), T, D, rs, dres=dres.t, dx=out["dx"].t,
                                 dxb=out["dxb"].t if dxb else None, dgamma=out["dgamma"].t if params else None,
                                 dbeta=out["dbeta"].t if params else None)
    torch.cuda.synchronize()
    skipped = ([] if dxb else ["dxb"]) + ([] if params else ["dgamma", "dbeta"])
    for k, r in out.items():
        r.assert_rest_untouched(f"{k} (T {T}, D {D}, row step {rs})", logical_too=k in skipped)
    return {k: r.numpy() for k, r in out.items() if k not in skipped}


@pytest.mark.parametrize("cls", R.LN_CLASSES)
def test_layernorm_bf16_backward(F, cls):
    w = Worst("lnb_bwd", cls)
    dense = {}
    for c in R.lnb_bwd_cases(cls):
        i = R.lnb_inputs(c.cls, c.T, c.D)
        mean, rstd = vec(c.T), vec(c.T)          # the statistics of the bf16 configuration's own forward
        F.op_diag_layernorm_fwd_bf16(dev(i["x"]).view(-1), dev(i["gamma"]), dev(i["beta"]), c.T, c.D, mean=mean.t, rstd=rstd.t)
        stats = (mean.t, rstd.t)
        got = _lnb_bwd_run(F, i, c.T, c.D, c.rs, stats)
        w.check(c, {k: v for k, v in got.items() if k != "dxb"})
        want = torch.from_numpy(got["dx"]).to(torch.bfloat16).float().numpy()
        assert same_bits(got["dxb"], want), f"{c}: dxb != bf16(dx)"
        again = _lnb_bwd_run(F, i, c.T, c.D, c.rs, stats)
        assert all(same_bits(got[k], again[k]) for k in got), f"{c}: two runs differ"
        if c.rs == 1:
            dense[(c.T, c.D)] = got
        else:
            assert all(same_bits(got[k], dense[(c.T, c.D)][k]) for k in got), f"{c}: strided and contiguous rows differ"
        for kw in ({"dxb": False}, {"params": False}):
            part = _lnb_bwd_run(F, i, c.T, c.D, c.rs, stats, **kw)
            assert all(same_bits(got[k], part[k]) for k in part), f"{c}: a NULL output ({kw}) changed another output"
    w.report()


# ------------------------------------------------------------------------------------------------ RMSNorm (product ABI)
class Window:
    """(B, D) logical matrix with leading dimension ld inside guard zones; padding and guards hold ``fill``"""

    def __init__(self, B, D, ld, data=None, fill=CANARY):
        self.B, self.D, self.ld, self.fill = B, D, ld, fill
        self.buf = torch.full((GUARD + B * ld + GUARD,), fill, device="cuda")
        self.win = self.buf[GUARD:GUARD + B * ld].view(B, ld)
        if data is not None:
            self.win[:, :D] = data

    def ptr(self):
        return ctypes.c_void_p(self.win.data_ptr())

    def numpy(self):
        return self.win[:, :self.D].cpu().numpy()

    def assert_rest_untouched(self, what, logical_too=False):
        rest = self.buf.clone()
        if not logical_too:
            rest[GUARD:GUARD + self.B * self.ld].view(self.B, self.ld)[:, :self.D] = self.fill
        assert bool((rest == self.fill).all()), f"{what}: wrote outside its window"


def _rms_run(lib, i, B, D, ldx, lddx, *, want_dg=True, backward=True):
    from dgvit_amd import _lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    x = Window(B, D, ldx, dev(i["x"]), fill=NAN)
    g, dy = dev(i["g"]), dev(i["dy"])
    y, dx, dg = Window(B, D, D), Window(B, D, lddx), Window(1, D, D)
    _lib.check(lib.dgvit_rmsnorm_forward(x.ptr(), ldx, p(g), y.ptr(), B, D, st), "dgvit_rmsnorm_forward")
    rc = 0
    if backward:
        nsc = int(lib.dgvit_rmsnorm_backward_scratch_floats(B, D))
        sc = torch.full((max(nsc, 4),), NAN, device="cuda")
        rc = lib.dgvit_rmsnorm_backward(p(dy), x.ptr(), ldx, p(g), dx.ptr(), lddx, dg.ptr() if want_dg else None, p(sc), nsc, B, D, st)
    torch.cuda.synchronize()
    y.assert_rest_untouched("y")
    dx.assert_rest_untouched("dx", logical_too=rc != 0)
    dg.assert_rest_untouched("dg", logical_too=rc != 0 or not want_dg)
    out = {"y": y.numpy()}
    if backward and rc == 0:
        out["dx"] = dx.numpy()
        if want_dg:
            out["dg"] = dg.numpy().reshape(-1)
    return rc, out


@pytest.mark.parametrize("cls", R.RMS_CLASSES)
def test_rmsnorm(amd, cls):
    """ldx = D + 3 (NaN behind every row), lddx = D + 5 (canary behind every row); the same bits with dense rows and with dg NULL"""
    lib = amd.load_library()
    w = Worst("rms", cls)
    for c in R.rms_cases(cls):
        i = R.rms_inputs(c.cls, c.B, c.D)
        rc, got = _rms_run(lib, i, c.B, c.D, c.D + 3, c.D + 5)
        assert rc == 0, lib.dgvit_last_error()
        w.check(c, got)
        for what, args, kw in (("two runs", (c.D + 3, c.D + 5), {}), ("dense rows", (c.D, c.D), {}), ("dg NULL", (c.D + 3, c.D + 5), {"want_dg": False})):
            rc, other = _rms_run(lib, i, c.B, c.D, *args, **kw)
            assert rc == 0 and all(same_bits(got[k], other[k]) for k in other), f"{c}: {what}: the bits differ"
    w.report()


def test_rmsnorm_backward_refuses_wide_rows(amd):
    lib = amd.load_library()
    D = 4097
    i = {"x": np.ones((3, D), dtype=R.F32), "g": np.ones(D, dtype=R.F32), "dy": np.ones((3, D), dtype=R.F32)}
    rc, out = _rms_run(lib, i, 3, D, D + 3, D + 5)       # (the forward has no such limit; the helper checks that dx and dg kept the canary)
    assert rc == -1 and lib.dgvit_last_error() and "dx" not in out
    assert np.allclose(out["y"], 1.0, rtol=0, atol=1e-6)      # rows of ones: x / sqrt(D) * sqrt(D) * g = 1


# ------------------------------------------------------------------------------------------------ fp32 column sums
def test_colsum(F):
    w = Worst("colsum", "normal")
    for c in R.col_cases():
        i = R.col_inputs(c)
        base = dev(i["buf"])
        a = base[c.off:]
        assert base.data_ptr() % 16 == 0 and a.data_ptr() % 16 == 4 * c.off
        runs = []
        for _ in range(2):
            out = vec(c.N)
            F.op_diag_colsum(a, c.lda, c.T, c.N, c.rgrp, out=out.t)
            torch.cuda.synchronize()
            out.assert_rest_untouched(f"{c}")
            runs.append(out.numpy())
        w.check(c, {"sum": runs[0]})
        assert same_bits(runs[0], runs[1]), f"{c}: two runs differ"
    w.report()


# ------------------------------------------------------------------------------------------------ exact helpers of the bf16 configuration
def test_residual_add_bf16_is_exact(F):
    bf = torch.bfloat16
    for rows, D, rs in R.RESIDUAL_CASES:
        g = torch.Generator().manual_seed(rows * 31 + D)
        x, d = torch.randn(rows, D, generator=g) * 3, torch.randn(rows, D, generator=g).to(bf)
        xr, dr, out = Rows(rows, D, rs, x.cuda(), fill=NAN), Rows(rows, D, rs, d.cuda(), fill=NAN, dtype=bf), Rows(rows, D, rs)
        F.op_diag_residual_add_bf16(xr.t, dr.t, rows, D, rs, xout=out.t)
        torch.cuda.synchronize()
        out.assert_rest_untouched(f"residual_add {rows} x {D}, row step {rs}")
        assert torch.equal(out.logical().cpu(), x + d.float()), (rows, D, rs)


def test_transpose_cast_is_exact(F):
    for rows, cols in R.TRANSPOSE_SHAPES:
        src = torch.from_numpy(R.transpose_input(rows, cols))
        dst = Rows(cols, rows, 1, dtype=torch.bfloat16)
        F.op_diag_transpose_cast_bf16(src.cuda(), dst=dst.t.view(cols, rows))
        torch.cuda.synchronize()
        dst.assert_rest_untouched(f"transpose {rows} x {cols}")
        assert torch.equal(dst.logical().cpu(), src.to(torch.bfloat16).T.contiguous()), (rows, cols)
