"""CPU (no GPU): conservative Q-learning -- the new entry points (dgvit_mlp_head_forward_shared, its sizing function and
backward, dgvit_sac_cql_penalty) and their argument checks, the Python checks of q_many / sample_many / cql_penalty / mlp_head(share=),
and the host restatement tests/cql_ref.py, pinned against torch.logsumexp + autograd in float64.
Every library call here fails its argument check before any launch: the pointers are never dereferenced."""
import ctypes
import os

import pytest
import torch

import cql_ref as R

FAKE = ctypes.c_void_p(0x1000)   # non-null, 16-byte aligned, never read: only argument checks run
OFF2 = ctypes.c_void_p(0x1002)
NAMES = ["dgvit_mlp_head_forward_shared", "dgvit_mlp_head_backward_shared_scratch_floats", "dgvit_mlp_head_backward_shared",
         "dgvit_sac_cql_penalty"]
MAX_SHARE = 256


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


def test_symbols_are_exported_bound_and_documented(lib):
    from dgvit_amd import _lib as L
    import dgvit_amd
    raw = ctypes.CDLL(L.LIB_PATH)
    with open(os.path.join(os.path.dirname(L.LIB_PATH), os.pardir, "include", "dgvit_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES, name
        assert name + "(" in header, name
    P, I, F, LL, T = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong, ctypes.POINTER(ctypes.c_void_p)
    D, S = ctypes.POINTER(L.dgvit_mlp_desc), ctypes.POINTER(ctypes.c_int)
    assert L.SIGNATURES["dgvit_mlp_head_forward_shared"] == (I, [D, S, T, T, P, P, P, P])
    assert L.SIGNATURES["dgvit_mlp_head_backward_shared_scratch_floats"] == (LL, [D, S])
    assert L.SIGNATURES["dgvit_mlp_head_backward_shared"] == (I, [D, S, T, T, P, P, T, T, T, P, LL, P])
    assert L.SIGNATURES["dgvit_sac_cql_penalty"] == (I, [P] * 6 + [I, P, F, F, F, I, P, P, P, I, I, I, P])
    assert dgvit_amd.sac_losses.cql_penalty and dgvit_amd.sac_losses.CQLLoss._fields == ("loss", "weight_loss", "gap", "used")
    assert dgvit_amd.GoTQNetwork.q_many and dgvit_amd.QNetwork.q_many and dgvit_amd.GoTPolicy.sample_many and dgvit_amd.GaussianPolicy.sample_many
    assert dgvit_amd.functional.MAX_HEAD_SHARE == MAX_SHARE and f"1 <= M <= {MAX_SHARE}" in header


def test_abi_version_is_unchanged(lib):
    assert lib.dgvit_abi_version() == 7


# ------------------------------------------------------------------------------------------------ argument checks: the shared head
def _desc(batch=12, ks=(64, 2), n1=128, n2=32, n3=2, towers=2, heads3=1, ld=None):
    from dgvit_amd import _lib as L
    d = L.dgvit_mlp_desc()
    d.batch, d.nseg, d.n1, d.n2, d.n3, d.towers, d.heads3 = batch, len(ks), n1, n2, n3, towers, heads3
    for s, k in enumerate(ks):
        d.kx[s], d.ldx[s] = k, (ld or ks)[s]
    return d


def _tab(n, null=None, ptr=FAKE):
    return (ctypes.c_void_p * n)(*[None if i == null else ptr.value for i in range(n)])


def _share(v):
    return None if v is None else (ctypes.c_int * len(v))(*v)


def _fwd(lib, share=(3, 1), desc=None, null_in=None, null_par=None, par=FAKE, h1=FAKE, h2=FAKE, y=FAKE, **kw):
    d = desc or _desc(**kw)
    return lib.dgvit_mlp_head_forward_shared(ctypes.byref(d), _share(share), _tab(d.nseg, null_in), _tab(12, null_par, par), h1, h2, y, None)


def _bwd(lib, share=(3, 1), desc=None, null_in=None, null_par=None, par=FAKE, h1=FAKE, h2=FAKE, dy=True, din=True, dpar=True, scratch=FAKE,
         floats=None, **kw):
    d = desc or _desc(**kw)
    if floats is None:
        floats = max(lib.dgvit_mlp_head_backward_shared_scratch_floats(ctypes.byref(d), _share(share)), 0)
    return lib.dgvit_mlp_head_backward_shared(ctypes.byref(d), _share(share), _tab(d.nseg, null_in), _tab(12, null_par, par), h1, h2,
                                              _tab(4) if dy else None, _tab(3) if din else None, _tab(12) if dpar else None, scratch, floats, None)


HEAD_BAD = []
for call in (_fwd, _bwd):
    HEAD_BAD += [
        (call, dict(share=None), b"null"),
        (call, dict(share=(0, 1)), b"share[0]=0"),
        (call, dict(share=(3, -1)), b"share[1]=-1"),
        (call, dict(share=(3, 2)), b"share[1]=2 differs"),
        (call, dict(share=(2, 3, 1), ks=(8, 8, 2), batch=12), b"share[1]=3 differs"),
        (call, dict(share=(5, 1)), b"batch=12 must be a multiple of the share count M=5"),
        (call, dict(share=(MAX_SHARE + 1, 1), batch=4 * (MAX_SHARE + 1)), b"M=257 must be at most 256"),
        (call, dict(share=(3, 1), batch=0), b"batch must be positive"),
        (call, dict(share=(3, 1, 1), ks=(8, 8, 8), n1=100), b"multiples of 32"),          # the restrictions of the head stay
        (call, dict(share=(3, 1), ks=(511, 2)), b"wider than 512"),
        (call, dict(share=(3, 1), ld=(63, 2)), b"bad input piece 0"),
        (call, dict(share=(3, 1), null_in=0), b"bad input piece 0"),
        (call, dict(share=(3, 1), null_par=2), b"parameter 2 of tower 0 is null"),
        (call, dict(share=(3, 1), par=OFF2), b"16-byte aligned"),
        (call, dict(share=(3, 1), h1=None), b"null"),
        (call, dict(share=(1, 1), h2=None), b"null"),              # all ones: the unshared call's checks
    ]
HEAD_BAD += [
    (_fwd, dict(y=None), b"null output"),
    (_bwd, dict(dy=False), b"null pointer"),
    (_bwd, dict(din=False), b"null pointer"),
    (_bwd, dict(dpar=False), b"null pointer"),
    (_bwd, dict(scratch=None), b"scratch"),
    (_bwd, dict(floats=0), b"scratch 0 <"),
]


@pytest.mark.parametrize("call, kw, word", HEAD_BAD, ids=[f"{c.__name__}-{i}" for i, (c, _, _) in enumerate(HEAD_BAD)])
def test_shared_head_refuses_bad_arguments_before_any_launch(lib, call, kw, word):
    assert call(lib, **kw) == -1          # DGVIT_ERR_ARG
    msg = lib.dgvit_last_error()
    assert b"mlp_head" in msg and word in msg, msg


def test_shared_scratch_one_float_short_is_refused(lib):
    """the shared call needs the unshared call's scratch plus the per-row buffers: the unshared size alone is too small"""
    d = _desc(batch=70, ks=(64, 2))
    base = lib.dgvit_mlp_head_backward_scratch_floats(ctypes.byref(d))
    need = lib.dgvit_mlp_head_backward_shared_scratch_floats(ctypes.byref(d), _share((10, 1)))
    assert need == base + 70 * 64
    for floats in (base, need - 1):
        assert _bwd(lib, share=(10, 1), desc=d, floats=floats) == -1
        assert f"scratch {floats} < {need}".encode() in lib.dgvit_last_error()


def test_shared_sizing(lib):
    f, g = lib.dgvit_mlp_head_backward_shared_scratch_floats, lib.dgvit_mlp_head_backward_scratch_floats
    for batch, ks, towers in ((15, (64, 2), 2), (70, (64, 2), 2), (36, (256, 32, 2), 2), (70, (64, 2), 1), (5, (64, 2), 2)):
        d = _desc(batch=batch, ks=ks, towers=towers)
        base = g(ctypes.byref(d))
        assert base > 0 and f(ctypes.byref(d), _share((1,) * len(ks))) == base, "all ones is the unshared sizing"
    d = _desc(batch=36, ks=(256, 32, 2))
    base = g(ctypes.byref(d))
    assert f(ctypes.byref(d), _share((9, 9, 1))) == base + 36 * 256 + 36 * 32
    assert f(ctypes.byref(d), _share((9, 1, 1))) == base + 36 * 256
    assert f(ctypes.byref(d), _share((1, 1, 4))) == base + 36 * 2                      # any piece may be the shared one
    d = _desc(batch=15, ks=(63, 2))
    assert f(ctypes.byref(d), _share((5, 1))) == g(ctypes.byref(d)) + ((15 * 63 + 3) & ~3), "each buffer rounded up to 4 floats"
    for bad in ((0, 1), (4, 1), (5, 3), (MAX_SHARE + 1, 1)):
        assert f(ctypes.byref(d), _share(bad)) == -1
    assert f(ctypes.byref(d), None) == -1 and f(None, _share((1, 1))) == -1


# ------------------------------------------------------------------------------------------------ argument checks: the penalty
def _cql(lib, q1c=FAKE, q2c=FAKE, q1d=FAKE, q2d=FAKE, log_w=None, mask=None, mask_u8=0, log_weight=None, weight=1.0, T=1.0, tau=0.0, lagrange=0,
         out=FAKE, grads=None, dlw=None, B=8, M=5, C=2):
    return lib.dgvit_sac_cql_penalty(q1c, q2c, q1d, q2d, log_w, mask, mask_u8, log_weight, weight, T, tau, lagrange, out, grads, dlw, B, M, C, None)


CQL_BAD = [({k: None}, b"null") for k in ("q1c", "q2c", "q1d", "q2d", "out")]
CQL_BAD += [({k: OFF2}, b"aligned") for k in ("q1c", "q2c", "q1d", "q2d", "log_w", "mask", "out", "grads")]
CQL_BAD += [
    (dict(log_weight=OFF2), b"aligned"),
    (dict(log_weight=FAKE, lagrange=1, dlw=OFF2), b"aligned"),
    (dict(B=0), b"B=0"), (dict(B=-3), b"B=-3"), (dict(M=0), b"M=0"), (dict(C=0), b"C=0"), (dict(C=17), b"C=17"),
    (dict(B=1 << 15, M=32, C=1), b"B*(M+1)*C=1081344"),
    (dict(B=(1 << 19) + 1, M=1, C=1), b"B*(M+1)*C=1048578"),
    (dict(mask_u8=2, mask=FAKE), b"mask_u8=2"),
    (dict(lagrange=2), b"lagrange=2"),
    (dict(T=0.0), b"temperature=0"), (dict(T=-1.0), b"temperature=-1"), (dict(T=float("inf")), b"temperature=inf"), (dict(T=float("nan")), b"temperature=nan"),
    (dict(weight=float("nan")), b"weight=nan"),
    (dict(lagrange=1), b"needs log_weight"),
    (dict(lagrange=1, log_weight=FAKE, tau=float("inf")), b"target_gap=inf"),
    (dict(dlw=FAKE), b"dlog_weight belongs to the Lagrange form"),
]


@pytest.mark.parametrize("kw, word", CQL_BAD, ids=[f"cql-{i}" for i in range(len(CQL_BAD))])
def test_cql_penalty_refuses_bad_arguments_before_any_launch(lib, kw, word):
    assert _cql(lib, **kw) == -1
    msg = lib.dgvit_last_error()
    assert b"sac_cql_penalty:" in msg and word in msg, msg


def test_a_bool_mask_may_sit_at_any_address(lib):
    assert _cql(lib, mask=ctypes.c_void_p(0x1001), mask_u8=1, B=0) == -1
    assert b"B=0" in lib.dgvit_last_error()


# ------------------------------------------------------------------------------------------------ the Python checks
def test_cql_penalty_checks_its_arguments():
    import dgvit_amd
    from dgvit_amd import sac_losses as S
    z = torch.zeros
    ok = (z(4, 3, 2), z(4, 3, 2), z(4, 2), z(4, 2))
    with pytest.raises(ValueError, match="exactly one of weight= .* and log_weight="):
        S.cql_penalty(*ok)
    with pytest.raises(ValueError, match="exactly one of weight= .* and log_weight="):
        S.cql_penalty(*ok, weight=1.0, log_weight=z(1))
    with pytest.raises(ValueError, match="target_gap needs log_weight="):
        S.cql_penalty(*ok, weight=1.0, target_gap=0.5)
    for bad in (True, "1", float("nan"), float("inf"), torch.tensor(1.0)):
        with pytest.raises(ValueError, match="weight must be a finite float"):
            S.cql_penalty(*ok, weight=bad)
    for bad in (z(2), 0.5, [0.0]):
        with pytest.raises(ValueError, match="log_weight must be a one-element tensor"):
            S.cql_penalty(*ok, log_weight=bad)
    for bad in (True, "1", float("nan"), z(1)):
        with pytest.raises(ValueError, match="target_gap must be a finite float"):
            S.cql_penalty(*ok, log_weight=z(1), target_gap=bad)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), True, None, z(1)):
        with pytest.raises(ValueError, match="temperature must be a finite float > 0"):
            S.cql_penalty(*ok, weight=1.0, temperature=bad)
    for bad in (z(4, 2), z(4, 3, 2, 1), None, [[0.0]]):
        with pytest.raises(ValueError, match=r"q1_cat must be \(B, M, C\)"):
            S.cql_penalty(bad, *ok[1:], weight=1.0)
    for bad in (z(0, 3, 2), z(4, 0, 2), z(4, 3, 17), z(1 << 15, 32, 1)):
        with pytest.raises(ValueError, match=r"cql_penalty: q1_cat is .*needs 1 <= B"):
            S.cql_penalty(bad, bad, z(bad.shape[0], bad.shape[2]), z(bad.shape[0], bad.shape[2]), weight=1.0)
    with pytest.raises(ValueError, match=r"q2_cat must be \(4, 3, 2\)"):
        S.cql_penalty(ok[0], z(4, 2, 2), ok[2], ok[3], weight=1.0)
    with pytest.raises(ValueError, match=r"q1_data must be \(4, 2\)"):
        S.cql_penalty(ok[0], ok[1], z(4, 3), ok[3], weight=1.0)
    with pytest.raises(ValueError, match=r"q2_data must be \(4, 2\)"):
        S.cql_penalty(ok[0], ok[1], ok[2], None, weight=1.0)
    for bad in (z(4, 2), z(4, 3, 1), z(3, 3)):
        with pytest.raises(ValueError, match=r"log_w must be \(4, 3\)"):
            S.cql_penalty(*ok, weight=1.0, log_w=bad)
    for bad in (z(5), z(4, 2), [1, 1, 1, 1]):
        with pytest.raises(ValueError, match="cql_penalty: mask must be"):
            S.cql_penalty(*ok, weight=1.0, mask=bad)
    with pytest.raises(ValueError, match="mask must be bool or float32"):
        S.cql_penalty(*ok, weight=1.0, mask=z(4, dtype=torch.int64))
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):        # there is no CPU path
        S.cql_penalty(*ok, weight=1.0)
    with pytest.raises(ValueError, match="cql_penalty: log_w is on meta, q1_cat on cpu"):
        S.cql_penalty(*ok, weight=1.0, log_w=z(4, 3, device="meta"))


class _Counting(torch.nn.Module):
    """stands where an encoder stands and fails the test if it is reached: the refusals come first"""

    def forward(self, *a, **k):
        raise AssertionError("the encoder ran before the argument checks")


def test_q_many_checks_its_arguments():
    import dgvit_amd
    z = torch.zeros
    got = dgvit_amd.GoTQNetwork(2, 2, 1, 2, 32, image_size=(24, 30), patch_size=(12, 10))
    cnn = dgvit_amd.QNetwork(2, 2)
    got.trans = _Counting()
    cnn._features = _Counting()
    for net, frames in ((got, z(4, 24, 30)), (cnn, z(4, 128, 160))):
        for bad in ([frames], [frames, z(4, 2), z(4, 3, 2)], frames, None):
            with pytest.raises(ValueError, match=r"q_many: inp must be \[istate, pstate\]"):
                net.q_many(bad, z(4, 3, 2))
        for bad in (z(4, 2), z(12, 2), z(4, 3, 3), z(4, 0, 2), z(4, 257, 2), None, z(4, 3, 2, 1)):
            with pytest.raises(ValueError, match=r"q_many: actions must be \(B, M, nb_actions\) = \(B, M, 2\) with 1 <= M <= 256"):
                net.q_many([frames, z(4, 2)], bad)
        with pytest.raises(ValueError, match="q_many: actions must be contiguous float32"):
            net.q_many([frames, z(4, 2)], z(4, 3, 2, dtype=torch.float64))
        with pytest.raises(ValueError, match="q_many: actions must be contiguous float32"):
            net.q_many([frames, z(4, 2)], z(4, 2, 3).transpose(1, 2))
        for bad in (z(5, 2), z(4), None):
            with pytest.raises(ValueError, match=r"q_many: pstate must be \(B, nb_pstate\) with the B = 4"):
                net.q_many([frames, bad], z(4, 3, 2))
        for bad in (frames[:3], z(4), None):
            with pytest.raises(ValueError, match="q_many: istate must be a batch of B = 4 frames"):
                net.q_many([bad, z(4, 2)], z(4, 3, 2))


def test_sample_many_checks_its_arguments():
    import dgvit_amd
    from dgvit_amd import sac_networks as N

    class Stub:
        def _head_outputs(self, inp):
            raise AssertionError("the networks ran before the argument checks")
    for bad in (0, -1, 2.0, True, None, "3", torch.tensor(2)):
        with pytest.raises(ValueError, match=r"sample_many: n must be an int >= 1 \(the result is \(B, n, nb_actions\)\)"):
            N._sample_many(Stub(), [None, None], bad)
    assert dgvit_amd.GoTPolicy.sample_many.__doc__ and dgvit_amd.GaussianPolicy.sample_many.__doc__


def test_mlp_head_share_checks_its_arguments():
    from dgvit_amd import functional as F
    z = torch.zeros
    lin = torch.nn.Linear
    towers = [(lin(10, 32), lin(32, 32), [lin(32, 2)])]
    xs = [z(4, 8), z(12, 2)]
    for bad in ((3,), (3, 1, 1), [3.0, 1], (True, 1), (0, 1), "31"):
        with pytest.raises(ValueError, match="share must hold one int >= 1 per input piece"):
            F.mlp_head(xs, towers, share=bad)
    for bad in ((3, 2), (257, 1)):
        with pytest.raises(ValueError, match="every share count is 1 or one common M <= 256"):
            F.mlp_head(xs, towers, share=bad)
    for bad in ((2, 1), (1, 1), (1, 3)):
        with pytest.raises(ValueError, match="piece s must be"):
            F.mlp_head(xs, towers, share=bad)
    assert F.mlp_head_supported(xs, towers) and F.mlp_head_supported(xs, towers, None) and F.mlp_head_supported(xs, towers, (3, 1))
    assert not F.mlp_head_supported(xs, towers, (257, 1)) and not F.mlp_head_supported(xs, towers, (3, 2)) and not F.mlp_head_supported(xs, towers, (3,))


def test_the_unfused_fallback_repeats_the_shared_pieces():
    """_head with widths the fused kernel does not take goes through the GEMM chain on repeat_interleave'd pieces (checked here up to the
    point where the chain needs a device)"""
    import dgvit_amd
    from dgvit_amd import sac_networks as N
    seen = {}

    def fake_lin(layer, x, relu=False):
        seen.setdefault("x", x)
        raise dgvit_amd.DgvitError("stop")
    lin = torch.nn.Linear
    towers = [(lin(10, 48), lin(48, 32), [lin(32, 2)])]          # 48: not a multiple of 32
    feat = torch.arange(4 * 8, dtype=torch.float32).reshape(4, 8)
    act = torch.arange(12 * 2, dtype=torch.float32).reshape(12, 2)
    orig, N._lin = N._lin, fake_lin
    try:
        with pytest.raises(dgvit_amd.DgvitError, match="stop"):
            N._head([feat, act], towers, share=[3, 1])
    finally:
        N._lin = orig
    assert torch.equal(seen["x"], torch.cat([feat.repeat_interleave(3, 0), act], 1))


# ------------------------------------------------------------------------------------------------ the restatement
def _autograd64(x, T, w, tau, mask):
    q = {k: (None if v is None else v.double().requires_grad_(k != "log_w")) for k, v in x.items()}
    B, M, C = q["q1_cat"].shape
    wb = R.row_weights(mask, B, torch.float64)
    used = wb.sum()
    gaps = []
    for qc, qd in ((q["q1_cat"], q["q1_data"]), (q["q2_cat"], q["q2_data"])):
        z = qc if q["log_w"] is None else qc - q["log_w"][:, :, None]
        lse = T * torch.logsumexp(z / T, dim=1)
        gaps.append((wb[:, None] * (lse - qd)).sum() / (used * C))
    loss = w * (gaps[0] + gaps[1] - 2 * tau)
    loss.backward()
    return dict(loss=loss.detach(), gap=torch.stack(gaps).detach(), used=used, dq1_cat=q["q1_cat"].grad, dq2_cat=q["q2_cat"].grad,
                dq1_data=q["q1_data"].grad, dq2_data=q["q2_data"].grad)


@pytest.mark.parametrize("shape, T, scale", R.CASES, ids=[f"{s}-T{t}" for s, t, _ in R.CASES])
@pytest.mark.parametrize("with_log_w", [False, True])
def test_the_restatement_is_logsumexp_under_autograd(shape, T, scale, with_log_w):
    x = R.inputs(shape, scale, 11, with_log_w)
    x64 = {k: None if v is None else v.double() for k, v in x.items()}
    for mask in (None, R.mixed_mask(shape[0]), R.mixed_mask(shape[0]).float() * 0.5):
        got = R.penalty(**x64, temperature=T, weight=0.7, mask=mask)
        want = _autograd64(x, T, 0.7, 0.0, mask)
        assert set(got) == set(R.OUTPUTS)
        for k in R.OUTPUTS:
            assert got[k].dtype == torch.float64 and got[k].shape == want[k].shape, k
            torch.testing.assert_close(got[k], want[k], rtol=1e-12, atol=1e-300, msg=lambda m, k=k: f"{k}: {m}")
        assert float(got["used"]) == (shape[0] if mask is None else float(mask.sum()))
        if mask is not None and mask.dtype == torch.bool:
            assert bool((got["dq1_cat"][~mask] == 0).all()) and bool((got["dq2_data"][~mask] == 0).all())
        sums = got["dq1_cat"].sum(1)                       # the softmax sums to one: w w_b / (used C) per (b, c)
        torch.testing.assert_close(sums, -got["dq1_data"], rtol=1e-12, atol=0)


def test_the_lagrange_pair_of_the_restatement():
    x = {k: None if v is None else v.double() for k, v in R.inputs((7, 30, 2), 1.0, 3, True).items()}
    lw = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    plain = R.penalty(**x, weight=float(torch.exp(lw.detach())))
    got = R.penalty(**x, log_weight=lw.detach(), target_gap=0.25)
    assert set(got) == set(R.OUTPUTS + R.LAGRANGE_OUTPUTS)
    w = torch.exp(lw.detach())[0]
    excess = got["gap"].sum() - 0.5
    torch.testing.assert_close(got["loss"], w * excess, rtol=1e-14, atol=0)
    torch.testing.assert_close(got["weight_loss"], -got["loss"], rtol=0, atol=0)
    torch.testing.assert_close(got["gap"], plain["gap"], rtol=0, atol=0)
    torch.testing.assert_close(got["dq1_cat"], plain["dq1_cat"], rtol=1e-14, atol=0)         # tau moves the value, not the gradients in q
    (-torch.exp(lw) * excess).sum().backward()
    torch.testing.assert_close(got["dlog_weight"], lw.grad, rtol=1e-14, atol=0)
    without = R.penalty(**x, log_weight=lw.detach())
    assert "weight_loss" not in without
    torch.testing.assert_close(without["loss"], plain["loss"], rtol=1e-14, atol=0)


def test_no_row_used_gives_exact_zeros():
    x = {k: None if v is None else v.double() for k, v in R.inputs((7, 30, 2), 50.0, 5, True).items()}
    for kw in (dict(weight=2.0), dict(log_weight=torch.tensor([0.3]), target_gap=0.25)):
        got = R.penalty(**x, temperature=0.1, mask=torch.zeros(7, dtype=torch.bool), **kw)
        for k, v in got.items():
            assert bool((v == 0).all()), k


def test_the_hard_case_is_finite_in_fp32():
    """(7, 30, 2) at T = 0.1 with q of scale 50: z / T lies beyond +-1000, where exp without the max subtraction overflows; the fp32
    evaluation of the restatement, the yardstick of the device test, is finite and non-zero in every output"""
    shape, T, scale = R.CASES[1]
    x = R.inputs(shape, scale, 11, True)
    assert float(((x["q1_cat"] - x["log_w"][:, :, None]) / T).abs().max()) > 1000
    y32 = R.penalty(**x, temperature=T, weight=0.7)
    y64 = R.penalty(**{k: v.double() for k, v in x.items()}, temperature=T, weight=0.7)
    for k in R.OUTPUTS:
        assert bool(torch.isfinite(y32[k]).all()) and float(y32[k].abs().max()) > 0, k
        assert float((y32[k].double() - y64[k]).abs().max() / y64[k].abs().max()) < 1e-5, k
