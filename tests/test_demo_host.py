"""CPU (no GPU): learning from demonstrations -- the new entry points (dgvit_tanh_gaussian_log_prob, its backward,
dgvit_sac_bc_loss) and their argument checks, the Python checks of replay.sample_mixed / update_priorities_mixed, sac_losses.bc_loss /
nll_loss and the policies' log_prob, and the host restatement tests/demo_ref.py, pinned against torch.distributions.
Every library call here fails its argument check before any launch: the pointers are never dereferenced."""
import ctypes
import os

import pytest
import torch
from torch.distributions import Normal, TransformedDistribution
from torch.distributions.transforms import AffineTransform, TanhTransform

import demo_ref as D

FAKE = ctypes.c_void_p(0x1000)   # non-null, aligned, never read: only argument checks run
OFF2 = ctypes.c_void_p(0x1002)
NAMES = ["dgvit_tanh_gaussian_log_prob", "dgvit_tanh_gaussian_log_prob_backward", "dgvit_sac_bc_loss"]


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
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert L.SIGNATURES["dgvit_tanh_gaussian_log_prob"] == (I, [P] * 5 + [I, F, F, P, I, I, P])
    assert L.SIGNATURES["dgvit_tanh_gaussian_log_prob_backward"] == (I, [P] * 5 + [I, F, F, P, P, P, I, I, P])
    assert L.SIGNATURES["dgvit_sac_bc_loss"] == (I, [P, P, P, I, P, P, P, P, I, P, P, I, I, P])
    assert "replay" in dgvit_amd.__all__ and "sac_losses" in dgvit_amd.__all__ and "functional" in dgvit_amd.__all__
    assert dgvit_amd.replay.sample_mixed and dgvit_amd.replay.update_priorities_mixed and issubclass(dgvit_amd.replay.MixedBatch, dict)
    assert dgvit_amd.sac_losses.bc_loss and dgvit_amd.sac_losses.nll_loss and dgvit_amd.sac_losses.BCLoss._fields == ("loss", "used")
    assert dgvit_amd.functional.tanh_gaussian_log_prob and dgvit_amd.GoTPolicy.log_prob and dgvit_amd.GaussianPolicy.log_prob
    assert "normalised within that ring" in dgvit_amd.replay.sample_mixed.__doc__


def test_abi_version_is_unchanged(lib):
    assert lib.dgvit_abi_version() == 7


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _lp(lib, mean=FAKE, lsr=FAKE, action=FAKE, scale=FAKE, bias=FAKE, sn=1, lo=-20.0, hi=2.0, logp=FAKE, B=32, A=2):
    return lib.dgvit_tanh_gaussian_log_prob(mean, lsr, action, scale, bias, sn, lo, hi, logp, B, A, None)


def _lpb(lib, mean=FAKE, lsr=FAKE, action=FAKE, scale=FAKE, bias=FAKE, sn=1, lo=-20.0, hi=2.0, dlp=FAKE, dmean=FAKE, dls=FAKE, B=32, A=2):
    return lib.dgvit_tanh_gaussian_log_prob_backward(mean, lsr, action, scale, bias, sn, lo, hi, dlp, dmean, dls, B, A, None)


def _bc(lib, pred=FAKE, action=FAKE, mask=None, mask_u8=0, q1_demo=None, q2_demo=None, q1_pi=None, q2_pi=None, nll=0, out=FAKE, grads=None,
        B=32, A=2):
    return lib.dgvit_sac_bc_loss(pred, action, mask, mask_u8, q1_demo, q2_demo, q1_pi, q2_pi, nll, out, grads, B, A, None)


_Q4 = dict(q1_demo=FAKE, q2_demo=FAKE, q1_pi=FAKE, q2_pi=FAKE)
BAD = []
for call, name, ptrs in ((_lp, "tanh_gaussian_log_prob", ("mean", "lsr", "action", "scale", "bias", "logp")),
                         (_lpb, "tanh_gaussian_log_prob_backward", ("mean", "lsr", "action", "scale", "bias", "dlp", "dmean", "dls"))):
    BAD += [(call, name, {k: None}, b"null") for k in ptrs]
    BAD += [(call, name, {k: OFF2}, b"aligned") for k in ptrs]
    BAD += [(call, name, dict(B=0), b"B=0"), (call, name, dict(B=-2), b"B=-2"), (call, name, dict(A=0), b"A=0"), (call, name, dict(A=17), b"A=17"),
            (call, name, dict(B=1 << 28, A=16), b"B*A=4294967296"), (call, name, dict(sn=0), b"scale_n=0"), (call, name, dict(sn=3, A=2), b"scale_n=3"),
            (call, name, dict(sn=2, A=3), b"scale_n=2"), (call, name, dict(lo=3.0, hi=2.0), b"ls_min=3")]
BAD += [(_bc, "sac_bc_loss", {k: None}, b"null") for k in ("pred", "action", "out")]
BAD += [(_bc, "sac_bc_loss", {k: OFF2}, b"aligned") for k in ("pred", "action", "mask", "out", "grads")]
BAD += [(_bc, "sac_bc_loss", {**_Q4, k: OFF2}, b"aligned") for k in _Q4]
BAD += [(_bc, "sac_bc_loss", {k: v for k, v in _Q4.items() if k != drop}, b"3 of 4") for drop in _Q4]
BAD += [
    (_bc, "sac_bc_loss", dict(q1_demo=FAKE), b"1 of 4"),
    (_bc, "sac_bc_loss", dict(B=0), b"B=0"),
    (_bc, "sac_bc_loss", dict(B=-1), b"B=-1"),
    (_bc, "sac_bc_loss", dict(A=0), b"A=0"),
    (_bc, "sac_bc_loss", dict(A=17), b"A=17"),
    (_bc, "sac_bc_loss", dict(B=(1 << 19) + 1, A=2), b"B*A=1048578"),
    (_bc, "sac_bc_loss", dict(nll=2), b"nll=2"),
    (_bc, "sac_bc_loss", dict(nll=-1), b"nll=-1"),
    (_bc, "sac_bc_loss", dict(mask_u8=2, mask=FAKE), b"mask_u8=2"),
    (_bc, "sac_bc_loss", dict(nll=1, A=2, action=None), b"A=2 must be 1"),
    (_bc, "sac_bc_loss", dict(nll=1, A=1, action=None, **_Q4), b"Q-filter"),
]


def _id(b):
    return f"{b[1]}-" + "-".join(f"{k}={v if not isinstance(v, ctypes.c_void_p) else v.value}" for k, v in b[2].items())


@pytest.mark.parametrize("call, name, kw, word", BAD, ids=[_id(b) for b in BAD])
def test_bad_arguments_are_refused_before_any_launch(lib, call, name, kw, word):
    assert call(lib, **kw) == -1          # DGVIT_ERR_ARG
    msg = lib.dgvit_last_error()
    assert name.encode() + b":" in msg and word in msg, msg


def test_a_bool_mask_may_sit_at_any_address(lib):
    """mask_u8=1 reads bytes: an odd address passes the alignment check and the call stops at the next one (B=0)"""
    assert _bc(lib, mask=ctypes.c_void_p(0x1001), mask_u8=1, B=0) == -1
    assert b"B=0" in lib.dgvit_last_error()


# ------------------------------------------------------------------------------------------------ the Python checks: sample_mixed
def _fake(prioritized=False, obs=(6, 10), pstate=2, act=2, stored=5):
    """a ring that exists only as far as sample_mixed's host checks look: nothing of it lives on a device"""
    from dgvit_amd import replay
    r = object.__new__(replay.PrioritizedDeviceReplayBuffer if prioritized else replay.DeviceReplayBuffer)
    n = obs[0] * obs[1]
    r.fields = {"obs": n, "pobs": pstate, "act": act, "rew": 1, "next_obs": n, "next_pobs": pstate, "done": 1}
    r.shapes = {"obs": tuple(obs), "next_obs": tuple(obs), "pobs": (pstate,), "next_pobs": (pstate,), "act": (act,), "rew": (1,), "done": (1,)}
    r.store, r.stored, r.device = {"obs": torch.zeros(1)}, stored, torch.device("cpu")
    return r


def test_sample_mixed_refuses_bad_pairs():
    from dgvit_amd.replay import sample_mixed as sm
    a, b = _fake(), _fake()
    for bad in (None, (), [], a, [(a, 1)] * 5, "ab"):
        with pytest.raises(ValueError, match="pairs must be a list of 1 to 4"):
            sm(bad)
    for bad in ([a], [(a,)], [(a, 1, 2)], [(a, 1), 3]):
        with pytest.raises(ValueError, match=r"pairs\[\d\] must be \(ring, n\)"):
            sm(bad)
    for bad in ("ring", None, torch.zeros(3), dict()):
        with pytest.raises(ValueError, match=r"pairs\[1\]\[0\] must be a DeviceReplayBuffer"):
            sm([(a, 1), (bad, 1)])
    for bad in (-1, 1.0, 2.5, True, None, "3", torch.tensor(2)):
        with pytest.raises(ValueError, match=r"pairs\[1\]\[1\].* must be an int >= 0"):
            sm([(a, 1), (b, bad)])
    with pytest.raises(ValueError, match="names a ring that the list holds already"):
        sm([(a, 1), (b, 1), (a, 2)])
    with pytest.raises(ValueError, match="add up to 0 rows"):
        sm([(a, 0), (b, 0)])


@pytest.mark.parametrize("kw, what", [(dict(obs=(5, 7)), "obs_shape"), (dict(obs=(10, 6)), "obs_shape"), (dict(pstate=3), "pstate_dim"),
                                      (dict(act=1), "act_dim")])
def test_sample_mixed_refuses_rings_that_disagree(kw, what):
    from dgvit_amd.replay import sample_mixed as sm
    with pytest.raises(ValueError, match=f"must agree in {what}"):
        sm([(_fake(), 2), (_fake(), 0), (_fake(**kw), 1)])
    with pytest.raises(ValueError, match=f"must agree in {what}"):
        sm([(_fake(), 2), (_fake(**kw), 0)])          # a share of 0 does not excuse a ring that could never share a batch


@pytest.mark.parametrize("kw, word", [(dict(n_step=0), "n_step"), (dict(n_step=65), "n_step"), (dict(n_step=2.0), "n_step"), (dict(gamma=1.5), "gamma"),
                                      (dict(gamma=None), "gamma"), (dict(frame_stack=0), "frame_stack"), (dict(frame_stack=17), "frame_stack"),
                                      (dict(random_shift=-1), "random_shift"), (dict(random_shift=6), "random_shift"),
                                      (dict(random_shift=1.5), "random_shift"), (dict(beta=2.0), "beta"), (dict(beta=True), "beta")])
def test_sample_mixed_checks_the_keywords_of_sample(kw, word):
    from dgvit_amd.replay import sample_mixed as sm
    with pytest.raises(ValueError, match=word):
        sm([(_fake(), 2), (_fake(prioritized=True), 1)], **kw)


def test_sample_mixed_checks_the_per_ring_keywords():
    from dgvit_amd.replay import sample_mixed as sm
    u, p = _fake(), _fake(prioritized=True)
    t = torch.zeros(2)
    for name in ("uniforms", "indices"):
        for bad in (t, [None], [None, None, None], 3):
            with pytest.raises(ValueError, match=f"{name} must be None or a list with one entry per pair"):
                sm([(u, 2), (p, 2)], **{name: bad})
    with pytest.raises(ValueError, match=r"uniforms\[0\] must be None: pairs\[0\] is a uniform ring"):
        sm([(u, 2), (p, 2)], uniforms=[t, t])
    with pytest.raises(ValueError, match=r"indices\[1\] must be None: pairs\[1\] is a prioritized ring"):
        sm([(u, 2), (p, 2)], indices=[t.long(), t.long()])
    with pytest.raises(ValueError, match=r"uniforms\[1\] must be None or a tensor"):
        sm([(u, 2), (p, 2)], uniforms=[None, [0.5, 0.5]])
    with pytest.raises(ValueError, match=r"indices\[0\] must be None or a tensor"):
        sm([(u, 2), (p, 2)], indices=[[1, 2], None])
    # an entry holds exactly the ring's share: the row ranges are fixed by the shares, so fewer would leave rows unwritten and more
    # would write into the next ring's rows
    for bad in (torch.zeros(1, dtype=torch.int64), torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"indices\[0\] must hold 2 values"):
            sm([(u, 2), (p, 2)], indices=[bad, None])
        with pytest.raises(ValueError, match=r"indices\[1\] must hold 2 values"):
            sm([(p, 1), (u, 2)], indices=[None, bad])
    for bad in (torch.zeros(1), torch.zeros(3), torch.zeros(4)):
        with pytest.raises(ValueError, match=r"uniforms\[1\] must hold 2 values"):
            sm([(u, 2), (p, 2)], uniforms=[None, bad])
    for bad in (torch.zeros(2), torch.zeros(2, dtype=torch.bool), torch.zeros(2, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"indices\[0\] must be an integer tensor"):
            sm([(u, 2), (p, 2)], indices=[bad, None])
    # the entry of a ring with a share of 0 is not read, whatever its size (the call goes on to the next check: an empty ring)
    with pytest.raises(RuntimeError, match="cannot sample from an empty buffer"):
        sm([(u, 0), (_fake(stored=0), 2)], indices=[torch.zeros(7, dtype=torch.int64), None])
    with pytest.raises(RuntimeError, match="cannot sample from an empty buffer"):
        sm([(_fake(stored=0), 2), (p, 0)], uniforms=[None, torch.zeros(7)])


def test_sample_mixed_on_an_empty_ring_raises_what_sample_raises():
    from dgvit_amd.replay import sample_mixed as sm
    with pytest.raises(RuntimeError, match="cannot sample from an empty buffer"):
        sm([(_fake(), 2), (_fake(stored=0), 1)])
    with pytest.raises(RuntimeError, match="cannot sample from an empty buffer"):
        sm([(_fake(prioritized=True, stored=0), 1)])


def test_update_priorities_mixed_checks_its_arguments():
    from dgvit_amd import replay
    td = torch.zeros(4)
    for bad in (dict(indexes=torch.zeros(4), counts=(4,)), None, [1, 2]):
        with pytest.raises(ValueError, match="batch must be what sample_mixed returned"):
            replay.update_priorities_mixed(bad, td)
    batch = replay.MixedBatch(indexes=torch.zeros(4, dtype=torch.int64), counts=(3, 1))
    with pytest.raises(ValueError, match="batch must be what sample_mixed returned"):
        replay.update_priorities_mixed(batch, td)       # no rings
    batch.rings = (_fake(), _fake(prioritized=True))
    for bad in (None, [0.0] * 4, torch.zeros(3), torch.zeros(4, 2), torch.zeros(1, 4), torch.zeros(5, 1)):
        with pytest.raises(ValueError, match=r"priorities must be \(4,\) or \(4, 1\)"):
            replay.update_priorities_mixed(batch, bad)
    with pytest.raises(ValueError, match="priorities must be an fp32 tensor"):
        replay.update_priorities_mixed(batch, torch.zeros(4, dtype=torch.float64))     # the prioritized ring's own refusal, of its row range
    batch.rings = (_fake(), _fake())
    replay.update_priorities_mixed(batch, td)           # no prioritized ring: nothing to do, nothing touched


# ------------------------------------------------------------------------------------------------ the Python checks: the losses
def test_bc_loss_checks_its_arguments():
    import dgvit_amd
    from dgvit_amd import sac_losses as S
    z = torch.zeros
    for bad in (z(4), z(4, 17), z(0, 2), None):
        with pytest.raises(ValueError, match="bc_loss: pred "):
            S.bc_loss(bad, z(4, 2))
    for bad in (z(4, 3), z(5, 2), z(8), None):
        with pytest.raises(ValueError, match="bc_loss: action "):
            S.bc_loss(z(4, 2), bad)
    pair = (z(4, 2), z(4, 2))
    for kw in (dict(q_demo=pair), dict(q_pi=pair)):
        with pytest.raises(ValueError, match="given together or not at all"):
            S.bc_loss(z(4, 2), z(4, 2), **kw)
    for bad in (z(4, 2), (z(4, 2),), (z(4, 2),) * 3, None):
        if bad is not None:
            with pytest.raises(ValueError, match=r"bc_loss: q_demo must be the pair"):
                S.bc_loss(z(4, 2), z(4, 2), q_demo=bad, q_pi=pair)
            with pytest.raises(ValueError, match=r"bc_loss: q_pi must be the pair"):
                S.bc_loss(z(4, 2), z(4, 2), q_demo=pair, q_pi=bad)
    with pytest.raises(ValueError, match=r"bc_loss: q_demo\[1\] "):
        S.bc_loss(z(4, 2), z(4, 2), q_demo=(z(4, 2), z(4, 3)), q_pi=pair)
    with pytest.raises(ValueError, match=r"bc_loss: q_pi\[0\] "):
        S.bc_loss(z(4, 2), z(4, 2), q_demo=pair, q_pi=(z(5, 2), z(4, 2)))
    for bad in (z(5), z(4, 2), z(2, 2), [1, 1, 1, 1]):
        with pytest.raises(ValueError, match="bc_loss: mask must be"):
            S.bc_loss(z(4, 2), z(4, 2), mask=bad)
    for bad in (z(4, dtype=torch.int64), z(4, 1, dtype=torch.float64), z(4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="bc_loss: mask must be bool or float32"):
            S.bc_loss(z(4, 2), z(4, 2), mask=bad)
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):        # there is no CPU path
        S.bc_loss(z(4, 2), z(4, 2), mask=z(4, dtype=torch.bool))
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):
        S.bc_loss(z(4, 2), z(4, 2))
    with pytest.raises(dgvit_amd.DgvitError, match="fp32 only|ROCm device"):
        S.bc_loss(z(4, 2, dtype=torch.float64), z(4, 2, dtype=torch.float64))
    meta = torch.device("meta")            # another device than the CPU's, without a GPU: the tensors of a call lie on one device
    with pytest.raises(ValueError, match="bc_loss: action is on meta, pred on cpu"):
        S.bc_loss(z(4, 2), z(4, 2, device=meta))
    with pytest.raises(ValueError, match=r"bc_loss: q_pi\[1\] is on meta, pred on cpu"):
        S.bc_loss(z(4, 2), z(4, 2), q_demo=pair, q_pi=(z(4, 2), z(4, 2, device=meta)))


def test_nll_loss_checks_its_arguments():
    import dgvit_amd
    from dgvit_amd import sac_losses as S
    z = torch.zeros
    for bad in (z(4, 2), z(4, 1, 1), z(0, 1), z(()), None, [0.0]):
        with pytest.raises(ValueError, match="nll_loss: log_prob must be"):
            S.nll_loss(bad)
    with pytest.raises(ValueError, match="nll_loss: mask must be"):
        S.nll_loss(z(4, 1), mask=z(3))
    with pytest.raises(TypeError):
        S.nll_loss(z(4, 1), q_demo=(z(4, 2), z(4, 2)), q_pi=(z(4, 2), z(4, 2)))      # the Q-filter is bc_loss's (see nll_loss)
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):
        S.nll_loss(z(4))


def test_log_prob_checks_its_arguments():
    import dgvit_amd
    from dgvit_amd import functional as F, sac_networks as N
    z, one, zero = torch.zeros, torch.tensor(1.0), torch.tensor(0.0)
    with pytest.raises(TypeError, match="must be tensors"):
        F.tanh_gaussian_log_prob(z(4, 2), z(4, 2), [[0.0, 0.0]] * 4, one, zero, -20, 2)
    for m, l, a in ((z(4), z(4), z(4)), (z(4, 2), z(4, 3), z(4, 2)), (z(4, 2), z(4, 2), z(5, 2)), (z(4, 2, 1), z(4, 2, 1), z(4, 2, 1))):
        with pytest.raises(ValueError, match=r"must be \(B, A\) alike"):
            F.tanh_gaussian_log_prob(m, l, a, one, zero, -20, 2)
    with pytest.raises(ValueError, match=r"A=17 must be in \[1, 16\]"):
        F.tanh_gaussian_log_prob(z(4, 17), z(4, 17), z(4, 17), one, zero, -20, 2)
    for sc, bi in ((torch.ones(3), z(3)), (torch.ones(2), zero), (one, z(2))):
        with pytest.raises(ValueError, match="scale and bias must hold 1 or A=2 values alike"):
            F.tanh_gaussian_log_prob(z(4, 2), z(4, 2), z(4, 2), sc, bi, -20, 2)
    with pytest.raises(ValueError, match="ls_min=3 must not exceed ls_max=2"):
        F.tanh_gaussian_log_prob(z(4, 2), z(4, 2), z(4, 2), one, zero, 3, 2)
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):
        F.tanh_gaussian_log_prob(z(4, 2), z(4, 2), z(4, 2), one, zero, -20, 2)
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):
        F.tanh_gaussian_log_prob(z(0, 2), z(0, 2), z(0, 2), one, zero, -20, 2)       # the empty batch is a device path too

    class Stub:
        action_scale, action_bias = one, zero
    for bad in (z(4, 3), z(5, 2), z(4), None, [[0.0, 0.0]] * 4):
        with pytest.raises(ValueError, match=r"log_prob: action must be a \(4, 2\) tensor"):
            N._log_prob(Stub(), z(4, 2), z(4, 2), bad)


# ------------------------------------------------------------------------------------------------ the restatement
def _case(B, A, per_action, seed, ymax=None):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    scale = (0.5 + torch.rand(A, generator=g, dtype=torch.float64)) if per_action else torch.tensor(1.7, dtype=torch.float64)
    bias = n(A) if per_action else torch.tensor(-0.3, dtype=torch.float64)
    y = torch.tanh(1.5 * n(B, A))
    if ymax is not None:
        y = y.clamp(-ymax, ymax)
    return n(B, A), 1.5 * n(B, A) - 1.0, y * scale + bias, scale, bias, y


@pytest.mark.parametrize("B, A, per_action", [(1, 1, False), (37, 2, False), (37, 2, True), (64, 3, True), (9, 16, True)])
def test_log_prob_is_the_exact_density_up_to_its_epsilon(B, A, per_action):
    """against torch.distributions' tanh-Gaussian, the exact density without the 1e-6: log(u + eps) - log u lies in [0, eps / u] with
    u = scale (1 - y^2), so the restatement is below the exact value by at most sum_a 1e-6 / (scale_a (1 - y_a^2)); |y| <= 0.9 keeps
    that bound at 5e-6 per action, so a wrong term of the formula cannot hide in it"""
    mean, lsr, action, scale, bias, y = _case(B, A, per_action, 10 * B + A, ymax=0.9)
    std = lsr.clamp(D.LOG_SIG_MIN, D.LOG_SIG_MAX).exp()
    dist = TransformedDistribution(Normal(mean, std), [TanhTransform(), AffineTransform(bias, scale)])
    exact = dist.log_prob(action).sum(1, keepdim=True)
    got = D.log_prob(mean, lsr, action, scale, bias)
    bound = (1e-6 / (scale * (1 - y * y))).expand(B, A).sum(1, keepdim=True)
    assert got.shape == (B, 1) and float(bound.max()) < 16 * 1.1e-5
    slack = 1e-12 * exact.abs().max()
    assert bool((exact - got >= -slack).all()) and bool((exact - got <= bound + slack).all()), (exact - got, bound)
    assert float((exact - got).max()) > 0.25 * float(bound.min()), "the epsilon is there"


def test_actions_at_and_beyond_the_bounds_take_the_value_at_the_clip():
    mean, lsr, action, scale, bias, _ = _case(12, 3, True, 5)
    y_clip = torch.full((12, 3), D.CLIP, dtype=torch.float64)
    y_clip[::2] = -D.CLIP
    at_clip = D.log_prob(mean, lsr, y_clip * scale + bias, scale, bias)
    sign = torch.sign(y_clip)
    for beyond in (1.0, 1.0 + 1e-9, 1.5, 40.0):
        got = D.log_prob(mean, lsr, sign * beyond * scale + bias, scale, bias)
        assert torch.isfinite(got).all()
        torch.testing.assert_close(got, at_clip, rtol=1e-9, atol=0)     # (y_clip * scale + bias - bias) / scale rounds within 1e-16 of the clip
    x = 0.5 * torch.log((1 + y_clip) / (1 - y_clip))
    assert float(x.abs().max()) == pytest.approx(7.2543, abs=1e-3)          # atanh(1 - 1e-6) = 0.5 log(2e6 - 1)
    inside = D.log_prob(mean, lsr, sign * 0.999 * scale + bias, scale, bias)
    assert not torch.allclose(inside, at_clip, rtol=1e-3)


def test_the_clamp_of_log_std_passes_the_gradient_inside_its_bounds_only():
    mean, _, action, scale, bias, _ = _case(6, 2, False, 3)
    lsr = torch.tensor([[-25.0, -20.0], [-20.0 - 1e-9, 0.3], [2.0, 2.0 + 1e-9], [5.0, -1.0], [D.LOG_SIG_MIN, D.LOG_SIG_MAX], [0.0, 1.0]],
                       dtype=torch.float64, requires_grad=True)
    mean.requires_grad_(True)
    D.log_prob(mean, lsr, action, scale, bias).sum().backward()
    inside = (lsr.detach() >= D.LOG_SIG_MIN) & (lsr.detach() <= D.LOG_SIG_MAX)
    assert torch.equal(lsr.grad == 0, ~inside) and inside.sum() == 8
    x = torch.atanh(D.squash_inverse(action, scale, bias))
    ls = lsr.detach().clamp(D.LOG_SIG_MIN, D.LOG_SIG_MAX)
    e = (x - mean.detach()) * torch.exp(-ls)
    torch.testing.assert_close(mean.grad, e * torch.exp(-ls), rtol=1e-12, atol=0)            # the kernel's closed forms
    torch.testing.assert_close(lsr.grad[inside], (e * e - 1)[inside], rtol=1e-12, atol=0)


def test_the_losses_of_the_restatement():
    g = torch.Generator().manual_seed(0)
    pred, act = torch.randn(7, 3, generator=g, dtype=torch.float64), torch.randn(7, 3, generator=g, dtype=torch.float64)
    loss, used = D.bc_loss(pred, act)
    assert float(used) == 7 and torch.equal(loss, torch.nn.functional.mse_loss(pred, act, reduction="none").mean(1).sum() / 7)
    mask = torch.tensor([1, 0, 1, 1, 0, 0, 1], dtype=torch.bool)
    loss, used = D.bc_loss(pred, act, mask)
    assert float(used) == 4
    torch.testing.assert_close(loss, ((pred[mask] - act[mask]) ** 2).mean(), rtol=1e-14, atol=0)
    w = torch.tensor([0.5, 0, 0.25, 1, 0, 0, 2.0], dtype=torch.float64)
    loss, used = D.bc_loss(pred, act, w)
    assert float(used) == 3.75
    # the filter: strict, a tie does not apply
    qd = (torch.tensor([[1.0], [1.0], [0.0]]).double().expand(3, 2), torch.tensor([[2.0], [2.0], [5.0]]).double().expand(3, 2))
    qp = (torch.tensor([[0.5], [1.0], [9.0]]).double().expand(3, 2), torch.tensor([[3.0], [1.0], [9.0]]).double().expand(3, 2))
    assert D.row_weights(3, qd[0], None, qd, qp).tolist() == [1.0, 0.0, 0.0]
    # nothing applies: zero, with zero gradients, not NaN
    p = pred.clone().requires_grad_(True)
    loss, used = D.bc_loss(p, act, torch.zeros(7))
    loss.backward()
    assert float(loss.detach()) == 0 and float(used) == 0 and torch.equal(p.grad, torch.zeros_like(p))
    lp = torch.randn(7, 1, generator=g, dtype=torch.float64)
    loss, used = D.nll_loss(lp, mask)
    torch.testing.assert_close(loss, -lp[mask].mean(), rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------------ the demonstration-regularised learner
def test_the_demo_learner_meets_the_cap_in_fp32_and_the_term_matters():
    """the case of tests/test_gpu_demo.py's trajectory: the reference's own fp32 run stays at rounding distance from its fp64 run, and a
    run without the demonstration term stands far outside the rule (its fp64 run stands where the device's result will)"""
    import sac_trajectory_ref as T
    case, stores, idx = D.make_demo_case()
    r64, r32 = (D.run_demo(case, stores, idx, dt, **T.BASE_KW) for dt in (torch.float64, torch.float32))
    Y = T.distance(r32, r64, T.BASE_LR)
    assert T.cap_violations(Y, D.DEMO_STEPS, T.BASE_LR) == []
    assert 0 < Y["qf"] < 1e-5 and 0 < Y["pl"] < 1e-4
    assert r64["used"] == [2.0] * D.DEMO_STEPS and all(b > 0.1 for b in r64["bc"]), "two demonstration rows per step, and they are not yet cloned"
    r, bad = T.check(T.distance(D.run_demo(case, stores, idx, torch.float64, lam=0.0, **T.BASE_KW), r64, T.BASE_LR), Y, D.DEMO_STEPS, T.BASE_LR)
    assert bad and max(r.values()) >= 100 * T.MARGIN
