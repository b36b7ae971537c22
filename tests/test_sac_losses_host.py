"""CPU (no GPU): the SAC loss head's entry points (dgvit_sac_critic_loss, dgvit_sac_actor_loss, dgvit_sac_scale_grads), their argument
checks, the Python checks of dgvit_amd.sac_losses in front of them, and the host restatement tests/sac_losses_ref.py with its learner.
Every library call here fails its argument check before any launch: the pointers are never dereferenced."""
import ctypes
import os

import pytest
import torch

from helpers import O
import sac_losses_ref as R
import sac_trajectory_ref as T

FAKE = ctypes.c_void_p(0x1000)   # non-null, aligned, never read: only argument checks run
OFF2 = ctypes.c_void_p(0x1002)
NAMES = ["dgvit_sac_critic_loss", "dgvit_sac_actor_loss", "dgvit_sac_scale_grads"]
CFG, B, K, LR, SEED = T.BASE_CFG, T.BASE_B, T.BASE_K, T.BASE_LR, T.BASE_SEED


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
    assert L.SIGNATURES["dgvit_sac_critic_loss"] == (I, [P] * 9 + [F, F] + [P] * 4 + [I, I, P])
    assert L.SIGNATURES["dgvit_sac_actor_loss"] == (I, [P] * 4 + [F, I, F] + [P] * 3 + [I, I, P])
    assert L.SIGNATURES["dgvit_sac_scale_grads"] == (I, [P, P, ctypes.c_longlong, P, P])
    assert dgvit_amd.sac_losses.critic_loss and dgvit_amd.sac_losses.actor_loss and "sac_losses" in dgvit_amd.__all__
    assert dgvit_amd.sac_losses.CriticLoss._fields == ("loss", "td", "target")
    from dgvit_amd import replay
    assert "critic_loss(weights=" in replay.PrioritizedDeviceReplayBuffer.__doc__


def test_abi_version_is_unchanged(lib):
    assert lib.dgvit_abi_version() == 7


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _critic(lib, q1=FAKE, q2=FAKE, reward=FAKE, done=None, weights=None, next_q1=FAKE, next_q2=FAKE, next_log_pi=FAKE, log_alpha=None,
            alpha=0.2, gamma=0.99, target=FAKE, td=None, loss=FAKE, grads=None, B=32, A=2):
    return lib.dgvit_sac_critic_loss(q1, q2, reward, done, weights, next_q1, next_q2, next_log_pi, log_alpha, alpha, gamma, target, td, loss,
                                     grads, B, A, None)


def _actor(lib, log_pi=FAKE, q1_pi=FAKE, q2_pi=FAKE, log_alpha=None, alpha=0.2, with_temperature=0, target_entropy=-2.0, losses=FAKE,
           grads=None, dlog_alpha=None, B=32, A=2):
    return lib.dgvit_sac_actor_loss(log_pi, q1_pi, q2_pi, log_alpha, alpha, with_temperature, target_entropy, losses, grads, dlog_alpha, B, A,
                                    None)


def _scale(lib, src=FAKE, dst=FAKE, n=64, scale=FAKE):
    return lib.dgvit_sac_scale_grads(src, dst, n, scale, None)


BAD = [(_critic, "sac_critic_loss", {k: None}, b"null") for k in ("q1", "q2", "reward", "next_q1", "next_q2", "next_log_pi", "target", "loss")]
BAD += [(_critic, "sac_critic_loss", {k: OFF2}, b"aligned") for k in ("q1", "q2", "reward", "done", "weights", "next_q1", "next_q2", "next_log_pi",
                                                                          "log_alpha", "target", "td", "loss", "grads")]
BAD += [
    (_critic, "sac_critic_loss", dict(B=0), b"B=0"),
    (_critic, "sac_critic_loss", dict(B=-3), b"B=-3"),
    (_critic, "sac_critic_loss", dict(A=0), b"A=0"),
    (_critic, "sac_critic_loss", dict(A=17), b"A=17"),
    (_critic, "sac_critic_loss", dict(B=(1 << 19) + 1, A=2), b"B*A=1048578"),
    (_critic, "sac_critic_loss", dict(B=1 << 30, A=16), b"B*A=17179869184"),
    (_critic, "sac_critic_loss", dict(alpha=float("nan")), b"alpha="),
    (_critic, "sac_critic_loss", dict(alpha=float("inf")), b"alpha=inf"),
    (_critic, "sac_critic_loss", dict(gamma=float("nan")), b"gamma="),
    (_critic, "sac_critic_loss", dict(gamma=float("-inf")), b"gamma=-inf"),
]
BAD += [(_actor, "sac_actor_loss", {k: None}, b"null") for k in ("log_pi", "q1_pi", "q2_pi", "losses")]
BAD += [(_actor, "sac_actor_loss", {k: OFF2}, b"aligned") for k in ("log_pi", "q1_pi", "q2_pi", "log_alpha", "losses", "grads", "dlog_alpha")]
BAD += [
    (_actor, "sac_actor_loss", dict(B=0), b"B=0"),
    (_actor, "sac_actor_loss", dict(A=0), b"A=0"),
    (_actor, "sac_actor_loss", dict(A=17), b"A=17"),
    (_actor, "sac_actor_loss", dict(B=(1 << 20) + 1, A=1), b"B*A=1048577"),
    (_actor, "sac_actor_loss", dict(alpha=float("nan")), b"alpha="),
    (_actor, "sac_actor_loss", dict(with_temperature=2, log_alpha=FAKE), b"with_temperature=2"),
    (_actor, "sac_actor_loss", dict(with_temperature=1), b"needs log_alpha"),
    (_actor, "sac_actor_loss", dict(with_temperature=1, log_alpha=FAKE, target_entropy=float("nan")), b"target_entropy="),
    (_actor, "sac_actor_loss", dict(with_temperature=1, log_alpha=FAKE, target_entropy=float("inf")), b"target_entropy=inf"),
    (_scale, "sac_scale_grads", dict(src=None), b"null"),
    (_scale, "sac_scale_grads", dict(dst=None), b"null"),
    (_scale, "sac_scale_grads", dict(scale=None), b"null"),
    (_scale, "sac_scale_grads", dict(n=0), b"n=0"),
    (_scale, "sac_scale_grads", dict(n=-4), b"n=-4"),
    (_scale, "sac_scale_grads", dict(n=3 * (1 << 20) + 1), b"n=3145729"),
    (_scale, "sac_scale_grads", dict(src=OFF2), b"aligned"),
    (_scale, "sac_scale_grads", dict(dst=OFF2), b"aligned"),
    (_scale, "sac_scale_grads", dict(scale=OFF2), b"aligned"),
]


@pytest.mark.parametrize("call, name, kw, word", BAD, ids=[f"{b[1]}-" + "-".join(f"{k}={v if not isinstance(v, ctypes.c_void_p) else v.value}"
                                                                                  for k, v in b[2].items()) for b in BAD])
def test_bad_arguments_are_refused_before_any_launch(lib, call, name, kw, word):
    assert call(lib, **kw) == -1          # DGVIT_ERR_ARG
    msg = lib.dgvit_last_error()
    assert name.encode() in msg and word in msg, msg


# ------------------------------------------------------------------------------------------------ the Python checks
def _critic_args(Bn=4, A=2):
    return [torch.zeros(Bn, A), torch.zeros(Bn, A), torch.zeros(Bn, 1), torch.zeros(Bn, A), torch.zeros(Bn, A), torch.zeros(Bn, 1)]


def test_exactly_one_temperature():
    from dgvit_amd import sac_losses as S
    la = torch.zeros(1)
    for kw in (dict(), dict(alpha=0.2, log_alpha=la)):
        with pytest.raises(ValueError, match="exactly one of alpha"):
            S.critic_loss(*_critic_args(), **kw)
        with pytest.raises(ValueError, match="exactly one of alpha"):
            S.actor_loss(torch.zeros(4, 1), torch.zeros(4, 2), torch.zeros(4, 2), **kw)
    for bad in (True, "0.2", float("nan"), torch.tensor(0.2)):
        with pytest.raises(ValueError, match="alpha must be a finite float"):
            S.critic_loss(*_critic_args(), alpha=bad)
    with pytest.raises(ValueError, match="log_alpha must be a one-element tensor"):
        S.actor_loss(torch.zeros(4, 1), torch.zeros(4, 2), torch.zeros(4, 2), log_alpha=torch.zeros(2))


def test_target_entropy_needs_log_alpha():
    from dgvit_amd import sac_losses as S
    with pytest.raises(ValueError, match="target_entropy needs log_alpha"):
        S.actor_loss(torch.zeros(4, 1), torch.zeros(4, 2), torch.zeros(4, 2), alpha=0.2, target_entropy=-2.0)
    with pytest.raises(ValueError, match="target_entropy must be a finite float"):
        S.actor_loss(torch.zeros(4, 1), torch.zeros(4, 2), torch.zeros(4, 2), log_alpha=torch.zeros(1), target_entropy=float("nan"))


@pytest.mark.parametrize("pos, name, bad", [(0, "q1", torch.zeros(4)), (0, "q1", torch.zeros(4, 17)), (0, "q1", torch.zeros(0, 2)),
                                            (1, "q2", torch.zeros(4, 3)), (2, "reward", torch.zeros(5, 1)), (2, "reward", torch.zeros(4, 2)),
                                            (3, "next_q1", torch.zeros(5, 2)), (4, "next_q2", torch.zeros(2, 4)),
                                            (5, "next_log_pi", torch.zeros(4, 1, 1))], ids=lambda v: v if isinstance(v, str) else None)
def test_critic_shape_mismatches_name_the_argument(pos, name, bad):
    """CPU tensors would be refused next (DgvitError), so a ValueError shows the shape check ran first"""
    from dgvit_amd import sac_losses as S
    args = _critic_args()
    args[pos] = bad
    with pytest.raises(ValueError, match=f"critic_loss: {name} "):
        S.critic_loss(*args, alpha=0.2)


@pytest.mark.parametrize("kw, name", [(dict(done=torch.zeros(3, 1)), "done"), (dict(weights=torch.zeros(4, 2)), "weights"),
                                      (dict(gamma=None), "gamma"), (dict(gamma=float("inf")), "gamma")], ids=lambda v: v if isinstance(v, str) else None)
def test_critic_keyword_mismatches_name_the_argument(kw, name):
    from dgvit_amd import sac_losses as S
    with pytest.raises(ValueError, match=f"critic_loss: {name} "):
        S.critic_loss(*_critic_args(), alpha=0.2, **kw)


@pytest.mark.parametrize("pos, name, bad", [(0, "log_pi", torch.zeros(5, 1)), (0, "log_pi", torch.zeros(4, 2)), (1, "q1_pi", torch.zeros(8)),
                                            (2, "q2_pi", torch.zeros(4, 1))], ids=lambda v: v if isinstance(v, str) else None)
def test_actor_shape_mismatches_name_the_argument(pos, name, bad):
    from dgvit_amd import sac_losses as S
    args = [torch.zeros(4, 1), torch.zeros(4, 2), torch.zeros(4, 2)]
    args[pos] = bad
    with pytest.raises(ValueError, match=f"actor_loss: {name} "):
        S.actor_loss(*args, alpha=0.2)


def test_there_is_no_cpu_path():
    import dgvit_amd
    from dgvit_amd import sac_losses as S
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):
        S.critic_loss(*_critic_args(), alpha=0.2)
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):
        S.actor_loss(torch.zeros(4), torch.zeros(4, 2), torch.zeros(4, 2), log_alpha=torch.zeros(1), target_entropy=-2.0)
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):
        S.actor_loss(torch.zeros(4, dtype=torch.float64), torch.zeros(4, 2), torch.zeros(4, 2), alpha=0.2)


# ------------------------------------------------------------------------------------------------ the restatement
def _inputs(Bn, A, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32).to(dtype)  # noqa: E731
    return dict(q1=n(Bn, A), q2=n(Bn, A), reward=n(Bn, 1), q1n=n(Bn, A), q2n=n(Bn, A), nlp=n(Bn, 1), lp=n(Bn, 1),
                done=(torch.rand(Bn, 1, generator=g) < 0.25).to(dtype), w=(1 - torch.rand(Bn, 1, generator=g)).to(dtype))


def test_the_restatement_is_the_oracle_in_fp64():
    """float alpha, no mask, no weights: bit for bit"""
    x = _inputs(37, 2, 0)
    with torch.no_grad():
        y = R.target(x["reward"], x["q1n"], x["q2n"], x["nlp"], 0.2, 0.99)
        assert torch.equal(y, x["reward"] + 0.99 * (torch.minimum(x["q1n"], x["q2n"]) - 0.2 * x["nlp"]))     # sac_trajectory_ref.run's line
        assert torch.equal(R.critic_loss(x["q1"], x["q2"], y), O.sac_critic_loss(x["q1"], x["q2"], y))
        assert torch.equal(R.actor_loss(0.2, x["lp"], x["q1"], x["q2"]), O.sac_actor_loss(0.2, x["lp"], x["q1"], x["q2"]))
        assert torch.equal(R.target(x["reward"], x["q1n"], x["q2n"], x["nlp"], 0.2, 0.99, torch.zeros(37, 1, dtype=torch.float64)), y)
        assert torch.equal(R.critic_loss(x["q1"], x["q2"], y, torch.ones(37, dtype=torch.float64)), R.critic_loss(x["q1"], x["q2"], y))
        yd = R.target(x["reward"], x["q1n"], x["q2n"], x["nlp"], 0.2, 0.99, x["done"])
        rows = x["done"][:, 0] == 1
        assert rows.any() and torch.equal(yd[rows], x["reward"][rows].expand(-1, 2)) and torch.equal(yd[~rows], y[~rows])
        assert R.td(x["q1"], y).shape == (37,)


@pytest.mark.parametrize("Bn, A", [(1, 1), (37, 2), (300, 3)])
def test_autograd_of_the_restatement_gives_the_closed_forms(Bn, A):
    x = _inputs(Bn, A, 1)
    n = Bn * A
    q1, q2 = x["q1"].clone().requires_grad_(True), x["q2"].clone().requires_grad_(True)
    la = torch.tensor([-1.3], dtype=torch.float64, requires_grad=True)
    y = R.target(x["reward"], x["q1n"].requires_grad_(True), x["q2n"], x["nlp"], la.exp(), 0.99, x["done"]).detach()
    R.critic_loss(q1, q2, y, x["w"]).backward()
    torch.testing.assert_close(q1.grad, 2 * x["w"] * (x["q1"] - y) / n, rtol=1e-14, atol=0)
    torch.testing.assert_close(q2.grad, 2 * x["w"] * (x["q2"] - y) / n, rtol=1e-14, atol=0)
    assert la.grad is None and x["q1n"].grad is None
    # the actor, with ties: the first element of every row (and whole rows 0 .. 2 where there are that many) tied
    q1p, q2p = x["q1n"].detach().clone(), x["q2n"].detach().clone()
    q2p[:, 0] = q1p[:, 0]
    q2p[:3] = q1p[:3]
    q1p.requires_grad_(True), q2p.requires_grad_(True)
    lp = x["lp"].clone().requires_grad_(True)
    alpha = float(la.detach().exp())
    R.actor_loss(alpha, lp, q1p, q2p).backward()
    torch.testing.assert_close(lp.grad, torch.full_like(lp, alpha / Bn), rtol=1e-14, atol=0)
    lt, tie = q1p.detach() < q2p.detach(), q1p.detach() == q2p.detach()
    assert tie.any()
    for got, smaller in ((q1p.grad, lt), (q2p.grad, ~lt & ~tie)):
        want = torch.zeros(Bn, A, dtype=torch.float64)
        want[smaller], want[tie] = -1.0 / n, -0.5 / n
        assert torch.equal(got, want)
    # the temperature: d log_alpha = -mean(log_pi + target_entropy), nothing into log_pi; the policy loss leaves log_alpha alone
    lp.grad = None
    R.alpha_loss(la, lp, -2.0).backward()
    torch.testing.assert_close(la.grad, -(x["lp"] + -2.0).mean().reshape(1), rtol=1e-14, atol=0)
    assert lp.grad is None and la.grad.shape == (1,)


# ------------------------------------------------------------------------------------------------ the reference learner
@pytest.fixture(scope="module")
def runs():
    """(case, done, fp64 run, fp32 run, yardstick) of the base case with a learned temperature, computed once"""
    case, done = R.make_case(CFG, B, K, SEED), R.make_done(B, K, SEED)
    r64, r32 = R.run(case, torch.float64, done=done), R.run(case, torch.float32, done=done)
    return case, done, r64, r32, R.distance(r32, r64, LR)


def test_the_fp32_run_meets_the_cap_on_its_own(runs):
    case, done, r64, r32, Y = runs
    print(T.report("fp32 against fp64, learned temperature", Y, Y, T.ratios(Y, Y)), "\n  al", Y["al"], "log_alpha", r64["log_alpha"],
          "ulps", R.log_alpha_ulps(r32, r64))
    assert T.cap_violations(Y, K, LR) == []
    assert 0 < Y["qf"] < 1e-5 and 0 < Y["pl"] < 1e-4 and 0 < Y["al"] < 1e-5, "the losses of the fp32 run are within rounding of the fp64 run's"
    assert all(0 < Y[f"{net}.median"] < Y[f"{net}.p999"] < 0.01 for net in T.NETWORKS)
    assert all(0 < float(d.mean()) < 1 for d in done), "every step has finished and unfinished rows"
    # the temperature moves by about alpha_lr per step, and every step's losses use the value of that time
    assert r64["alpha"][0] == pytest.approx(0.2, rel=1e-7) and len(set(r64["alpha"])) == K
    assert all(abs(a - b) > 0.5 * R.ALPHA_LR for a, b in zip([R.LOG_ALPHA0] + r64["log_alpha"], r64["log_alpha"]))
    assert max(R.log_alpha_ulps(r32, r64)) <= K, "the fp32 run's own log_alpha is within K ulps of the fp64 run's"


def test_another_seed_leaves_the_cap():
    """as sac_trajectory_ref's base case: with seed 7 a ReLU unit that flips between the two precisions takes the fp32 run out of the cap,
    which is why the seed is pinned"""
    case, done = R.make_case(CFG, B, K, 7), R.make_done(B, K, 7)
    Y = R.distance(R.run(case, torch.float32, done=done), R.run(case, torch.float64, done=done), LR)
    assert T.cap_violations(Y, K, LR) != []


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_every_defect_breaks_the_rule(runs, defect):
    """the defect's fp64 run stands where the device's result will"""
    case, done, r64, _, Y = runs
    res = R.run(case, torch.float64, done=done, defect=defect)
    r, bad = R.check(R.distance(res, r64, LR), Y, K, LR)
    worst = max(r, key=r.get)
    moved = max(abs(a - b) for a, b in zip(res["log_alpha"], r64["log_alpha"]))
    print(f"{defect}: worst {worst} at {r[worst]:.3g} x the yardstick; log_alpha off by {moved:.3g};", {k: float(f"{v:.3g}") for k, v in r.items()})
    assert bad and r[worst] >= 100 * T.MARGIN
    if defect == "no_alpha_step":
        assert moved > 1e-2 and max(R.log_alpha_ulps(res, r64)) > 1000 * K
    else:
        assert res["log_alpha"] != r64["log_alpha"] and len(set(res["alpha"])) == 1


def test_two_runs_are_bit_equal(runs):
    case, done, r64, _, _ = runs
    again = R.run(case, torch.float64, done=done)
    assert all(again[k] == r64[k] for k in ("qf", "pl", "al", "log_alpha"))
    assert all(torch.equal(again["critic"][k], r64["critic"][k]) for k in r64["critic"])


def test_done_changes_the_trajectory(runs):
    case, _, r64, _, Y = runs
    _, bad = R.check(R.distance(R.run(case, torch.float64, done=None), r64, LR), Y, K, LR)
    assert bad
