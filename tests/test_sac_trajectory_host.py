"""Host: the float64 SAC trajectory reference (tests/sac_trajectory_ref.py) and the rule the GPU cases are judged by, checked on the CPU
alone -- the yardstick (the reference's own fp32 run) meets the cap by itself, every seeded defect breaks the rule by two orders of
magnitude, the reference is deterministic, and the clipping thresholds the GPU test uses do clip at every step.

Base case and seed: sac_trajectory_ref.BASE_*."""
import pytest
import torch

import sac_trajectory_ref as T

CFG, B, K, LR, SEED, KW = T.BASE_CFG, T.BASE_B, T.BASE_K, T.BASE_LR, T.BASE_SEED, T.BASE_KW


@pytest.fixture(scope="module")
def runs():
    """{critic: (case, fp64 run, fp32 run, yardstick)}, each computed once"""
    out = {}
    for critic in ("cnn", "got"):
        case = T.make_case(CFG, B, K, SEED, critic)
        r64, r32 = T.run(case, torch.float64, **KW), T.run(case, torch.float32, **KW)
        out[critic] = (case, r64, r32, T.distance(r32, r64, LR))
    return out


@pytest.mark.parametrize("critic", ["cnn", "got"])
def test_the_fp32_run_meets_the_cap_on_its_own(runs, critic):
    """(a): otherwise a cap taken from the yardstick would hide a failure.  Also what the yardstick is: rounding."""
    case, r64, r32, Y = runs[critic]
    print(T.report(f"fp32 against fp64, {critic} critic", Y, Y, T.ratios(Y, Y)))
    assert T.cap_violations(Y, K, LR) == []
    # (pl is a difference of terms of order 1, alpha logp and q, that leaves a few tenths: its relative error is the larger)
    assert Y["qf"] < 1e-5 and Y["pl"] < 1e-4, "the losses of the fp32 run are within rounding of the fp64 run's"
    assert all(0 < Y[f"{net}.median"] < Y[f"{net}.p999"] < 0.01 for net in T.NETWORKS)
    assert case["steps"][0]["e1"].abs().max() == T.NOISE_CLAMP, "the draws are clamped, and the clamp is reached"
    assert r64["untouched"]["actor"] == sorted(["trans.cls_token", "trans.mlp_head.0.weight", "trans.mlp_head.0.bias",
                                                "trans.mlp_head.1.weight", "trans.mlp_head.1.bias"])
    dead = [k for k in case["critic_params"] if k.startswith(("conv", "trans.cls_token", "trans.mlp_head"))]
    assert r64["untouched"]["critic"] == (sorted(dead) if critic == "got" else [])
    # the trajectory is one: every network has moved, the target less than the critic
    moved = {net: max(float((r64[net][k] - init[k].double()).abs().max()) for k in init)
             for net, init in (("actor", case["actor"]), ("critic", case["critic_params"]), ("target", case["critic_params"]))}
    assert moved["actor"] > 3 * LR and moved["critic"] > 3 * LR and 0 < moved["target"] <= moved["critic"]


@pytest.mark.parametrize("defect", T.DEFECTS)
def test_every_defect_breaks_the_rule_a_hundredfold(runs, defect):
    """(b): the defect's fp64 run stands where the device's result will; its worst quantity is at least 100 margins out"""
    case, r64, _, Y = runs["cnn"]
    d = T.distance(T.run(case, torch.float64, defect=defect, **KW), r64, LR)
    r, bad = T.check(d, Y, K, LR)
    worst = max(r, key=r.get)
    print(f"{defect}: worst {worst} at {r[worst]:.3g} x the yardstick;", {k: float(f"{v:.3g}") for k, v in r.items()})
    assert bad and r[worst] >= 100 * T.MARGIN


def test_two_runs_are_bit_equal(runs):
    """(c)"""
    for dtype, first in ((torch.float64, runs["cnn"][1]), (torch.float32, runs["cnn"][2])):
        again = T.run(runs["cnn"][0], dtype, **KW)
        assert again["qf"] == first["qf"] and again["pl"] == first["pl"]
        for net in T.NETWORKS:
            assert all(torch.equal(again[net][k], first[net][k]) for k in first[net]), net
        assert all(torch.equal(a, b) for a, b in zip(again["td"], first["td"]))


def test_the_clipping_thresholds_clip_at_every_step(runs):
    """(d): half the smallest gradient norm of the unclipped run clips both networks at every step of the clipped one, and the clipped
    trajectory is another one"""
    case, r64, _, Y = runs["cnn"]
    mgn = T.clip_norms(r64)
    assert all(m > 0 for m in mgn)
    clipped = T.run(case, torch.float64, max_grad_norm=mgn, **KW)
    print("max_grad_norm (actor, critic):", mgn, "coefficients:", clipped["coef_actor"], clipped["coef_critic"])
    assert len(clipped["coef_actor"]) == len(clipped["coef_critic"]) == K
    assert all(c < 1 for c in clipped["coef_actor"] + clipped["coef_critic"])
    assert all(c == 1 for c in r64["coef_actor"] + r64["coef_critic"])
    _, bad = T.check(T.distance(clipped, r64, LR), Y, K, LR)
    assert bad, "clipping changes the trajectory"


def test_the_rule_itself():
    """the cap's arithmetic on a hand-made distance, and a margin of its own for one quantity"""
    assert T.max_move(6, 1e-4) == pytest.approx(2 * 6 * 1e-4 * 0.1 / 0.001 ** 0.5)
    Y = {k: 1.0 for k in T.MEASURED}
    d = dict(Y, **{f"{net}.{q}": v for net in T.NETWORKS for q, v in (("frac", 0.0), ("max", 0.0), ("numel", 10))})
    assert T.check(d, Y, 6, 1e-4) == ({k: 1.0 for k in T.MEASURED}, [])
    d["qf"] = 4.5
    assert len(T.check(d, Y, 6, 1e-4)[1]) == 1 and T.check(d, Y, 6, 1e-4, margins={"qf": 9.0})[1] == []
    d["critic.frac"], d["target.max"] = 1.1e-4, 1.01 * T.max_move(6, 1e-4)
    assert len(T.check(d, Y, 6, 1e-4, margins={"qf": 9.0})[1]) == 2
    d["pl"] = float("nan")
    assert len(T.check(d, Y, 6, 1e-4, margins={"qf": 9.0})[1]) == 3, "a NaN fails"
