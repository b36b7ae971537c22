"""A functional SAC learner over parameter dicts, on the CPU, in a chosen dtype: the independent reference that several learn() steps of
the HIP networks are followed against (test_sac_trajectory_host.py, test_gpu_sac_trajectory.py), and the rule by which they are compared.

The arithmetic is the oracle's (oracle/dgvit_oracle.py: policy_sample, cnn_qnet_forward / qnet_forward, sac_critic_loss, sac_actor_loss,
soft_update) with torch.optim.Adam and torch.nn.utils.clip_grad_norm_; the step order is that of bench.py's small_batch.learn():

  1. no-grad target  y = r + gamma (min(q1n, q2n) - alpha logp_next), the next action sampled with the draw e1
  2. critic loss on (obs, pobs, act), critic Adam step
  3. actor sample with the draw e2, critic forward on pi
  4. both gradient sets dropped, backward of the actor loss, actor Adam step (the critic's gradients of this backward are never applied)
  5. target <- target (1 - tau) + critic tau

Everything random is an input (``make_case``): per step the frames, pstate, actions, rewards and the two N(0, 1) draws, the draws clamped
to [-1.5, 1.5] -- unclamped, log(1 - tanh^2 + 1e-6) is ill-conditioned in fp32 and the reference's own fp32 run moves y by 7e-4 at step 0.
All inputs and initial parameters are fp32 values, so a float64 run and the fp32 device consume the same numbers.

The rule (``distance`` / ``check``): a run is measured by its distance from the float64 run, and judged against the distance Y of the
float32 run of this same learner -- the yardstick, nothing of it comes from the code under test:

  * losses: the largest relative difference over the steps, qf and pl separately, against ``margin`` x Y's largest (not the same step's:
    one step's fp32 error can be near zero by luck);
  * parameters, per network (actor, critic, target): median and 99.9th percentile of |delta| / lr against ``margin`` x the same quantile of Y;
  * the cap, a condition and not a measurement: at most 1e-4 of a network's elements differ by more than 0.1 lr, and none by more than
    2 K lr (1 - beta1) / sqrt(1 - beta2), twice the farthest Adam can move a weight in K steps.

MARGIN = 4: the project grants 2x where the same arithmetic runs in another summation order (the last-block fold's "within twice the
unfolded error"); the device's exp, tanh and log also differ from libm by a further ulp or so, and both effects feed every Adam step.
"""
import math

import numpy as np
import torch

from helpers import O
import prioritized_replay_ref as R
import replay_shift_ref as S

DEFECTS = ("skip_soft", "stale_grad", "same_noise", "frozen_step")
NOISE_CLAMP = 1.5
BETA1, BETA2 = 0.9, 0.999          # torch.optim.Adam's and FlatAdam's defaults
MARGIN = 4.0
CAP_FRACTION, CAP_STEP = 1e-4, 0.1
NETWORKS = ("actor", "critic", "target")

# The base case of both test files: 84 x 84 frames in 12 x 12 patches, dim 64, depth 2, heads 2 (50 tokens); B = 37 spans two 32-row blocks
# of the head kernels; tau 0.25, not the shipped 0.005, at which a missed target update moves nothing measurable in six steps.
# BASE_SEED was chosen on the CPU, as replay_shift_ref.SEED was: with it the reference's own fp32 run stays at rounding distance from its
# fp64 run and meets the cap (test_sac_trajectory_host.py); with other seeds (1, 7, 2024) a ReLU unit that flips between the two
# precisions puts up to 2e-3 of the CNN critic's elements more than 0.1 lr away after the first Adam step.
BASE_CFG = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2)
BASE_B, BASE_K, BASE_LR, BASE_SEED = 37, 6, 1e-4, 61
BASE_KW = dict(lr=BASE_LR, alpha=0.2, gamma=0.99, tau=0.25)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def critic_spec(cfg, critic):
    if critic not in ("cnn", "got"):
        raise ValueError(critic)
    return O.cnn_qnet_param_spec() if critic == "cnn" else O.qnet_param_spec(cfg)


def make_case(cfg, batch, steps, seed, critic="cnn"):
    """Initial parameters (actor: seed, critic and target: seed + 1) and the inputs of every step, all fp32 tensors.  ``steps[k]`` holds
    obs, pobs, act, rew, next_obs, next_pobs and the clamped draws e1 (next action) and e2 (actor sample)."""
    rs = np.random.RandomState(seed + 7)
    per_step = []
    for k in range(steps):
        obs, pobs, act, _ = O.make_inputs(cfg, batch, seed + 10 * k + 1)
        nobs, npobs, _, _ = O.make_inputs(cfg, batch, seed + 10 * k + 2)
        per_step.append(dict(obs=obs, pobs=pobs, act=act, next_obs=nobs, next_pobs=npobs, rew=_t(rs.standard_normal((batch, 1))),
                             e1=_t(np.clip(rs.standard_normal((batch, 2)), -NOISE_CLAMP, NOISE_CLAMP)),
                             e2=_t(np.clip(rs.standard_normal((batch, 2)), -NOISE_CLAMP, NOISE_CLAMP))))
    return dict(cfg=cfg, critic=critic, batch=batch, actor=O.make_params(O.policy_param_spec(cfg), seed),
                critic_params=O.make_params(critic_spec(cfg, critic), seed + 1), steps=per_step)


def make_store(cfg, n, seed):
    """n transitions for a replay buffer (fp32 tensors, first axis = transitions), field names as replay.DeviceReplayBuffer's"""
    obs, pobs, act, _ = O.make_inputs(cfg, n, seed + 1)
    nobs, npobs, _, _ = O.make_inputs(cfg, n, seed + 2)
    rs = np.random.RandomState(seed + 3)
    return dict(obs=obs, pobs=pobs, act=act, rew=_t(rs.standard_normal((n, 1))), next_obs=nobs, next_pobs=npobs, done=torch.zeros(n, 1))


def _leafs(params, dtype):
    return {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in params.items()}


def _drop_grads(p):
    for v in p.values():
        v.grad = None


def _grad_norm(p):
    return math.sqrt(sum(float(v.grad.double().pow(2).sum()) for v in p.values() if v.grad is not None))


def _adam_step(opt, p, max_norm, frozen):
    """(gradient norm before clipping, clip coefficient): clip_grad_norm_ when asked, then the step.  ``frozen``: the bias correction sees
    step 1 every time, which is what a step counter frozen into a captured graph would do."""
    norm = _grad_norm(p)
    coef = 1.0
    if max_norm is not None:
        total = torch.nn.utils.clip_grad_norm_([v for v in p.values() if v.grad is not None], max_norm)
        coef = min(max_norm / (float(total) + 1e-6), 1.0)
    if frozen:
        for st in opt.state.values():
            st["step"].zero_()
    opt.step()
    return norm, coef


def run(case, dtype, lr=1e-4, alpha=0.2, gamma=0.99, tau=0.25, max_grad_norm=None, defect=None, per=None):
    """K = len(case["steps"]) learn() steps in ``dtype``.  ``max_grad_norm``: None or (actor's, critic's).  ``defect``: one of DEFECTS.

    ``per``: the prioritized, shifted loop, teacher-forced -- a dict with ``store`` (make_store), ``priorities`` (the initial priority of
    every stored transition), ``alpha``, ``eps``, ``beta``, ``pad`` and per step ``idx`` (B,), ``obs_shift`` and ``next_obs_shift`` (B, 2)
    as the device drew them.  The batch of step k is then the stored transitions at idx[k] with replay_shift_ref.ref_shift applied to this
    learner's own copy of the frames; the leaves are its own, float64 (prioritized_replay_ref.leaves / weights; a repeated index keeps the
    largest new value); the critic loss is (w (q - y)^2).mean() summed over the twins and |q1 - y|.mean(1) is written back.

    Returns per-step lists qf, pl, td (|q1 - y|, (B, A)), gnorm / coef of both optimisers, the final ``actor``, ``critic``, ``target``
    dicts, ``untouched`` (the keys of actor and critic that never received a gradient) and, with ``per``, ``weights`` and ``leaves``."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    cfg, kind = case["cfg"], case["critic"]
    A, C = _leafs(case["actor"], dtype), _leafs(case["critic_params"], dtype)
    T = {k: v.detach().clone() for k, v in C.items()}
    opt_a = torch.optim.Adam(list(A.values()), lr=lr, betas=(BETA1, BETA2))
    opt_c = torch.optim.Adam(list(C.values()), lr=lr, betas=(BETA1, BETA2))
    mgn_a, mgn_c = (None, None) if max_grad_norm is None else max_grad_norm
    frozen = defect == "frozen_step"

    def q(p, img, pst, a):
        return O.cnn_qnet_forward(p, img, pst, a) if kind == "cnn" else O.qnet_forward(p, img, pst, a, cfg)

    out = dict(qf=[], pl=[], td=[], gnorm_actor=[], gnorm_critic=[], coef_actor=[], coef_critic=[], weights=[], leaves=[])
    touched_a, touched_c = set(), set()
    if per is not None:
        eps = np.float64(np.float32(per["eps"]))
        leaf = R.leaves(np.asarray(per["priorities"], dtype=np.float32), per["alpha"], eps)
        store = {k: v.to(dtype) for k, v in per["store"].items()}
    for k, s in enumerate(case["steps"]):
        w = None
        if per is not None:
            idx = np.asarray(per["idx"][k], dtype=np.int64)
            ti = torch.from_numpy(idx)
            b = {f: store[f][ti] for f in ("pobs", "act", "rew", "next_pobs")}
            b["obs"] = S.ref_shift(store["obs"][ti], torch.as_tensor(per["obs_shift"][k]), per["pad"])
            b["next_obs"] = S.ref_shift(store["next_obs"][ti], torch.as_tensor(per["next_obs_shift"][k]), per["pad"])
            wk = R.weights(leaf, idx, per["beta"])
            out["weights"].append(wk.copy())
            w = torch.from_numpy(wk).to(dtype)[:, None]
        else:
            b = {f: s[f].to(dtype) for f in ("obs", "pobs", "act", "rew", "next_obs", "next_pobs")}
        e1 = s["e1"].to(dtype)
        e2 = e1 if defect == "same_noise" else s["e2"].to(dtype)
        zero_critic = not (defect == "stale_grad" and k > 0)
        # 1. target
        with torch.no_grad():
            na, nlogp, _ = O.policy_sample(A, b["next_obs"], b["next_pobs"], cfg, e1)
            q1n, q2n = q(T, b["next_obs"], b["next_pobs"], na)
            y = b["rew"] + gamma * (torch.minimum(q1n, q2n) - alpha * nlogp)
        # 2. critic
        q1, q2 = q(C, b["obs"], b["pobs"], b["act"])
        if w is None:
            qf = O.sac_critic_loss(q1, q2, y)
        else:
            qf = (w * (q1 - y) ** 2).mean() + (w * (q2 - y) ** 2).mean()
        td = (q1 - y).abs().detach()
        if zero_critic:
            _drop_grads(C)
        qf.backward()
        touched_c |= {n for n, v in C.items() if v.grad is not None}
        norm, coef = _adam_step(opt_c, C, mgn_c, frozen)
        out["gnorm_critic"].append(norm), out["coef_critic"].append(coef)
        # 3. actor sample, critic on pi
        pi, logp, _ = O.policy_sample(A, b["obs"], b["pobs"], cfg, e2)
        q1p, q2p = q(C, b["obs"], b["pobs"], pi)
        pl = O.sac_actor_loss(alpha, logp, q1p, q2p)
        # 4. actor
        _drop_grads(A)
        if zero_critic:
            _drop_grads(C)
        pl.backward()
        touched_a |= {n for n, v in A.items() if v.grad is not None}
        norm, coef = _adam_step(opt_a, A, mgn_a, frozen)
        out["gnorm_actor"].append(norm), out["coef_actor"].append(coef)
        # 5. target
        if not (defect == "skip_soft" and k == 3):
            with torch.no_grad():
                O.soft_update(T, C, tau)
        out["qf"].append(float(qf.detach())), out["pl"].append(float(pl.detach())), out["td"].append(td)
        if per is not None:
            new = R.leaves(td.mean(1).double().numpy(), per["alpha"], eps)
            for i in np.unique(idx):
                leaf[i] = new[idx == i].max()
            out["leaves"].append(leaf.copy())
    out["actor"] = {n: v.detach() for n, v in A.items()}
    out["critic"] = {n: v.detach() for n, v in C.items()}
    out["target"] = T
    out["untouched"] = dict(actor=sorted(set(A) - touched_a), critic=sorted(set(C) - touched_c))
    for net, init in (("actor", case["actor"]), ("critic", case["critic_params"])):
        for n in out["untouched"][net]:
            assert torch.equal(out[net][n], init[n].to(dtype)), n
    return out


def td_yardstick(res32, res64):
    """the largest difference of a written-back priority |q1 - y|.mean(1) between the fp32 and the fp64 run"""
    return max(float((a.double().mean(1) - b.mean(1)).abs().max()) for a, b in zip(res32["td"], res64["td"]))


def leaf_widening(per, res, slack):
    """Per step, for every stored slot: how far its leaf (|p| + eps)^alpha moves when the priority p last written to it moves by
    ``slack`` -- slack alpha (p + eps)^(alpha - 1), 0 for a slot that still holds its initial priority."""
    eps, alpha = float(np.float32(per["eps"])), per["alpha"]
    wide, out = np.zeros(len(per["priorities"])), []
    for k, td in enumerate(res["td"]):
        idx, p = np.asarray(per["idx"][k], dtype=np.int64), td.double().mean(1).numpy()
        for i in np.unique(idx):
            wide[i] = slack * alpha * (p[idx == i].max() + eps) ** (alpha - 1.0)
        out.append(wide.copy())
    return out


def clip_norms(res):
    """(actor's, critic's) max_grad_norm that clips at every step: half the smallest per-step gradient norm of an unclipped run"""
    return 0.5 * min(res["gnorm_actor"]), 0.5 * min(res["gnorm_critic"])


def max_move(steps, lr):
    """twice the farthest Adam can move a weight in ``steps`` steps: each update is at most lr (1 - beta1) / sqrt(1 - beta2)"""
    return 2.0 * steps * lr * (1.0 - BETA1) / math.sqrt(1.0 - BETA2)


def distance(res, ref, lr):
    """The distance of the run ``res`` from ``ref`` (its float64 twin): {"qf", "pl"}: largest relative loss difference over the steps;
    per network its "<net>.median" and "<net>.p999" of |delta| / lr, and for the cap "<net>.frac" (share of elements beyond 0.1 lr) and
    "<net>.max" (largest |delta|).  ``res``'s parameters may be any float tensors on the CPU."""
    d = {}
    for name in ("qf", "pl"):
        a, b = np.asarray(res[name], dtype=np.float64), np.asarray(ref[name], dtype=np.float64)
        d[name] = float(np.max(np.abs(a - b) / np.abs(b)))
    for net in NETWORKS:
        assert set(res[net]) == set(ref[net]), net
        delta = np.concatenate([(res[net][n].detach().double().cpu() - ref[net][n].double()).abs().reshape(-1).numpy() for n in ref[net]])
        d[net + ".median"] = float(np.median(delta)) / lr
        d[net + ".p999"] = float(np.quantile(delta, 0.999)) / lr
        d[net + ".frac"] = float(np.mean(delta > CAP_STEP * lr))
        d[net + ".max"] = float(delta.max())
        d[net + ".numel"] = int(delta.size)
    return d


MEASURED = ("qf", "pl") + tuple(f"{net}.{q}" for net in NETWORKS for q in ("median", "p999"))


def cap_violations(d, steps, lr):
    """the cap of the rule on a ``distance``: a list of what breaks it (empty: holds)"""
    bad = []
    for net in NETWORKS:
        if d[net + ".frac"] > CAP_FRACTION:
            bad.append(f"{net}: {d[net + '.frac']:.3g} of the elements differ by more than {CAP_STEP} lr (cap {CAP_FRACTION})")
        if d[net + ".max"] > max_move(steps, lr):
            bad.append(f"{net}: an element differs by {d[net + '.max']:.3g} > {max_move(steps, lr):.3g}")
    return bad


def ratios(d, yardstick):
    """distance / yardstick for every measured quantity (inf where the yardstick is 0 and the distance is not)"""
    return {k: (d[k] / yardstick[k] if yardstick[k] > 0 else (0.0 if d[k] == 0 else math.inf)) for k in MEASURED}


def check(d, yardstick, steps, lr, margin=MARGIN, margins=None):
    """(ratios, failures) of the whole rule; ``margins``: {quantity: margin} for quantities with a documented margin of their own"""
    r = ratios(d, yardstick)
    bad = [f"{k}: {d[k]:.3g} is {r[k]:.3g} x the yardstick {yardstick[k]:.3g} (margin {(margins or {}).get(k, margin)})"
           for k in MEASURED if not r[k] <= (margins or {}).get(k, margin)]
    return r, bad + cap_violations(d, steps, lr)


def report(title, d, yardstick, r):
    lines = [f"{title}: quantity  hip  yardstick  hip/yardstick"]
    lines += [f"  {k:14s} {d[k]:.3e}  {yardstick[k]:.3e}  {r[k]:.2f}" for k in MEASURED]
    lines += [f"  {net}: {d[net + '.frac'] * d[net + '.numel']:.0f} of {d[net + '.numel']} elements beyond {CAP_STEP} lr, largest |delta| "
              f"{d[net + '.max']:.3e}" for net in NETWORKS]
    return "\n".join(lines)
