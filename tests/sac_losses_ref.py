"""The SAC loss head (dgvit_amd.sac_losses) restated as torch functions in any dtype on the CPU -- autograd gives their
gradients -- and a reference learner with a learned temperature that the device's learn() steps are followed against.

Formulas (q*: (B, A); reward, done, weights, log_pi, next_log_pi: (B, 1) or (B,); alpha a float or a 0-d / (1,) tensor):

    target      y = reward + (1 - done) gamma (min(q1n, q2n) - alpha next_log_pi)            done None: 0
    critic      mean(w (q1 - y)^2) + mean(w (q2 - y)^2),   td = |q1 - y|.mean(1)             w None: 1
    actor       mean(alpha log_pi - min(q1pi, q2pi))
    temperature -log_alpha mean(log_pi + target_entropy)                                     log_pi a constant

``run`` is sac_trajectory_ref.run's loop (same helpers, same ``make_case``, same step order) with ``done`` in the target and, after the
actor step and before the Polyak update, the temperature step: Adam on ``log_alpha`` with the actor sample's log_pi, detached; alpha is
exp(log_alpha) at the time of each use.  log_alpha starts at the fp32 value of log 0.2, so a float64 run and the fp32 device consume the
same number.  The form of the temperature step is the standard one (log_alpha = zeros(1), Adam([log_alpha]), target_entropy = -|A|,
DRL.py:417-425 by SURVEY 3(A)); the reference's source is not at hand, so it is unpinned.

The rule is sac_trajectory_ref's (``distance`` / ``check`` here add the temperature loss "al" as one more loss quantity under it).
"""
import math

import numpy as np
import torch

from helpers import O
import sac_trajectory_ref as T
from sac_trajectory_ref import make_case  # noqa: F401  (the cases are sac_trajectory_ref's)

DEFECTS = ("stale_alpha", "no_alpha_step")
LOG_ALPHA0 = float(np.float32(math.log(0.2)))
TARGET_ENTROPY, ALPHA_LR, DONE_P = -2.0, 1e-2, 0.25


def _col(t, like):
    """a (B,) or (B, 1) tensor as (B, 1), to broadcast over the A columns of ``like``"""
    return t.reshape(like.shape[0], 1)


def target(reward, next_q1, next_q2, next_log_pi, alpha, gamma, done=None):
    y = torch.minimum(next_q1, next_q2) - alpha * _col(next_log_pi, next_q1)
    if done is not None:
        y = (1 - _col(done, next_q1)) * gamma * y
    else:
        y = gamma * y
    return _col(reward, next_q1) + y


def critic_loss(q1, q2, y, weights=None):
    if weights is None:
        return ((q1 - y) ** 2).mean() + ((q2 - y) ** 2).mean()
    w = _col(weights, q1)
    return (w * (q1 - y) ** 2).mean() + (w * (q2 - y) ** 2).mean()


def td(q1, y):
    return (q1 - y).abs().mean(1).detach()


def actor_loss(alpha, log_pi, q1_pi, q2_pi):
    return (alpha * _col(log_pi, q1_pi) - torch.minimum(q1_pi, q2_pi)).mean()


def alpha_loss(log_alpha, log_pi, target_entropy):
    return (-log_alpha * (log_pi.detach() + target_entropy).mean()).reshape(())


def make_done(batch, steps, seed):
    """per step a (B, 1) fp32 tensor of Bernoulli(0.25) draws"""
    rs = np.random.RandomState(seed + 11)
    return [torch.from_numpy((rs.random_sample((batch, 1)) < DONE_P).astype(np.float32)) for _ in range(steps)]


def run(case, dtype, alpha_lr=ALPHA_LR, done=None, defect=None, lr=1e-4, gamma=0.99, tau=0.25, target_entropy=TARGET_ENTROPY):
    """K = len(case["steps"]) learn() steps in ``dtype`` with a learned temperature.  ``done``: None or make_done's list.  ``defect``:
    "stale_alpha" (the losses keep step 0's alpha although log_alpha moves) or "no_alpha_step" (log_alpha never moves).

    Returns per-step lists qf, pl, al, td ((B,)), y ((B, A)), log_alpha (after the step) and alpha (the one the step's losses used), and
    the final ``actor``, ``critic``, ``target`` dicts."""
    if defect is not None and defect not in DEFECTS:
        raise ValueError(defect)
    cfg, kind = case["cfg"], case["critic"]
    A, C = T._leafs(case["actor"], dtype), T._leafs(case["critic_params"], dtype)
    Tg = {k: v.detach().clone() for k, v in C.items()}
    log_alpha = torch.tensor([LOG_ALPHA0], dtype=dtype, requires_grad=True)
    opt_a = torch.optim.Adam(list(A.values()), lr=lr, betas=(T.BETA1, T.BETA2))
    opt_c = torch.optim.Adam(list(C.values()), lr=lr, betas=(T.BETA1, T.BETA2))
    opt_t = torch.optim.Adam([log_alpha], lr=alpha_lr, betas=(T.BETA1, T.BETA2))
    alpha0 = log_alpha.detach().exp().clone()

    def q(p, img, pst, a):
        return O.cnn_qnet_forward(p, img, pst, a) if kind == "cnn" else O.qnet_forward(p, img, pst, a, cfg)

    def alpha_now():
        return alpha0 if defect == "stale_alpha" else log_alpha.detach().exp()

    out = dict(qf=[], pl=[], al=[], td=[], y=[], log_alpha=[], alpha=[])
    for k, s in enumerate(case["steps"]):
        b = {f: s[f].to(dtype) for f in ("obs", "pobs", "act", "rew", "next_obs", "next_pobs")}
        e1, e2 = s["e1"].to(dtype), s["e2"].to(dtype)
        dk = None if done is None else done[k].to(dtype)
        out["alpha"].append(float(alpha_now()))
        # 1. target
        with torch.no_grad():
            na, nlogp, _ = O.policy_sample(A, b["next_obs"], b["next_pobs"], cfg, e1)
            q1n, q2n = q(Tg, b["next_obs"], b["next_pobs"], na)
            y = target(b["rew"], q1n, q2n, nlogp, alpha_now(), gamma, dk)
        # 2. critic
        q1, q2 = q(C, b["obs"], b["pobs"], b["act"])
        qf = critic_loss(q1, q2, y)
        T._drop_grads(C)
        qf.backward()
        T._adam_step(opt_c, C, None, False)
        # 3. actor sample, critic on pi; 4. actor
        pi, logp, _ = O.policy_sample(A, b["obs"], b["pobs"], cfg, e2)
        q1p, q2p = q(C, b["obs"], b["pobs"], pi)
        pl = actor_loss(alpha_now(), logp, q1p, q2p)
        T._drop_grads(A)
        T._drop_grads(C)
        pl.backward()
        T._adam_step(opt_a, A, None, False)
        # 5. temperature, with the actor sample's log_pi
        al = alpha_loss(log_alpha, logp, target_entropy)
        log_alpha.grad = None
        al.backward()
        if defect != "no_alpha_step":
            opt_t.step()
        # 6. target network
        with torch.no_grad():
            O.soft_update(Tg, C, tau)
        out["qf"].append(float(qf.detach())), out["pl"].append(float(pl.detach())), out["al"].append(float(al.detach()))
        out["td"].append(td(q1.detach(), y)), out["y"].append(y.clone()), out["log_alpha"].append(float(log_alpha.detach().double()))
    out["actor"] = {n: v.detach() for n, v in A.items()}
    out["critic"] = {n: v.detach() for n, v in C.items()}
    out["target"] = Tg
    return out


def distance(res, ref, lr):
    """sac_trajectory_ref.distance and "al": the largest relative difference of the temperature loss over the steps"""
    d = T.distance(res, ref, lr)
    a, b = np.asarray(res["al"], dtype=np.float64), np.asarray(ref["al"], dtype=np.float64)
    d["al"] = float(np.max(np.abs(a - b) / np.abs(b)))
    return d


def check(d, yardstick, steps, lr, margin=T.MARGIN):
    """(ratios, failures): sac_trajectory_ref.check, and "al" judged as qf and pl are"""
    r, bad = T.check(d, yardstick, steps, lr, margin=margin)
    r["al"] = d["al"] / yardstick["al"] if yardstick["al"] > 0 else (0.0 if d["al"] == 0 else math.inf)
    if not r["al"] <= margin:
        bad.insert(0, f"al: {d['al']:.3g} is {r['al']:.3g} x the yardstick {yardstick['al']:.3g} (margin {margin})")
    return r, bad


def log_alpha_ulps(res, ref):
    """per step: |log_alpha - the fp64 run's| in units of 2^-23 of the fp64 value's magnitude"""
    return [abs(a - b) / (2.0 ** -23 * abs(b)) for a, b in zip(res["log_alpha"], ref["log_alpha"])]
