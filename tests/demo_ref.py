"""Host restatement of the learning-from-demonstrations pieces in plain torch, in whatever dtype its inputs have: the
log-density of a given action under the tanh-Gaussian policies (functional.tanh_gaussian_log_prob, GoTPolicy.log_prob) and the two
demonstration losses (sac_losses.bc_loss, sac_losses.nll_loss).  Evaluated in float64 it is the reference of tests/test_gpu_demo.py; the
same functions in float32 are that file's yardstick.  Nothing here imports the package under test.

tests/test_demo_host.py pins ``log_prob`` against torch.distributions on the CPU."""
import math

import torch

LOG_SIG_MIN, LOG_SIG_MAX = -20.0, 2.0
EPSILON = 1e-6
CLIP = 1.0 - 1e-6
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def squash_inverse(action, scale, bias):
    """y, the action on the tanh's scale, clipped so that atanh stays finite"""
    return ((action - bias) / scale).clamp(-CLIP, CLIP)


def log_prob(mean, log_std_raw, action, scale, bias, ls_min=LOG_SIG_MIN, ls_max=LOG_SIG_MAX):
    """(B, 1): sum_a [ -e^2 / 2 - ls - log sqrt(2 pi) - log(scale (1 - y^2) + 1e-6) ], e = (atanh(y) - mean) exp(-ls)"""
    y = squash_inverse(action, scale, bias)
    x = 0.5 * torch.log((1 + y) / (1 - y))
    ls = torch.clamp(log_std_raw, min=ls_min, max=ls_max)
    e = (x - mean) * torch.exp(-ls)
    return (-0.5 * e * e - ls - HALF_LOG_2PI - torch.log(scale * (1 - y * y) + EPSILON)).sum(1, keepdim=True)


def row_weights(B, like, mask=None, q_demo=None, q_pi=None):
    """m_b f_b, (B,): the mask as numbers (None = 1) times the Q-filter's strict decision (None = 1)"""
    w = torch.ones(B, dtype=like.dtype) if mask is None else mask.reshape(B).to(like.dtype)
    if q_demo is not None:
        demo, pi = torch.minimum(*q_demo).mean(1), torch.minimum(*q_pi).mean(1)
        w = w * (demo > pi).to(like.dtype)
    return w


def masked_mean(rows, w):
    """(sum_b w_b l_b / used or 0, used)"""
    used = w.sum()
    if float(used) > 0:
        return (w * rows).sum() / used, used
    return (rows * 0).sum(), used


def bc_loss(pred, action, mask=None, q_demo=None, q_pi=None):
    return masked_mean(((pred - action) ** 2).mean(1), row_weights(pred.shape[0], pred, mask, q_demo, q_pi))


def nll_loss(logp, mask=None):
    return masked_mean(-logp.reshape(-1), row_weights(logp.shape[0], logp, mask))


# ------------------------------------------------------------------------------------------------ a demonstration-regularised learner
# sac_trajectory_ref.run's plain loop with two changes: each step's batch is gathered from two stores (the agent's rows first, then the
# demonstrations') at injected indices, as replay.sample_mixed does, and the actor loss gains LAMBDA x the behaviour-cloning term over
# the demonstration rows.  Configuration, optimiser, step order, distance and check are sac_trajectory_ref's, by import.
LAMBDA = 0.5
DEMO_COUNTS, DEMO_STEPS, DEMO_SLOTS = (6, 2), 4, (16, 8)
FIELDS = ("obs", "pobs", "act", "rew", "next_obs", "next_pobs")


def make_demo_case(seed=None):
    """(case, stores, idx): sac_trajectory_ref.make_case at its base configuration with B = 6 + 2 and 4 steps (parameters and the two
    draws per step), a store of 16 agent and one of 8 demonstration transitions (make_store), and per step the slots drawn from each"""
    import sac_trajectory_ref as T
    seed = T.BASE_SEED if seed is None else seed
    case = T.make_case(T.BASE_CFG, sum(DEMO_COUNTS), DEMO_STEPS, seed)
    stores = [T.make_store(T.BASE_CFG, n, seed + 100 * (i + 1)) for i, n in enumerate(DEMO_SLOTS)]
    g = torch.Generator().manual_seed(seed)
    idx = [[torch.randint(0, slots, (n,), generator=g) for n, slots in zip(DEMO_COUNTS, DEMO_SLOTS)] for _ in range(DEMO_STEPS)]
    return case, stores, idx


def run_demo(case, stores, idx, dtype, lam=LAMBDA, lr=1e-4, alpha=0.2, gamma=0.99, tau=0.25):
    """the steps in ``dtype`` -> what sac_trajectory_ref.run returns of qf, pl (the whole actor loss), td, bc, used, actor, critic, target"""
    import sac_trajectory_ref as T
    from helpers import O
    cfg = case["cfg"]
    A, C = T._leafs(case["actor"], dtype), T._leafs(case["critic_params"], dtype)
    Tg = {k: v.detach().clone() for k, v in C.items()}
    opt_a = torch.optim.Adam(list(A.values()), lr=lr, betas=(T.BETA1, T.BETA2))
    opt_c = torch.optim.Adam(list(C.values()), lr=lr, betas=(T.BETA1, T.BETA2))
    held = [{k: v.to(dtype) for k, v in s.items()} for s in stores]
    source = torch.cat([torch.full((n,), i) for i, n in enumerate(DEMO_COUNTS)])
    out = dict(qf=[], pl=[], td=[], bc=[], used=[])
    for k, s in enumerate(case["steps"]):
        b = {f: torch.cat([h[f][i] for h, i in zip(held, idx[k])]) for f in FIELDS}
        e1, e2 = s["e1"].to(dtype), s["e2"].to(dtype)
        with torch.no_grad():
            na, nlogp, _ = O.policy_sample(A, b["next_obs"], b["next_pobs"], cfg, e1)
            q1n, q2n = O.cnn_qnet_forward(Tg, b["next_obs"], b["next_pobs"], na)
            y = b["rew"] + gamma * (torch.minimum(q1n, q2n) - alpha * nlogp)
        q1, q2 = O.cnn_qnet_forward(C, b["obs"], b["pobs"], b["act"])
        qf = O.sac_critic_loss(q1, q2, y)
        T._drop_grads(C)
        qf.backward()
        T._adam_step(opt_c, C, None, False)
        pi, logp, _ = O.policy_sample(A, b["obs"], b["pobs"], cfg, e2)
        q1p, q2p = O.cnn_qnet_forward(C, b["obs"], b["pobs"], pi)
        bc, used = bc_loss(pi, b["act"], source == 1)
        pl = O.sac_actor_loss(alpha, logp, q1p, q2p) + lam * bc
        T._drop_grads(A), T._drop_grads(C)
        pl.backward()
        T._adam_step(opt_a, A, None, False)
        with torch.no_grad():
            O.soft_update(Tg, C, tau)
        out["qf"].append(float(qf.detach())), out["pl"].append(float(pl.detach())), out["td"].append((q1 - y).abs().detach())
        out["bc"].append(float(bc.detach())), out["used"].append(float(used))
    out["actor"], out["critic"], out["target"] = {n: v.detach() for n, v in A.items()}, {n: v.detach() for n, v in C.items()}, Tg
    return out
