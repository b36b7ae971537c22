"""The SAC loss head on the device (include/dgvit_hip.h: The SAC loss head): the arithmetic of SAC.learn between the network
forwards and the backwards (DRL.py:384-425) -- the target, the twin-critic loss with ``done`` and importance weights, the |q1 - y| a
prioritized replay takes back, the actor loss and the temperature loss -- as one HIP launch per loss forward and one per backward.

    out = critic_loss(q1, q2, batch["rew"], q1n, q2n, next_log_pi, log_alpha=log_alpha, done=batch["done"], weights=batch["weights"])
    out.loss.backward(); critic_opt.step(); buf.update_priorities(batch["indexes"], out.td)
    policy_loss, alpha_loss = actor_loss(log_pi, q1_pi, q2_pi, log_alpha=log_alpha, target_entropy=-2.0)
    policy_loss.backward(); actor_opt.step()
    alpha_loss.backward(); alpha_opt.step()          # FlatAdam([log_alpha]); log_alpha.grad is a (1,) fp32 tensor

Learning from demonstrations: ``bc_loss`` and ``nll_loss`` are the demonstration term of the actor loss over the rows of a
``replay.sample_mixed`` batch that came from the demonstration ring, normalised on the device by how many rows that is:

    bc = bc_loss(pi, batch["act"], mask=batch["source"] == 1)            # BCLoss(loss, used)
    (policy_loss + lam * bc.loss).backward()

Conservative Q-learning: ``cql_penalty`` is the CQL(H) term of a critic loss over the Q-values of M proposal actions per
state, ``q_many`` of the critics on ``sample_many`` draws and uniform actions:

    cql = cql_penalty(q1_cat, q2_cat, q1, q2, log_w=log_w, weight=5.0)             # CQLLoss(loss, weight_loss, gap, used)
    (out.loss + cql.loss).backward()

The temperature is either the float ``alpha=`` or ``exp(log_alpha[0])`` read from device memory when the kernel runs (``log_alpha=``, a
one-element fp32 device tensor): nothing here synchronises with the host, and a step captured by ``GraphedStep`` follows a ``log_alpha``
that an optimiser changes between replays.  fp32 tensors on a ROCm device only; there is no CPU path.
"""
import math
from collections import namedtuple

import torch

from . import _lib
from .functional import _dev, _ptr, _stream

CriticLoss = namedtuple("CriticLoss", ["loss", "td", "target"])
ActorLoss = namedtuple("ActorLoss", ["policy_loss", "alpha_loss"])
BCLoss = namedtuple("BCLoss", ["loss", "used"])
CQLLoss = namedtuple("CQLLoss", ["loss", "weight_loss", "gap", "used"])

MAX_ACTIONS, MAX_ELEMS = 16, 1 << 20      # sac_loss.hip


def _temperature(alpha, log_alpha, what):
    """(float alpha for the ABI, log_alpha tensor or None): exactly one of the two is given"""
    if (alpha is None) == (log_alpha is None):
        raise ValueError(f"{what}: give exactly one of alpha= (a float) and log_alpha= (a one-element fp32 device tensor)")
    if log_alpha is None:
        if isinstance(alpha, (bool, torch.Tensor)) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha):
            raise ValueError(f"{what}: alpha must be a finite float (a device-side temperature goes in as log_alpha=), got {alpha!r}")
        return float(alpha), None
    if not isinstance(log_alpha, torch.Tensor) or log_alpha.numel() != 1:
        raise ValueError(f"{what}: log_alpha must be a one-element tensor")
    return 0.0, log_alpha


def _matrix(t, name, what, shape=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or (shape is not None and tuple(t.shape) != shape):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what}: {name} must be " + ("(B, A)" if shape is None else str(shape)) + f", got {got}")
    B, A = t.shape
    if B < 1 or not 1 <= A <= MAX_ACTIONS or B * A > MAX_ELEMS:
        raise ValueError(f"{what}: {name} is {tuple(t.shape)}; needs 1 <= B, 1 <= A <= {MAX_ACTIONS} and B * A <= {MAX_ELEMS}")
    return (B, A)


def _column(t, name, what, B):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) not in ((B,), (B, 1)):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise ValueError(f"{what}: {name} must be ({B}, 1) or ({B},), got {got}")


def _on_device(named):
    """the shapes are checked by now: fp32 on a ROCm device or DgvitError; None stays None"""
    return [None if t is None else _dev(t, name) for name, t in named]


class _Precomputed(torch.autograd.Function):
    """A loss whose value and whose gradients for a unit upstream gradient the forward launch has already written: ``value`` is a 0-d
    view of the kernel's output, ``grads`` the saved buffer holding the gradients of ``inputs`` one after the other.  The backward is
    one launch, grads times the 0-d upstream gradient into a fresh buffer (the saved one serves a second backward unchanged)."""

    @staticmethod
    def forward(ctx, value, grads, *inputs):
        ctx.save_for_backward(grads)
        ctx.shapes = [tuple(t.shape) for t in inputs]
        return value.detach()

    @staticmethod
    def backward(ctx, g):
        grads, = ctx.saved_tensors
        g = _dev(g, "upstream gradient")
        out = torch.empty_like(grads)
        with torch.cuda.device(grads.device):
            rc = _lib.load().dgvit_sac_scale_grads(_ptr(grads), _ptr(out), grads.numel(), _ptr(g), _stream())
        _lib.check(rc, "dgvit_sac_scale_grads")
        res, o = [], 0
        for shape, need in zip(ctx.shapes, ctx.needs_input_grad[2:]):
            n = math.prod(shape)
            res.append(out[o:o + n].view(shape) if need else None)
            o += n
        return (None, None, *res)


def critic_loss(q1, q2, reward, next_q1, next_q2, next_log_pi, *, alpha=None, log_alpha=None, gamma=0.99, done=None, weights=None,
                discount=None):
    """``CriticLoss(loss, td, target)`` of the twin critics, one launch:

        target = reward + (1 - done) gamma (min(next_q1, next_q2) - alpha next_log_pi)           (B, A), detached: the no_grad target
        loss   = mean(weights (q1 - target)^2) + mean(weights (q2 - target)^2)                   0-d, differentiable in q1 and q2
        td     = |q1 - target|.mean(1)                                                           (B,), detached: update_priorities takes it

    ``done=None`` is 0 (the reference fetches ``dones`` and never applies them), ``weights=None`` is 1.  Nothing flows to ``next_*``,
    ``reward``, ``weights`` or ``log_alpha``.  ``loss.backward()`` is one further launch.

    ``discount=`` ((B,) or (B, 1) fp32 on the device) takes the place of ``gamma`` sample by sample,

        target = reward + (1 - done) discount_b (min(next_q1, next_q2) - alpha next_log_pi)

    which is the n-step target when ``reward``, ``done`` and ``discount`` are ``rew``, ``done`` and ``discount`` = gamma^m of
    ``DeviceReplayBuffer.sample(..., n_step=n)``.  With ``discount=`` the float ``gamma`` is not read."""
    what = "critic_loss"
    alpha_f, la = _temperature(alpha, log_alpha, what)
    if discount is None and (isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not math.isfinite(gamma)):
        raise ValueError(f"{what}: gamma must be a finite float, got {gamma!r}")
    B, A = _matrix(q1, "q1", what)
    for name, t in (("q2", q2), ("next_q1", next_q1), ("next_q2", next_q2)):
        _matrix(t, name, what, (B, A))
    for name, t in (("reward", reward), ("next_log_pi", next_log_pi), ("done", done), ("weights", weights), ("discount", discount)):
        if t is not None or name in ("reward", "next_log_pi"):
            _column(t, name, what, B)
    q1c, q2c, r, n1, n2, nlp, d, w, g, la = _on_device([("q1", q1), ("q2", q2), ("reward", reward), ("next_q1", next_q1), ("next_q2", next_q2),
                                                        ("next_log_pi", next_log_pi), ("done", done), ("weights", weights),
                                                        ("discount", discount), ("log_alpha", la)])
    need = torch.is_grad_enabled() and (q1.requires_grad or q2.requires_grad)
    dev = q1c.device
    target, td = torch.empty(B, A, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    grads = torch.empty(2 * B * A, dtype=torch.float32, device=dev) if need else None
    with torch.cuda.device(dev):
        if g is None:
            rc = _lib.load().dgvit_sac_critic_loss(_ptr(q1c), _ptr(q2c), _ptr(r), _ptr(d), _ptr(w), _ptr(n1), _ptr(n2), _ptr(nlp), _ptr(la),
                                                   alpha_f, float(gamma), _ptr(target), _ptr(td), _ptr(loss), _ptr(grads), B, A, _stream())
        else:
            rc = _lib.load().dgvit_sac_critic_loss_v2(_ptr(q1c), _ptr(q2c), _ptr(r), _ptr(d), _ptr(w), _ptr(g), _ptr(n1), _ptr(n2), _ptr(nlp),
                                                      _ptr(la), alpha_f, 0.0, _ptr(target), _ptr(td), _ptr(loss), _ptr(grads), B, A, _stream())
    _lib.check(rc, "dgvit_sac_critic_loss")
    value = loss.view(())
    if need:
        value = _Precomputed.apply(value, grads, q1, q2)
    return CriticLoss(value, td, target)


def actor_loss(log_pi, q1_pi, q2_pi, *, alpha=None, log_alpha=None, target_entropy=None):
    """``ActorLoss(policy_loss, alpha_loss)``, both from one launch:

        policy_loss = mean(alpha log_pi - min(q1_pi, q2_pi))            differentiable in log_pi, q1_pi and q2_pi, not in log_alpha
        alpha_loss  = -log_alpha mean(log_pi + target_entropy)          differentiable in log_alpha only; None without target_entropy

    The two are separate autograd nodes: backpropagate them one after the other in either order, or their sum.  Each backward is one
    launch; ``log_alpha.grad`` is a (1,) fp32 tensor as ``FlatAdam([log_alpha])`` consumes it."""
    what = "actor_loss"
    alpha_f, la = _temperature(alpha, log_alpha, what)
    if target_entropy is not None:
        if log_alpha is None:
            raise ValueError(f"{what}: target_entropy needs log_alpha= (the temperature loss is a function of log_alpha)")
        if isinstance(target_entropy, bool) or not isinstance(target_entropy, (int, float)) or not math.isfinite(target_entropy):
            raise ValueError(f"{what}: target_entropy must be a finite float, got {target_entropy!r}")
    B, A = _matrix(q1_pi, "q1_pi", what)
    _matrix(q2_pi, "q2_pi", what, (B, A))
    _column(log_pi, "log_pi", what, B)
    lp, q1c, q2c, la = _on_device([("log_pi", log_pi), ("q1_pi", q1_pi), ("q2_pi", q2_pi), ("log_alpha", la)])
    grad_on = torch.is_grad_enabled()
    need_pl = grad_on and (log_pi.requires_grad or q1_pi.requires_grad or q2_pi.requires_grad)
    need_al = grad_on and target_entropy is not None and log_alpha.requires_grad
    dev = q1c.device
    losses = torch.empty(2, dtype=torch.float32, device=dev)
    grads = torch.empty(B + 2 * B * A, dtype=torch.float32, device=dev) if need_pl else None
    dla = torch.empty(1, dtype=torch.float32, device=dev) if need_al else None
    with torch.cuda.device(dev):
        rc = _lib.load().dgvit_sac_actor_loss(_ptr(lp), _ptr(q1c), _ptr(q2c), _ptr(la), alpha_f,
                                              int(target_entropy is not None), float(target_entropy or 0.0), _ptr(losses), _ptr(grads), _ptr(dla),
                                              B, A, _stream())
    _lib.check(rc, "dgvit_sac_actor_loss")
    policy = losses[0]
    if need_pl:
        policy = _Precomputed.apply(policy, grads, log_pi, q1_pi, q2_pi)
    temp = None
    if target_entropy is not None:
        temp = losses[1]
        if need_al:
            temp = _Precomputed.apply(temp, dla, log_alpha)
    return ActorLoss(policy, temp)


def _same_device(what, named):
    """the tensors of one launch lie on one device (the first one's): the kernel runs there and reads every pointer there"""
    first = next(((n, t) for n, t in named if t is not None), None)
    for n, t in named:
        if t is not None and t.device != first[1].device:
            raise ValueError(f"{what}: {n} is on {t.device}, {first[0]} on {first[1].device}; all tensors of a call lie on one device")


def _mask(mask, what, B):
    """``mask`` after its shape check -> (tensor or None, 1 when its bytes are a bool tensor's): (B,) or (B, 1), bool or fp32"""
    if mask is None:
        return None, 0
    _column(mask, "mask", what, B)
    if mask.dtype not in (torch.bool, torch.float32):
        raise ValueError(f"{what}: mask must be bool or float32, got {mask.dtype}")
    if not mask.is_cuda:
        raise _lib.DgvitError(f"{what}: mask is on {mask.device}; the DGViT HIP path needs a ROCm device (no CPU fallback)")
    mask = mask.detach().contiguous()
    return (mask.view(torch.uint8), 1) if mask.dtype == torch.bool else (mask, 0)      # the bool's own bytes: no cast launch


def _bc(what, pred, action, mask, q, nll, B, A):
    """the one dgvit_sac_bc_loss launch of bc_loss and nll_loss, whose shape checks have run"""
    mk, u8 = _mask(mask, what, B)
    named = [("log_prob" if nll else "pred", pred), ("action", None if nll else action.detach())] + [(n, None if t is None else t.detach()) for n, t in q]
    _same_device(what, named + [("mask", mk)])
    p, a, q1d, q2d, q1p, q2p = _on_device(named)
    need = torch.is_grad_enabled() and pred.requires_grad
    dev = p.device
    out = torch.empty(2, dtype=torch.float32, device=dev)
    grads = torch.empty(B * A, dtype=torch.float32, device=dev) if need else None
    with torch.cuda.device(dev):
        rc = _lib.load().dgvit_sac_bc_loss(_ptr(p), _ptr(a), _ptr(mk), u8, _ptr(q1d), _ptr(q2d), _ptr(q1p), _ptr(q2p), int(nll), _ptr(out),
                                           _ptr(grads), B, A, _stream())
    _lib.check(rc, "dgvit_sac_bc_loss")
    loss = out[0]
    if need:
        loss = _Precomputed.apply(loss, grads, pred)
    return BCLoss(loss, out[1])


def bc_loss(pred, action, *, mask=None, q_demo=None, q_pi=None):
    """``BCLoss(loss, used)``: the behaviour-cloning term of an actor loss over the demonstration rows of a batch, one launch:

        l_b  = mean_a (pred_ba - action_ba)^2
        m_b  = mask_b: None = 1, a bool tensor, or fp32 weights >= 0 (0/1 or fractional); (B,) or (B, 1) on the device
        f_b  = 1, or with the Q-filter [ mean_a min(q1_demo, q2_demo)_b > mean_a min(q1_pi, q2_pi)_b ]      (strict: a tie does not apply)
        used = sum_b m_b f_b            loss = sum_b m_b f_b l_b / used, or 0 when used == 0

    ``pred`` is the policy's action for the batch's states (``sample()``'s action or its tanh(mean)), ``action`` the stored one, both
    (B, A).  ``q_demo=(q1, q2)`` are the critic's values of the stored actions and ``q_pi=(q1, q2)`` those of ``pred``, each (B, A), given
    together or not at all: the demonstration then counts only where the critic rates it above the policy's own action.  ``loss`` is 0-d
    and differentiable in ``pred`` only (the backward is one launch, as ``actor_loss``'s); ``used`` is a 0-d detached device tensor for
    logging.  Nothing reads a count back: when no row applies the loss and its gradients are exact zeros, never NaN, and a step
    captured by ``GraphedStep`` follows a mask refilled between replays."""
    what = "bc_loss"
    if (q_demo is None) != (q_pi is None):
        raise ValueError(f"{what}: q_demo= and q_pi= are given together or not at all")
    q = []
    B, A = _matrix(pred, "pred", what)
    _matrix(action, "action", what, (B, A))
    if q_demo is not None:
        for name, pair in (("q_demo", q_demo), ("q_pi", q_pi)):
            if not isinstance(pair, (tuple, list)) or len(pair) != 2:
                raise ValueError(f"{what}: {name} must be the pair (q1, q2) of (B, A) tensors")
            for j, t in enumerate(pair):
                _matrix(t, f"{name}[{j}]", what, (B, A))
                q.append((f"{name}[{j}]", t))
    else:
        q = [("q", None)] * 4
    return _bc(what, pred, action, mask, q, False, B, A)


def nll_loss(log_prob, *, mask=None):
    """``BCLoss(loss, used)``: maximum-likelihood behaviour cloning, ``bc_loss`` with ``l_b = -log_prob_b`` for ``log_prob`` = ``policy.log_prob(
    inp, batch["act"])``, (B,) or (B, 1); same ``mask``, same normalisation by ``used`` on the device, differentiable in ``log_prob`` only.
    There is no Q-filter here: its two sides are critic values of two ACTIONS, and this loss never forms the policy's action."""
    what = "nll_loss"
    if not isinstance(log_prob, torch.Tensor) or log_prob.dim() not in (1, 2) or (log_prob.dim() == 2 and log_prob.shape[1] != 1) \
            or not 1 <= log_prob.shape[0] <= MAX_ELEMS:
        got = tuple(log_prob.shape) if isinstance(log_prob, torch.Tensor) else type(log_prob).__name__
        raise ValueError(f"{what}: log_prob must be (B, 1) or (B,) with 1 <= B <= {MAX_ELEMS}, got {got}")
    return _bc(what, log_prob, None, mask, [("q", None)] * 4, True, log_prob.shape[0], 1)


def cql_penalty(q1_cat, q2_cat, q1_data, q2_data, *, log_w=None, temperature=1.0, weight=None, log_weight=None, target_gap=None, mask=None):
    """``CQLLoss(loss, weight_loss, gap, used)``: the CQL(H) penalty of a twin critic, one launch (``dgvit_sac_cql_penalty``):

        z        = q_cat[b, m, c] - log_w[b, m]                      q*_cat (B, M, C): the critic at M proposal actions per state
        lse[b,c] = T log sum_m exp(z / T)                            T = temperature; max-subtracted, in double
        gap_i    = sum_{b used, c} (lse_i - q_data_i) / (used C)     q*_data (B, C): the critic at the stored action; i = 1, 2
        loss     = w (gap_1 + gap_2)

    ``log_w`` (B, M) is the log-density of the proposal that drew action m: ``-sum_a log(2 scale_a)`` for uniform draws on the action box,
    ``log_prob`` for policy draws (``sample_many``); ``None`` is 0.  ``mask`` ((B,) or (B, 1), bool or fp32 weights, as ``bc_loss`` takes
    it) picks the rows the penalty applies to; ``used`` is their count, a 0-d device tensor.  ``w`` is the float ``weight=`` or
    ``exp(log_weight[0])``, read on the device when the kernel runs (exactly one of the two).  With ``log_weight=`` and ``target_gap=tau``
    this is the Lagrange form:

        loss        = w (gap_1 + gap_2 - 2 tau)                      w a constant here
        weight_loss = -exp(log_weight) (gap_1 + gap_2 - 2 tau)       differentiable in log_weight only, the gaps detached

    otherwise ``weight_loss`` is ``None``.  ``gap`` is (2,), detached.  ``loss`` is differentiable in q*_cat (w softmax_m(z / T) / (used C)
    on the used rows) and q*_data (-w / (used C)); nothing flows to ``log_w``.  When no row is used every output and gradient is an exact
    zero, never NaN.  Nothing synchronises with the host: a step captured by ``GraphedStep`` follows ``log_weight`` and ``mask``."""
    what = "cql_penalty"
    if (weight is None) == (log_weight is None):
        raise ValueError(f"{what}: give exactly one of weight= (a float) and log_weight= (a one-element fp32 device tensor)")
    if log_weight is None:
        if isinstance(weight, (bool, torch.Tensor)) or not isinstance(weight, (int, float)) or not math.isfinite(weight):
            raise ValueError(f"{what}: weight must be a finite float (a device-side weight goes in as log_weight=), got {weight!r}")
        if target_gap is not None:
            raise ValueError(f"{what}: target_gap needs log_weight= (the Lagrange multiplier's loss is a function of log_weight)")
    elif not isinstance(log_weight, torch.Tensor) or log_weight.numel() != 1:
        raise ValueError(f"{what}: log_weight must be a one-element tensor")
    if target_gap is not None and (isinstance(target_gap, bool) or not isinstance(target_gap, (int, float)) or not math.isfinite(target_gap)):
        raise ValueError(f"{what}: target_gap must be a finite float, got {target_gap!r}")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError(f"{what}: temperature must be a finite float > 0, got {temperature!r}")
    if not isinstance(q1_cat, torch.Tensor) or q1_cat.dim() != 3:
        got = tuple(q1_cat.shape) if isinstance(q1_cat, torch.Tensor) else type(q1_cat).__name__
        raise ValueError(f"{what}: q1_cat must be (B, M, C), got {got}")
    B, M, C = q1_cat.shape
    if B < 1 or M < 1 or not 1 <= C <= MAX_ACTIONS or B * (M + 1) * C > MAX_ELEMS:
        raise ValueError(f"{what}: q1_cat is {(B, M, C)}; needs 1 <= B, 1 <= M, 1 <= C <= {MAX_ACTIONS} and B * (M + 1) * C <= {MAX_ELEMS}")
    for name, t, shape in (("q2_cat", q2_cat, (B, M, C)), ("q1_data", q1_data, (B, C)), ("q2_data", q2_data, (B, C)), ("log_w", log_w, (B, M))):
        if (t is not None or name != "log_w") and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape):
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what}: {name} must be {shape}, got {got}")
    mk, u8 = _mask(mask, what, B)
    named = [("q1_cat", q1_cat), ("q2_cat", q2_cat), ("q1_data", q1_data), ("q2_data", q2_data), ("log_w", None if log_w is None else log_w.detach()),
             ("log_weight", None if log_weight is None else log_weight.detach())]
    _same_device(what, named + [("mask", mk)])
    c1, c2, d1, d2, lw, lwt = _on_device(named)
    inputs = (q1_cat, q2_cat, q1_data, q2_data)
    grad_on = torch.is_grad_enabled()
    need = grad_on and any(t.requires_grad for t in inputs)
    lagrange = target_gap is not None
    need_w = grad_on and lagrange and log_weight.requires_grad
    dev = c1.device
    out = torch.empty(5, dtype=torch.float32, device=dev)
    grads = torch.empty(2 * B * M * C + 2 * B * C, dtype=torch.float32, device=dev) if need else None
    dlw = torch.empty(1, dtype=torch.float32, device=dev) if need_w else None
    with torch.cuda.device(dev):
        rc = _lib.load().dgvit_sac_cql_penalty(_ptr(c1), _ptr(c2), _ptr(d1), _ptr(d2), _ptr(lw), _ptr(mk), u8, _ptr(lwt),
                                               float(weight or 0.0), float(temperature), float(target_gap or 0.0), int(lagrange), _ptr(out),
                                               _ptr(grads), _ptr(dlw), B, M, C, _stream())
    _lib.check(rc, "dgvit_sac_cql_penalty")
    loss = out[0]
    if need:
        loss = _Precomputed.apply(loss, grads, q1_cat, q2_cat, q1_data, q2_data)
    wl = None
    if lagrange:
        wl = out[1]
        if need_w:
            wl = _Precomputed.apply(wl, dlw, log_weight)
    return CQLLoss(loss, wl, out[2:4], out[4])
