"""The SAC loss head on the device (include/dgvit_hip.h: The SAC loss head): the arithmetic of SAC.learn between the network
forwards and the backwards (DRL.py:384-425) -- the target, the twin-critic loss with ``done`` and importance weights, the |q1 - y| a
prioritized replay takes back, the actor loss and the temperature loss -- as one HIP launch per loss forward and one per backward.

    out = critic_loss(q1, q2, batch["rew"], q1n, q2n, next_log_pi, log_alpha=log_alpha, done=batch["done"], weights=batch["weights"])
    out.loss.backward(); critic_opt.step(); buf.update_priorities(batch["indexes"], out.td)
    policy_loss, alpha_loss = actor_loss(log_pi, q1_pi, q2_pi, log_alpha=log_alpha, target_entropy=-2.0)
    policy_loss.backward(); actor_opt.step()
    alpha_loss.backward(); alpha_opt.step()          # FlatAdam([log_alpha]); log_alpha.grad is a (1,) fp32 tensor

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
