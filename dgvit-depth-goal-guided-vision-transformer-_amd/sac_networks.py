"""MI355X-native twins of the GoT networks in the reference's ``got_sac_network.py``:
``GoTPolicy`` (:172-256), ``GoTQNetwork`` (:75-123), ``DeterministicGoTPolicy`` (:389-449).

Constructor signatures, attribute names (``trans``, ``fc_embed``, ``fc1`` ... used by DRL.py:107-111,145-148 to pick
optimiser sub-sets) and ``state_dict`` keys match the reference.  The encoder and every Linear run in
libdgvit_hip.so, and so does ``sample()`` (clamp / exp / tanh / log_prob and their gradients: one launch each way,
``functional.tanh_gaussian_sample``); only the N(0, 1) draw stays in PyTorch.

``image_size`` / ``patch_size`` are extra keyword arguments (default = the reference's hard-wired 128x160 @ 16x20).
"""
import numpy as np
import torch
from torch import nn
from torch.distributions import Normal

from . import functional as F_
from .goalformer import GoT

LOG_SIG_MAX = 2
LOG_SIG_MIN = -20
epsilon = 1e-6


def set_seed(seed):
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed(seed)


def weights_init_(m):
    """Xavier-uniform (gain 1) on every nn.Linear weight; biases keep PyTorch's default (got_sac_network.py:30-33)."""
    if isinstance(m, nn.Linear):
        torch.nn.init.xavier_uniform_(m.weight, gain=1)


def _lin(layer, x, relu=False):
    return F_.linear(x, layer.weight, layer.bias, relu=relu)


def _head(xs, towers, share=None):
    """relu(fc1) -> relu(fc2) -> third layer(s) on cat(xs): ONE fused HIP launch each way when the widths fit the fused head
    kernel (every network of the reference does), else the same arithmetic as a chain of MFMA GEMM launches.
    Returns [[y of third layer j of tower t]].  ``share``: see ``functional.mlp_head``; the chain repeats the shared pieces."""
    if share is None:
        if xs[0].shape[0] > 0 and F_.mlp_head_supported(xs, towers):
            return F_.mlp_head(xs, towers)
    elif xs[0].shape[0] > 0 and F_.mlp_head_supported(xs, towers, share):
        return F_.mlp_head(xs, towers, share)
    else:
        xs = [x if m == 1 else x.repeat_interleave(m, 0) for x, m in zip(xs, share)]
    x = xs[0] if len(xs) == 1 else torch.cat(xs, dim=1)
    out = []
    for l1, l2, l3s in towers:
        h = _lin(l2, _lin(l1, x, True), True)
        out.append([_lin(l3, h) for l3 in l3s])
    return out


def _standard_normal(like):
    """The N(0, 1) draw inside Normal.rsample (got_sac_network.py:242), made on the device.  Tests replace this function to
    inject the reference run's own draw."""
    return torch.randn_like(like)


def _tanh_gaussian(module, mean, log_std_raw):
    """sample() of got_sac_network.py:238-251 / :310-321 from the head outputs: (action, log_prob, tanh(mean) * scale + bias)."""
    if mean.shape[0] == 0:       # empty batch: the reference's torch ops accept it
        log_std = torch.clamp(log_std_raw, min=LOG_SIG_MIN, max=LOG_SIG_MAX)
        normal = Normal(mean, log_std.exp(), validate_args=False)
        x_t = normal.rsample()
        y_t = torch.tanh(x_t)
        log_prob = (normal.log_prob(x_t) - torch.log(module.action_scale * (1 - y_t.pow(2)) + epsilon)).sum(1, keepdim=True)
        return y_t * module.action_scale + module.action_bias, log_prob, torch.tanh(mean) * module.action_scale + module.action_bias
    scale, bias = module.action_scale, module.action_bias
    if scale.device != mean.device:          # module moved with .cuda() instead of the reference's .to(): follow it once
        module.action_scale, module.action_bias = scale, bias = scale.to(mean.device), bias.to(mean.device)
    return F_.tanh_gaussian_sample(mean, log_std_raw, _standard_normal(mean), scale, bias, LOG_SIG_MIN, LOG_SIG_MAX)


def _log_prob(module, mean, log_std_raw, action):
    """log_prob() of the tanh-Gaussian policies from the head outputs: the density sample() reports, at a given action"""
    if not isinstance(action, torch.Tensor) or action.shape != mean.shape:
        got = tuple(action.shape) if isinstance(action, torch.Tensor) else type(action).__name__
        raise ValueError(f"log_prob: action must be a {tuple(mean.shape)} tensor, one row per state, got {got}")
    scale, bias = module.action_scale, module.action_bias
    if scale.device != mean.device:
        module.action_scale, module.action_bias = scale, bias = scale.to(mean.device), bias.to(mean.device)
    return F_.tanh_gaussian_log_prob(mean, log_std_raw, action, scale, bias, LOG_SIG_MIN, LOG_SIG_MAX)


def _many_actions(inp, actions, nb_actions):
    """the checks of q_many, on the host before anything runs -> (istate, pstate, B, M)"""
    want = f"(B, M, nb_actions) = (B, M, {nb_actions}) with 1 <= M <= {F_.MAX_HEAD_SHARE}"
    if not isinstance(inp, (list, tuple)) or len(inp) != 2:
        raise ValueError(f"q_many: inp must be [istate, pstate] (the actions go in as the {want} second argument)")
    istate, pstate = inp
    if not torch.is_tensor(actions) or actions.dim() != 3 or actions.shape[2] != nb_actions or not 1 <= actions.shape[1] <= F_.MAX_HEAD_SHARE:
        got = tuple(actions.shape) if torch.is_tensor(actions) else type(actions).__name__
        raise ValueError(f"q_many: actions must be {want}, got {got}")
    if actions.dtype != torch.float32 or not actions.is_contiguous():
        raise ValueError(f"q_many: actions must be contiguous float32 {want}, got {actions.dtype}{'' if actions.is_contiguous() else ', not contiguous'}")
    if not torch.is_tensor(pstate) or pstate.dim() != 2 or pstate.shape[0] != actions.shape[0]:
        got = tuple(pstate.shape) if torch.is_tensor(pstate) else type(pstate).__name__
        raise ValueError(f"q_many: pstate must be (B, nb_pstate) with the B = {actions.shape[0]} of actions {tuple(actions.shape)}, got {got}")
    if not torch.is_tensor(istate) or istate.dim() < 3 or istate.shape[0] != actions.shape[0]:
        got = tuple(istate.shape) if torch.is_tensor(istate) else type(istate).__name__
        raise ValueError(f"q_many: istate must be a batch of B = {actions.shape[0]} frames, one per row of actions {tuple(actions.shape)}, got {got}")
    return istate, pstate, actions.shape[0], actions.shape[1]


def _sample_many(module, inp, n):
    """sample_many of the tanh-Gaussian policies: one encoder and head pass, then sample()'s launch on the head outputs repeated n times"""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"sample_many: n must be an int >= 1 (the result is (B, n, nb_actions)), got {n!r}")
    mean, log_std_raw = module._head_outputs(inp)
    B, A = mean.shape
    action, log_prob, tanh_mean = _tanh_gaussian(module, mean.repeat_interleave(n, 0), log_std_raw.repeat_interleave(n, 0))
    return action.view(B, n, A), log_prob.view(B, n), tanh_mean.view(B, n, A)[:, 0]


def _action_affine(action_space):
    if action_space is None:
        return torch.tensor(1.), torch.tensor(0.)
    return (torch.FloatTensor((action_space.high - action_space.low) / 2.),
            torch.FloatTensor((action_space.high + action_space.low) / 2.))


def _encoder_maps(module, inp, rows):
    istate, pstate = inp
    with torch.no_grad():
        goal = _lin(module.fc_embed, pstate)                    # no activation (:226, :429)
    return module.trans.attention_maps(istate, goal, rows)


def _encoder(dim, depth, heads, image_size, patch_size, frame_channels=1):
    return GoT(image_size=image_size, patch_size=patch_size, num_classes=2, dim=dim, depth=depth, heads=heads, mlp_dim=2048,
               channels=1, frame_channels=frame_channels)


class GoTQNetwork(nn.Module):
    """Twin-Q critic on GoT features: forward([istate, pstate, a]) -> (q1, q2), each (B, nb_actions)."""

    def __init__(self, nb_actions, nb_pstate, block, head, l_f_size, image_size=(128, 160), patch_size=(16, 20), *, frame_channels=1):
        super().__init__()
        self.trans = _encoder(l_f_size, block, head, image_size, patch_size, frame_channels)
        # dead parameters of the reference (got_sac_network.py:90-92): kept so checkpoints load strictly
        self.conv1 = nn.Conv2d(4, 16, 5, stride=2)
        self.conv2 = nn.Conv2d(16, 64, 5, stride=2)
        self.conv3 = nn.Conv2d(64, 256, 5, stride=2)
        self.avg = nn.AdaptiveAvgPool2d(output_size=(1, 1))
        self.fc1 = nn.Linear(l_f_size + nb_actions, 128)
        self.fc2 = nn.Linear(128, 32)
        self.fc3 = nn.Linear(32, nb_actions)
        self.fc_embed = nn.Linear(nb_pstate, l_f_size)
        self.fc11 = nn.Linear(l_f_size + nb_actions, 128)
        self.fc21 = nn.Linear(128, 32)
        self.fc31 = nn.Linear(32, nb_actions)
        self.apply(weights_init_)

    def forward(self, inp):
        istate, pstate, a = inp
        goal = _lin(self.fc_embed, pstate, relu=True)          # ReLU on the goal embedding (:111)
        feat = self.trans(istate, goal)
        (q1,), (q2,) = _head([feat.view(feat.size(0), -1), a], [(self.fc1, self.fc2, [self.fc3]), (self.fc11, self.fc21, [self.fc31])])
        return q1, q2

    def q_many(self, inp, actions):
        """``(q1, q2)``, each (B, M, nb_actions): both critics for M actions per state, ``actions`` a contiguous fp32 (B, M, nb_actions)
        device tensor and ``inp = [istate, pstate]`` -- the Q(s, a_m) of a CQL penalty (``sac_losses.cql_penalty``) or of a best-of-N
        evaluation (argmax over dim 1).  The encoder runs ONCE on the B frames; the fused head runs on the B * M rows and reads each
        state's features in place (``functional.mlp_head(share=)``).  Bit-equal to forward() on frames repeated M times, at the
        encoder's cost for B; differentiable in the parameters, in ``actions`` and in the frame where it asks for a gradient."""
        istate, pstate, B, M = _many_actions(inp, actions, self.fc3.out_features)
        goal = _lin(self.fc_embed, pstate, relu=True)
        feat = self.trans(istate, goal)
        (q1,), (q2,) = _head([feat.view(feat.size(0), -1), actions.view(B * M, -1)],
                             [(self.fc1, self.fc2, [self.fc3]), (self.fc11, self.fc21, [self.fc31])], share=[M, 1])
        return q1.view(B, M, -1), q2.view(B, M, -1)

    def attention_maps(self, inp, rows="goal"):
        """(features, maps) of the encoder (GoT.attention_maps) for the goal embedding forward computes; ``inp`` is [istate, pstate] or
        forward's [istate, pstate, a] (the action is not used)."""
        istate, pstate = inp[0], inp[1]
        with torch.no_grad():
            goal = _lin(self.fc_embed, pstate, relu=True)
        return self.trans.attention_maps(istate, goal, rows)


class GoTPolicy(nn.Module):
    """Tanh-Gaussian actor on GoT features."""

    def __init__(self, nb_actions, nb_pstate, block, head, l_f_size, action_space=None, image_size=(128, 160),
                 patch_size=(16, 20), *, frame_channels=1):
        super().__init__()
        self.trans = _encoder(l_f_size, block, head, image_size, patch_size, frame_channels)
        self.fc_embed = nn.Linear(nb_pstate, l_f_size)
        self.fc1 = nn.Linear(l_f_size, 128)
        self.fc2 = nn.Linear(128, 128)
        self.mean_linear = nn.Linear(128, nb_actions)
        self.log_std_linear = nn.Linear(128, nb_actions)
        self.device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
        self.apply(weights_init_)
        self.action_scale, self.action_bias = _action_affine(action_space)

    def choose_action(self, istate, pstate, evaluate=False):
        dev = self.fc1.weight.device
        K = getattr(self.trans, "frame_channels", 1)
        if K > 1:                               # a channel-last stack, (H, W, K) or (E, H, W, K), as replay.FrameStack returns it
            single = istate.ndim < 4
            istate = torch.as_tensor(istate).float().to(dev)
            pstate = torch.as_tensor(pstate).float().to(dev)
            if single:
                istate, pstate = istate.unsqueeze(0), pstate.unsqueeze(0)
            istate = istate.contiguous()
        elif istate.ndim < 4:
            istate = torch.FloatTensor(istate).float().permute(2, 0, 1)      # (H, W, 1) -> (1, H, W)
            pstate = torch.FloatTensor(pstate).float().unsqueeze(0)
        else:
            istate = torch.FloatTensor(istate).float().permute(0, 3, 1, 2)
            pstate = torch.FloatTensor(pstate).float()
        if K == 1:
            istate, pstate = istate.to(dev), pstate.to(dev)
        if evaluate is False:
            action, _, _ = self.sample([istate, pstate])
        else:
            _, _, action = self.sample([istate, pstate])
        return action.detach().squeeze(0).cpu().numpy()

    def _head_outputs(self, inp):
        istate, pstate = inp
        goal = _lin(self.fc_embed, pstate)                      # no activation (:226)
        feat = self.trans(istate, goal)
        ((mean, log_std_raw),) = _head([feat], [(self.fc1, self.fc2, [self.mean_linear, self.log_std_linear])])
        return mean, log_std_raw

    def forward(self, inp):
        mean, log_std_raw = self._head_outputs(inp)
        return mean, torch.clamp(log_std_raw, min=LOG_SIG_MIN, max=LOG_SIG_MAX)

    def attention_maps(self, inp, rows="goal"):
        """(features, maps) of the encoder (GoT.attention_maps) for the goal embedding forward computes from [istate, pstate]"""
        return _encoder_maps(self, inp, rows)

    def sample(self, inp):
        """(action, log_prob, tanh(mean)) of got_sac_network.py:238-251: clamp, exp, rsample, tanh and the tanh-corrected Gaussian
        log-density as ONE HIP launch behind the head (no Normal object: its argument check alone is a host sync per call)."""
        mean, log_std_raw = self._head_outputs(inp)
        return _tanh_gaussian(self, mean, log_std_raw)

    def sample_many(self, inp, n):
        """``(action (B, n, nb_actions), log_prob (B, n), tanh_mean (B, nb_actions))``: n draws per state from ONE encoder and head pass,
        ``sample``'s launch on the head outputs repeated n times (row b * n + j is draw j of state b).  The proposals of a CQL penalty:
        ``log_prob`` is their ``log_w``."""
        return _sample_many(self, inp, n)

    def log_prob(self, inp, action):
        """``log pi(action | inp)``, (B, 1): the density ``sample`` reports, at a given ``action`` (B, nb_actions) -- a demonstration's --
        with one HIP launch behind the head (``functional.tanh_gaussian_log_prob``).  Actions at or beyond the bounds are clipped to
        ``tanh^-1`` of +-(1 - 1e-6), so the value is finite.  Differentiable in the parameters, not in ``action``."""
        mean, log_std_raw = self._head_outputs(inp)
        return _log_prob(self, mean, log_std_raw, action)

    def to(self, device):
        self.action_scale = self.action_scale.to(device)
        self.action_bias = self.action_bias.to(device)
        return super().to(device)


class DeterministicGoTPolicy(nn.Module):
    def __init__(self, nb_actions, nb_pstate, block, head, l_f_size, action_space=None, image_size=(128, 160),
                 patch_size=(16, 20), *, frame_channels=1):
        super().__init__()
        self.trans = _encoder(l_f_size, block, head, image_size, patch_size, frame_channels)
        self.fc_embed = nn.Linear(nb_pstate, l_f_size)
        self.fc1 = nn.Linear(l_f_size, 128)
        self.fc2 = nn.Linear(128, 32)
        self.noise = torch.Tensor(nb_actions)
        self.apply(weights_init_)
        # created after the Xavier pass, as in the reference (:410-413): default nn.Linear init
        self.mean_linear = nn.Linear(32, nb_actions)
        self.log_std_linear = nn.Linear(32, nb_actions)
        self.action_scale, self.action_bias = _action_affine(action_space)

    def forward(self, inp):
        istate, pstate = inp
        goal = _lin(self.fc_embed, pstate)
        feat = self.trans(istate, goal)
        ((mean,),) = _head([feat.view(feat.size(0), -1)], [(self.fc1, self.fc2, [self.mean_linear])])
        return torch.tanh(mean) * self.action_scale + self.action_bias

    def attention_maps(self, inp, rows="goal"):
        """(features, maps) of the encoder (GoT.attention_maps) for the goal embedding forward computes from [istate, pstate]"""
        return _encoder_maps(self, inp, rows)

    def sample(self, inp):
        mean = self.forward(inp)
        noise = self.noise.normal_(0., std=0.1).clamp(-0.25, 0.25)
        return mean + noise, torch.tensor(0.), mean

    def to(self, device):
        self.action_scale = self.action_scale.to(device)
        self.action_bias = self.action_bias.to(device)
        self.noise = self.noise.to(device)
        return super().to(device)
