"""MI355X-native twins of the reference's CNN networks: ``QNetwork`` -- the critic the
shipped configuration trains with (``critic_type: "CNN"``, config.yaml:61; got_sac_network.py:125-170) -- and the
CNN actor ``GaussianPolicy`` (:258-327).  Same constructor signatures, attribute names and ``state_dict`` keys
(``conv1..3`` keep the reference's (cout, cin, 5, 5) weight layout); the conv stack is one fused HIP node
(functional.cnn_features), every Linear runs on the MFMA GEMM.

``frame_channels=K`` (keyword-only, 1 <= K <= 16) makes ``conv1`` an ``nn.Conv2d(K, 16, 5, stride=2)`` that reads the contiguous
channel-last (B, H, W, K) stacks of ``sample(frame_stack=K)`` / ``replay.FrameStack.push``: the network equals the reference module with
that conv1 applied to ``stack.permute(0, 3, 1, 2)``.  The stack is conv1's NHWC input as it stands -- no permute is made anywhere.
"""
import torch
from torch import nn
from torch.distributions import Normal

from . import functional as F_
from . import sac_networks as _S
from .goalformer import _frame_channels
from .sac_networks import LOG_SIG_MAX, LOG_SIG_MIN, epsilon, weights_init_, _lin, _head, _action_affine


class _ConvStack(nn.Module):
    def _make_convs(self, frame_channels=1):
        self.frame_channels = _frame_channels(frame_channels)
        self.conv1 = nn.Conv2d(self.frame_channels, 16, 5, stride=2)
        self.conv2 = nn.Conv2d(16, 64, 5, stride=2)
        self.conv3 = nn.Conv2d(64, 256, 5, stride=2)
        self.avg = nn.AdaptiveAvgPool2d(output_size=(1, 1))

    def _frames(self, istate):
        """``istate`` as the fused stack takes it: unchanged for single frames; with frame_channels = K > 1 a contiguous channel-last
        (B, H, W, K) stack, checked on the host before anything touches a device"""
        K = getattr(self, "frame_channels", 1)
        if K == 1:
            return istate
        if not torch.is_tensor(istate) or istate.dim() != 4 or istate.shape[3] != K or not istate.is_contiguous():
            got = (f"{tuple(istate.shape)}{'' if istate.is_contiguous() else ', not contiguous'}" if torch.is_tensor(istate)
                   else type(istate).__name__)
            raise ValueError(f"istate must be a contiguous channel-last (B, H, W, K) = (B, H, W, {K}) stack of frame_channels={K} frames, "
                             f"channel K - 1 the newest (a channel-first batch takes permute(0, 2, 3, 1).contiguous() first), got {got}")
        return istate

    def _features(self, istate):
        istate = self._frames(istate)
        return F_.cnn_features(istate, [self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                                        self.conv3.weight, self.conv3.bias])


class QNetwork(_ConvStack):
    """Twin-Q CNN critic: forward([istate (B,H,W), pstate (B,2), a (B,2)]) -> (q1, q2); istate (B,H,W,K) with frame_channels=K."""

    def __init__(self, nb_actions, nb_pstate, *, frame_channels=1):
        super().__init__()
        self._make_convs(frame_channels)
        self.fc1 = nn.Linear(256 + 32 + nb_actions, 128)
        self.fc2 = nn.Linear(128, 32)
        self.fc3 = nn.Linear(32, nb_actions)
        self.fc_embed = nn.Linear(nb_pstate, 32)
        self.fc11 = nn.Linear(256 + 32 + nb_actions, 128)
        self.fc21 = nn.Linear(128, 32)
        self.fc31 = nn.Linear(32, nb_actions)
        self.apply(weights_init_)

    def forward(self, inp):
        istate, pstate, a = inp
        x1 = self._features(istate)
        x2 = _lin(self.fc_embed, pstate, relu=True)
        (q1,), (q2,) = _head([x1, x2, a], [(self.fc1, self.fc2, [self.fc3]), (self.fc11, self.fc21, [self.fc31])])
        return q1, q2

    def q_many(self, inp, actions):
        """``(q1, q2)``, each (B, M, nb_actions), for ``actions`` (B, M, nb_actions) and ``inp = [istate, pstate]``: ``GoTQNetwork.q_many``
        behind the CNN stack.  The conv stack and fc_embed run once on the B frames; the head's 256 conv features and 32 goal features
        are both shared by the M rows of a state."""
        istate, pstate, B, M = _S._many_actions(inp, actions, self.fc3.out_features)
        x1 = self._features(istate)
        x2 = _lin(self.fc_embed, pstate, relu=True)
        (q1,), (q2,) = _head([x1, x2, actions.view(B * M, -1)], [(self.fc1, self.fc2, [self.fc3]), (self.fc11, self.fc21, [self.fc31])],
                             share=[M, M, 1])
        return q1.view(B, M, -1), q2.view(B, M, -1)


class GaussianPolicy(_ConvStack):
    """Tanh-Gaussian CNN actor (got_sac_network.py:258-327); istate (B,H,W,K) with frame_channels=K."""

    def __init__(self, nb_actions, nb_pstate, action_space=None, *, frame_channels=1):
        super().__init__()
        self._make_convs(frame_channels)
        self.fc_embed = nn.Linear(nb_pstate, 32)
        self.fc1 = nn.Linear(256 + 32, 128)
        self.fc2 = nn.Linear(128, 32)
        self.mean_linear = nn.Linear(32, nb_actions)
        self.log_std_linear = nn.Linear(32, nb_actions)
        self.apply(weights_init_)
        self.action_scale, self.action_bias = _action_affine(action_space)

    def _head_outputs(self, inp):
        istate, pstate = inp
        xs = [self._features(istate), _lin(self.fc_embed, pstate)]                    # no activation on the goal (:299)
        ((mean, log_std_raw),) = _head(xs, [(self.fc1, self.fc2, [self.mean_linear, self.log_std_linear])])
        return mean, log_std_raw

    def forward(self, inp):
        mean, log_std_raw = self._head_outputs(inp)
        return mean, torch.clamp(log_std_raw, min=LOG_SIG_MIN, max=LOG_SIG_MAX)

    def sample(self, inp):
        mean, log_std_raw = self._head_outputs(inp)
        return _S._tanh_gaussian(self, mean, log_std_raw)

    def sample_many(self, inp, n):
        """``(action (B, n, nb_actions), log_prob (B, n), tanh_mean (B, nb_actions))``: ``GoTPolicy.sample_many`` behind the CNN head"""
        return _S._sample_many(self, inp, n)

    def log_prob(self, inp, action):
        """``log pi(action | inp)``, (B, 1), at a given ``action`` (B, nb_actions): ``GoTPolicy.log_prob`` behind the CNN head"""
        mean, log_std_raw = self._head_outputs(inp)
        return _S._log_prob(self, mean, log_std_raw, action)

    def to(self, device):
        self.action_scale = self.action_scale.to(device)
        self.action_bias = self.action_bias.to(device)
        return super().to(device)
