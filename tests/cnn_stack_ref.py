"""fp64 reference of the CNN critic / actor on channel-last frame stacks, and the exact data its parity cases run on.

The reference is the reference module itself with ``nn.Conv2d(K, 16, 5, stride=2)``: three times relu(conv2d(., stride=2)) on
``stack.permute(0, 3, 1, 2)`` in fp64, the mean over space, then the heads of the oracle's ``cnn_qnet_forward`` / ``cnn_policy_forward``.
Gradients come from autograd.

Inputs must not sit on a ReLU kink.  With N(0, 1)-style parameters an fp32 pre-activation within rounding of zero flips its mask against
fp64, and a whole unit's gradient changes (torch fp32 against fp64 on the CPU missed the tolerance by 12x and 1600x at two of 42 such
cases, from one flip each).  So the parity data makes every forward sum exact in fp32 in ANY order: frames are integers in {0, 1, 2, 3},
the conv weights ternary {-1, 0, 1} (density 0.5, 0.1, 0.03), the biases integers in [-3, 0], [-7, 0], [-15, 0].  Every partial sum is
then an integer below ``max conv(|x|, |w|) + |b|``, which ``features`` asserts to be < 2^24 at every layer: fp32 pre-activations equal
the fp64 ones bit for bit and the masks agree by construction (relu'(0) = 0 on both sides).  The head parameters and the output
weights are N(0, 1)."""
import functools

import numpy as np
import torch

from helpers import O

FRAMES = [(29, 29), (30, 37), (61, 75)]      # the smallest frame (conv3 output 1 x 1); an even height (the last row is in no window); ragged
CHANNELS = [2, 3, 4, 5, 8, 16]               # 2, 3, 5: padded rows (KP 52, 76, 128); 4, 8: float4 / loader routes; 16: the maximum (KP 400)
BATCHES = [3, 33]
CASES = [(hw, K, B) for hw in FRAMES for K in CHANNELS for B in BATCHES]
CONV = ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias"]
EXACT = float(1 << 24)

OUT_TOL = 2e-5        # outputs and features: max-abs <= OUT_TOL * max(1, max |ref|)
GRAD_RTOL = 2e-3      # conv and head gradients (tests/test_gpu_parity.py::test_cnn_stack_vs_oracle_batch)
GRAD_ATOL = 2e-5      # ... atol = GRAD_ATOL * max(1, max |ref|)
DIMG_TOL = 1e-4       # frame gradient, relative L2 (tests/test_gpu_input_grad.py::test_cnn_image_gradient)


def param_spec(kind, K):
    spec = O.cnn_qnet_param_spec() if kind == "qnet" else O.cnn_policy_param_spec()
    return [(n, (16, K, 5, 5) if n == "conv1.weight" else s, t) for n, s, t in spec]


def _ternary(g, shape, density):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float() * (torch.rand(shape, generator=g) < density).float()


def exact_params(kind, K, seed=0):
    """state dict (fp32, CPU) of the network `kind` ('qnet' / 'policy') with frame_channels = K on the exact conv data"""
    g = torch.Generator().manual_seed(1000 * seed + K)
    p = {}
    for name, shape, _ in param_spec(kind, K):
        layer = {"conv1": 0, "conv2": 1, "conv3": 2}.get(name.split(".")[0])
        if layer is None:
            p[name] = torch.randn(shape, generator=g)
        elif name.endswith("weight"):
            p[name] = _ternary(g, shape, (0.5, 0.1, 0.03)[layer])
        else:
            p[name] = -torch.randint(0, (4, 8, 16)[layer], shape, generator=g).float()
    return p


def exact_stack(B, hw, K, seed=0):
    """(B, H, W, K) channel-last stack of integer frames in {0, 1, 2, 3}"""
    g = torch.Generator().manual_seed(7919 * seed + 131 * B + 17 * hw[0] + hw[1] + K)
    return torch.randint(0, 4, (B, *hw, K), generator=g).float()


def small_inputs(B, seed=0):
    g = torch.Generator().manual_seed(seed + B)
    return torch.rand(B, 2, generator=g), torch.rand(B, 2, generator=g) * 2 - 1      # pstate, action


def out_weights(B, n, seed=0):
    return [torch.randn(B, 2, generator=torch.Generator().manual_seed(seed + 50 + i)) for i in range(n)]


def features(p, stack, bounds=None):
    """(B, 256) fp64 features of the channel-last stack; asserts the exactness bound of every layer (appended to `bounds`)"""
    x = stack.permute(0, 3, 1, 2)
    for i in (1, 2, 3):
        w, b = p[f"conv{i}.weight"], p[f"conv{i}.bias"]
        with torch.no_grad():
            bound = float((torch.nn.functional.conv2d(x.detach().abs(), w.detach().abs(), stride=2)
                           + b.detach().abs()[None, :, None, None]).max())
        assert bound < EXACT, f"conv{i}: a partial sum may reach {bound:.3g} >= 2^24, the fp32 forward is not exact"
        if bounds is not None:
            bounds.append(bound)
        x = torch.relu(torch.nn.functional.conv2d(x, w, b, stride=2))
    return x.mean(dim=(2, 3))


def forward(kind, p, stack, pstate, a=None):
    """(q1, q2) of QNetwork.forward / (mean, log_std) of GaussianPolicy.forward (oracle: cnn_qnet_forward, cnn_policy_forward)"""
    lin = O.linear
    x1 = features(p, stack)
    if kind == "qnet":
        x = torch.cat([x1, torch.relu(lin(pstate, p["fc_embed.weight"], p["fc_embed.bias"])), a], dim=1)
        outs = []
        for f1, f2, f3 in (("fc1", "fc2", "fc3"), ("fc11", "fc21", "fc31")):
            h = torch.relu(lin(x, p[f1 + ".weight"], p[f1 + ".bias"]))
            h = torch.relu(lin(h, p[f2 + ".weight"], p[f2 + ".bias"]))
            outs.append(lin(h, p[f3 + ".weight"], p[f3 + ".bias"]))
        return tuple(outs)
    x = torch.cat([x1, lin(pstate, p["fc_embed.weight"], p["fc_embed.bias"])], dim=1)       # no activation on the goal
    x = torch.relu(lin(x, p["fc1.weight"], p["fc1.bias"]))
    x = torch.relu(lin(x, p["fc2.weight"], p["fc2.bias"]))
    mean = lin(x, p["mean_linear.weight"], p["mean_linear.bias"])
    return mean, lin(x, p["log_std_linear.weight"], p["log_std_linear.bias"]).clamp(O.LOG_SIG_MIN, O.LOG_SIG_MAX)


def loss(outs, wts):
    return sum((o * w.to(o)).sum() for o, w in zip(outs, wts))


@functools.lru_cache(maxsize=None)
def reference(kind, hw, K, B):
    """fp64 results of one case, computed once and left unchanged: {'outs', 'feat', 'grads' (by parameter name), 'dstack'}"""
    p = {k: v.double().requires_grad_(True) for k, v in exact_params(kind, K).items()}
    stack = exact_stack(B, hw, K).double().requires_grad_(True)
    pstate, a = (t.double() for t in small_inputs(B))
    outs = forward(kind, p, stack, pstate, a)
    loss(outs, out_weights(B, 2)).backward()
    with torch.no_grad():
        feat = features(p, stack)
    return {"outs": [o.detach() for o in outs], "feat": feat, "grads": {k: v.grad for k, v in p.items()}, "dstack": stack.grad}


def rel_l2(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def check_close(got, ref, what):
    """max-abs <= OUT_TOL * max(1, max |ref|)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err, scale = float((got - ref).abs().max()), max(1.0, float(ref.abs().max()))
    assert err <= OUT_TOL * scale, f"{what}: max-abs error {err:.3e} > {OUT_TOL} * {scale:.3e}"


def check_grad(got, ref, what):
    assert got is not None, f"{what}: no gradient"
    r = ref.detach().double().cpu().numpy()
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), r, rtol=GRAD_RTOL, atol=GRAD_ATOL * max(1.0, float(np.abs(r).max())),
                               err_msg=what)
