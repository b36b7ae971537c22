"""GPU: ``GoT(frame_channels=K)`` and the GoT SAC networks on channel-last frame stacks.

A contiguous (B, H, W, K) stack viewed as (B, H, W K) with patches of (ph, pw K) has the rows of einops'
'b (h p1) (w p2) c -> b (h w) (p1 p2 c)', so the K-channel encoder IS the single-channel encoder of the wider image:
  * twin bit-equality: against ``GoT(image (H, W K), patch (ph, pw K))`` with the same state dict on the reshaped input, features,
    parameter gradients, the frame gradient and the attention maps are bit-equal, fp32 and bf16 -- the same kernels on the same bytes;
  * column order through the real kernels: on an input whose only non-zero channel is c the K-channel model equals the single-channel
    ``GoT(image (H, W), patch (ph, pw))`` whose patch weight is w[:, c::K], to the project's fp32 parity tolerance (1e-4 on outputs,
    2e-3 relative on gradients: the sums are grouped differently, so not bit-equal).
Cases: image (12, 20), patch (3, 5), K in {2, 3} (pw K = 15 takes the non-gather patch path, 45 is a bf16 patch area that is no multiple
of 8); image (16, 16), patch 4, K = 4 (pw K = 16 takes the gather path).  B in {2, 33}: the block path and the GEMM schedule."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [((12, 20), (3, 5), 2), ((12, 20), (3, 5), 3), ((16, 16), (4, 4), 4)]
BATCHES = [2, 33]
DIM, DEPTH, HEADS = 64, 2, 2


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


def _got(amd, image, patch, K=1, seed=3):
    torch.manual_seed(seed)
    kw = {"frame_channels": K} if K != 1 else {}
    return amd.GoT(image_size=image, patch_size=patch, num_classes=2, dim=DIM, depth=DEPTH, heads=HEADS, mlp_dim=128, **kw)


def _inputs(B, image, K):
    g = torch.Generator().manual_seed(100 * B + K)
    x = torch.randint(0, 256, (B, *image, K), generator=g).float() / 255.0
    return x.cuda(), torch.randn(B, DIM, generator=g).cuda(), torch.randn(B, DIM, generator=g).cuda()


def _run(m, x, goal, w):
    """(features, frame gradient, parameter gradients) of (m(x, goal) * w).sum() in train mode under a fixed seed"""
    for q in m.parameters():
        q.grad = None
    x = x.clone().requires_grad_(True)
    torch.manual_seed(7)                         # the emb-dropout seed of this forward
    y = m(x, goal)
    (y * w).sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape
    return y.detach(), x.grad, {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("image, patch, K", CASES, ids=str)
def test_the_k_channel_encoder_is_the_single_channel_encoder_of_the_wider_image(amd, image, patch, K, B, dtype):
    H, W = image
    m = _got(amd, image, patch, K).cuda().set_compute_dtype(dtype)
    wide = _got(amd, (H, W * K), (patch[0], patch[1] * K), seed=4).cuda().set_compute_dtype(dtype)
    wide.load_state_dict(m.state_dict(), strict=True)
    x, goal, w = _inputs(B, image, K)
    y, dx, grads = _run(m, x, goal, w)
    yw, dxw, gradsw = _run(wide, x.view(B, H, W * K), goal, w)
    assert y.shape == (B, DIM) and _bits(y, yw), "features"
    assert dx.shape == (B, H, W, K) and dx.is_contiguous() and _bits(dx.view(B, H, W * K), dxw), "the frame gradient, reshaped"
    assert float(dx.abs().max()) > 0
    assert set(grads) == set(gradsw) and "to_patch_embedding.1.weight" in grads
    for k in grads:
        assert _bits(grads[k], gradsw[k]), k
    for rows in ("goal", "all"):
        for mod in (m, wide):
            mod.eval()
        (f, maps), (fw, mapsw) = m.attention_maps(x, goal, rows), wide.attention_maps(x.view(B, H, W * K), goal, rows)
        assert _bits(f, fw) and _bits(maps, mapsw), rows
        for mod in (m, wide):
            mod.train()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("image, patch, K", CASES, ids=str)
def test_the_patch_weights_columns_are_ordered_p1_p2_c(amd, image, patch, K, B):
    m = _got(amd, image, patch, K).cuda().eval()
    x, goal, w = _inputs(B, image, K)
    for c in range(K):
        single = _got(amd, image, patch, seed=5).cuda().eval()
        state = {k: v.clone() for k, v in m.state_dict().items()}
        state["to_patch_embedding.1.weight"] = state["to_patch_embedding.1.weight"][:, c::K].contiguous()
        single.load_state_dict(state, strict=True)
        only = torch.zeros_like(x)
        only[..., c] = x[..., c]
        y, dx, grads = _run(m, only, goal, w)
        ys, dxs, gradss = _run(single, x[..., c].contiguous(), goal, w)
        assert float((y - ys).abs().max()) <= 1e-4, ("features", c)

        def close(a, b, what):
            assert float((a - b).abs().max()) <= 2e-3 * float(b.abs().max()) + 1e-12, (what, c)

        close(dx[..., c], dxs, "the frame gradient of channel c")
        close(grads["to_patch_embedding.1.weight"][:, c::K], gradss["to_patch_embedding.1.weight"], "the patch weight's columns of channel c")
        for k in ("to_patch_embedding.1.bias", "pos_embedding", "transformer.layers.0.0.fn.to_qkv.weight"):
            close(grads[k], gradss[k], k)


def _filled_ring(amd, image, E=3, steps=8, dtype=torch.uint8):
    from dgvit_amd.replay import DeviceReplayBuffer
    buf = DeviceReplayBuffer(E * steps, obs_shape=image, num_envs=E, frame_dtype=dtype, seed=2)
    g = torch.Generator().manual_seed(9)
    frame = torch.randint(0, 256, (E, *image), generator=g, dtype=torch.uint8).cuda()
    for t in range(steps):
        nxt = torch.randint(0, 256, (E, *image), generator=g, dtype=torch.uint8).cuda()
        buf.add_vec(obs=frame, pobs=torch.randn(E, 2, generator=g), act=torch.randn(E, 2, generator=g), rew=torch.randn(E, generator=g),
                    next_obs=nxt, next_pobs=torch.randn(E, 2, generator=g), done=torch.zeros(E), episode_end=np.array([t == 4] * E))
        frame = nxt
    return buf


@pytest.mark.parametrize("image, patch, K", CASES[1:], ids=str)
def test_the_sac_networks_train_on_a_batch_straight_from_the_ring(amd, image, patch, K):
    from dgvit_amd.sac_networks import DeterministicGoTPolicy, GoTPolicy, GoTQNetwork
    buf = _filled_ring(amd, image)
    batch = buf.sample(16, frame_stack=K)
    assert batch["obs"].shape == (16, *image, K)
    torch.manual_seed(1)
    kw = dict(image_size=image, patch_size=patch, frame_channels=K)
    pi, q, det = GoTPolicy(2, 2, DEPTH, HEADS, DIM, **kw).to("cuda"), GoTQNetwork(2, 2, DEPTH, HEADS, DIM, **kw).to("cuda"), \
        DeterministicGoTPolicy(2, 2, DEPTH, HEADS, DIM, **kw).to("cuda")
    action, log_prob, mean = pi.sample([batch["obs"], batch["pobs"]])
    m2, log_std = pi([batch["next_obs"], batch["next_pobs"]])
    q1, q2 = q([batch["obs"], batch["pobs"], batch["act"]])
    a = det([batch["obs"], batch["pobs"]])
    assert action.shape == log_std.shape == q1.shape == a.shape == (16, 2) and log_prob.shape == (16, 1)
    (log_prob.sum() + (m2 ** 2).sum() + (q1 * q2).sum() + (a ** 2).sum()).backward()
    for net in (pi, q, det):
        g = net.trans.to_patch_embedding[1].weight.grad
        assert g is not None and g.shape == (DIM, patch[0] * patch[1] * K) and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    feats, maps = pi.attention_maps([batch["obs"], batch["pobs"]])
    assert maps.shape == (16, DEPTH, HEADS, (image[0] // patch[0]) * (image[1] // patch[1]) + 1)
    stack = batch["obs"][0].cpu().numpy()
    pi.eval()                                    # no embedding dropout: one frame alone and in a batch of three give one action
    act = pi.choose_action(stack, np.zeros(2, np.float32), evaluate=True)
    assert act.shape == (2,) and np.isfinite(act).all()
    many = pi.choose_action(batch["obs"][:3].cpu().numpy(), np.zeros((3, 2), np.float32), evaluate=True)
    assert many.shape == (3, 2) and np.allclose(many[0], act, rtol=0, atol=1e-4)
    for bad in (batch["obs"][..., 0], batch["obs"].permute(0, 3, 1, 2).contiguous(), batch["obs"][..., :K - 1].contiguous(),
                batch["obs"].permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)):
        with pytest.raises(ValueError, match=r"channel-last \(B, H, W, K\)"):
            pi.sample([bad, batch["pobs"]])
    with pytest.raises(ValueError, match=r"channel-last \(B, H, W, K\)"):
        pi.choose_action(stack[..., 0], np.zeros(2, np.float32))
