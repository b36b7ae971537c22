"""GPU: the bf16 configuration at 225 to 288 tokens (ViT-B/16 at 256x256 and 128x160 depth frames with 8x10 patches: 257 tokens, the
token count of ViT-B/14 at 224x224).  The raw attention kernels against fp64 softmax attention with the bounds of tests/test_gpu_bf16.py, both forward kernels (the
per-item one below 512 (frame, head) items, the persistent one from 512 on), the backward, and the encoder at 257 tokens against the
oracle.  Before this change every call here failed with `tokens N=... outside [1, 224]`."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O  # noqa: E402

DH = 64
NS = [225, 241, 256, 257, 288]


@pytest.fixture(scope="module")
def F():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd.functional


def _qkv(B, N, H, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, N, 3 * H * DH, generator=g, dtype=torch.float64) * scale).float().to(torch.bfloat16).double()


def _split(qkv, H):
    B, N, _ = qkv.shape
    I = H * DH
    return [qkv[..., j * I:(j + 1) * I].reshape(B, N, H, DH).permute(0, 2, 1, 3) for j in range(3)]


def _ref_fwd(qkv, H):
    q, k, v = _split(qkv, H)
    dots = (q @ k.transpose(-1, -2)) * DH ** -0.5
    B, N = qkv.shape[:2]
    return (torch.softmax(dots, -1) @ v).permute(0, 2, 1, 3).reshape(B, N, H * DH), torch.logsumexp(dots, -1) / math.log(2.0)


def _within(got, ref, atol, rtol, msg):
    err = (got.detach().double().cpu() - ref).abs() / (atol + rtol * ref.abs())
    assert float(err.max()) <= 1.0, f"{msg}: {float(err.max()):.3f} x the bound"


# ------------------------------------------------------------------------------------------------ raw kernels
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B,H,want_lse", [(2, 3, True), (3, 2, False), (43, 12, True), (130, 4, False)],
                         ids=["item-lse", "item", "persistent-lse", "persistent"])
def test_attention_forward(F, N, B, H, want_lse):
    """B*H < 512: the per-item kernel (eight or nine waves); >= 512: the persistent kernel (items per workgroup 2 to 3, both LDS
    buffers end a stream, padding rows N..NP-1 that must read as zeros, an exactly full 288-row image)"""
    qkv = _qkv(B, N, H, seed=N + B)
    res = F.op_attention_bf16(qkv.float().to(torch.bfloat16).cuda(), H, DH, want_lse=want_lse)
    out, lse = res if want_lse else (res, None)
    ref, lref = _ref_fwd(qkv, H)
    _within(out, ref, 6e-3, 2 ** -7, f"out B{B} N{N} H{H}")
    if want_lse:
        _within(lse, lref, 2e-4, 0.0, f"lse B{B} N{N} H{H}")


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B,H", [(2, 3), (1, 12)])
def test_attention_backward(F, N, B, H):
    I = H * DH
    qkv = _qkv(B, N, H, seed=N + 1).requires_grad_(True)
    g = torch.Generator().manual_seed(N + 2)
    dout = torch.randn(B, N, I, generator=g, dtype=torch.float64).float().to(torch.bfloat16).double()
    ref, _ = _ref_fwd(qkv, H)
    (ref * dout).sum().backward()
    x = qkv.detach().float().to(torch.bfloat16).cuda()
    out, lse = F.op_attention_bf16(x, H, DH, want_lse=True)
    dqkv = F.op_attention_bwd_bf16(x, out, dout.float().to(torch.bfloat16).cuda(), lse, H, DH)
    got, r = dqkv.double().cpu(), qkv.grad
    for j, name in enumerate(("dq", "dk", "dv")):
        gj, rj = got[..., j * I:(j + 1) * I], r[..., j * I:(j + 1) * I]
        assert float((gj - rj).norm()) < 1.5e-2 * float(rj.norm()) + 1e-3, name
    _within(dqkv, r, 6e-2, 3e-2, f"dqkv B{B} N{N} H{H}")


@pytest.mark.parametrize("B,H", [(1, 2), (43, 12)], ids=["item", "persistent"])
def test_attention_large_logits_288(F, B, H):
    """the running maximum moves in the last key tiles (keys 250..287 dominate): the online-softmax rescale at nine key tiles"""
    N = 288
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, N, 3 * H * DH, generator=g, dtype=torch.float64)
    qkv[..., :H * DH] *= 4.0
    qkv[:, 250:, H * DH:2 * H * DH] *= 6.0
    qkv = qkv.float().to(torch.bfloat16).double()
    out = F.op_attention_bf16(qkv.float().to(torch.bfloat16).cuda(), H, DH)
    ref, _ = _ref_fwd(qkv, H)
    _within(out, ref, 1.5e-2, 2 ** -7, "large logits")


@pytest.mark.parametrize("N", [257, 288])
def test_attention_reproducible_and_equal_across_kernels(F, N):
    """bitwise equal from launch to launch; and a frame's output does not depend on which kernel ran it (the persistent kernel for a
    batch of 516 items, the per-item kernel for 12 of them): same fragments, same key-tile order, same arithmetic"""
    B, H = 43, 12
    x = _qkv(B, N, H, seed=7 * N).float().to(torch.bfloat16).cuda()
    a, la = F.op_attention_bf16(x, H, DH, want_lse=True)
    b, lb = F.op_attention_bf16(x, H, DH, want_lse=True)
    assert torch.equal(a, b) and torch.equal(la, lb), "not reproducible from launch to launch"
    one, l1 = F.op_attention_bf16(x[20:21].contiguous(), H, DH, want_lse=True)
    assert torch.equal(one, a[20:21]) and torch.equal(l1, la[20:21]), "per-item and persistent kernels differ"
    dout = _qkv(B, N, H, seed=N).float().to(torch.bfloat16).cuda()[..., :H * DH].contiguous()
    d1 = F.op_attention_bwd_bf16(x, a, dout, la, H, DH)
    d2 = F.op_attention_bwd_bf16(x, a, dout, la, H, DH)
    assert torch.equal(d1, d2), "backward not reproducible"


@pytest.mark.parametrize("N", [257, 288])
def test_attention_variants_are_bit_identical(F, N):
    """the A/B forms of the diagnostic library (persistent or per-item forward, eight- or nine-wave workgroups) give the same bits"""
    import dgvit_amd
    B, H = 43, 12
    x = _qkv(B, N, H, seed=N + 11).float().to(torch.bfloat16).cuda()
    dout = _qkv(B, N, H, seed=N + 12).float().to(torch.bfloat16).cuda()[..., :H * DH].contiguous()
    base = None
    with dgvit_amd.diagnostic_library() as lib:
        try:
            for bits in (3, 0, 1, 2):
                lib.dgvit_set_attention_bf16_long(bits)
                o, l = F.op_attention_bf16(x, H, DH, want_lse=True)
                d = F.op_attention_bwd_bf16(x, o, dout, l, H, DH)
                if base is None:
                    base = (o, l, d)
                else:
                    assert all(torch.equal(p, q) for p, q in zip(base, (o, l, d))), f"variant bits {bits} differ"
        finally:
            lib.dgvit_set_attention_bf16_long(-1)


# B = 440 frames x 12 heads at 257 tokens (ViT-B/14): 5 280 items over the persistent kernel's workgroups, in the style of
# tests/test_gpu_c5_bench_batch.py
def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _poison(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def test_attention_at_bench_batch_257_tokens():
    import dgvit_amd
    lib = dgvit_amd.load_library()
    B, H, N = 440, 12, 257
    I = H * DH
    g = torch.Generator(device="cuda").manual_seed(110)
    qkv = torch.randn(B, N, 3 * I, device="cuda", generator=g).to(torch.bfloat16)
    dout = torch.randn(B, N, I, device="cuda", generator=g).to(torch.bfloat16)
    out, lse = _poison((B, N, I), torch.bfloat16), _poison((B, H, N), torch.float32)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.dgvit_attention_forward_bf16(_ptr(qkv), _ptr(out), _ptr(lse), B, N, H, DH, stream) == 0, lib.dgvit_last_error()
    dqkv, delta = _poison((B, N, 3 * I), torch.bfloat16), _poison((B * H * N,), torch.float32)
    assert lib.dgvit_attention_backward_bf16(_ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), _ptr(dqkv), _ptr(delta), B, N, H, DH,
                                             stream) == 0, lib.dgvit_last_error()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any()) and bool(torch.isfinite(lse).all())
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(delta).all())
    items = {0, 1, 255, 256, 511, 512, 5119, 5120, B * H - 2, B * H - 1}
    items |= set(int(v) for v in np.random.RandomState(11).randint(0, B * H, size=14))
    worst = {"out": 0.0, "lse": 0.0, "dqkv": 0.0, "dqkv rel L2": 0.0}
    for it in sorted(items):
        f, h = divmod(it, H)
        q, k, v = (qkv[f, :, j * I + h * DH: j * I + (h + 1) * DH].double().cpu().requires_grad_(True) for j in range(3))
        dots = (q @ k.T) * DH ** -0.5
        ref = torch.softmax(dots, -1) @ v
        (ref * dout[f, :, h * DH:(h + 1) * DH].double().cpu()).sum().backward()
        o = out[f, :, h * DH:(h + 1) * DH].double().cpu()
        worst["out"] = max(worst["out"], float(((o - ref.detach()).abs() / (6e-3 + 2 ** -7 * ref.detach().abs())).max()))
        lref = torch.logsumexp(dots.detach(), -1) / math.log(2.0)
        worst["lse"] = max(worst["lse"], float((lse[f, h].double().cpu() - lref).abs().max() / 2e-4))
        for j, gr in enumerate((q.grad, k.grad, v.grad)):
            got = dqkv[f, :, j * I + h * DH: j * I + (h + 1) * DH].double().cpu()
            worst["dqkv"] = max(worst["dqkv"], float(((got - gr).abs() / (6e-2 + 3e-2 * gr.abs())).max()))
            worst["dqkv rel L2"] = max(worst["dqkv rel L2"], float((got - gr).norm()) / (1.5e-2 * float(gr.norm()) + 1e-3))
    print(f"[B={B} N={N}] attention, {len(items)} items: max error / bound = " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f"attention {k}: {v:.2f} x the bound"


# ------------------------------------------------------------------------------------------------ encoder at 257 tokens
# (ViT-B/14 and 7x7 patches have 257 tokens too, but the bf16 patch embedding takes patch areas that are multiples of 8 only)
VITB16 = O.GoTConfig(image=(256, 256), patch=(16, 16), dim=768, depth=2, heads=12, dim_head=64, mlp_dim=3072)
SMALL = O.GoTConfig(image=(128, 160), patch=(8, 10), dim=128, depth=2, heads=2, dim_head=64, mlp_dim=256)


def _got(cfg, params, pool="cls"):
    import dgvit_amd
    m = dgvit_amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=2, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads,
                      mlp_dim=cfg.mlp_dim, dim_head=cfg.dim_head, channels=1, pool=pool)
    m.load_state_dict(params, strict=True)
    return m.cuda().eval()


def _inputs(cfg, batch, seed):
    params = O.make_params(O.got_param_spec(cfg, prefix=""), seed)
    img, _, _, _ = O.make_inputs(cfg, batch, seed)
    goal = torch.from_numpy(np.random.RandomState(seed + 7).standard_normal((batch, cfg.dim))).float()
    return params, img, goal


@pytest.mark.parametrize("cfg,batch", [(VITB16, 3), (SMALL, 5)], ids=["vitb16_256_l2", "128x160p8x10"])
def test_encoder_forward_257_tokens(cfg, batch):
    assert cfg.tokens == 257
    params, img, goal = _inputs(cfg, batch, 31)
    m = _got(cfg, params).set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        feat = m(img.cuda(), goal.cuda()).cpu()
        dense = m.set_schedule(dense_last_block=True)(img.cuda(), goal.cuda()).cpu()
    emu = O.got_forward_bf16(params, img, goal, cfg, prefix="")
    ref32 = O.got_forward(params, img, goal, cfg, prefix="")
    d_emu, d32 = (feat - emu).abs(), (feat - ref32).abs()
    print(f"N=257 {cfg.dim}: vs emulation max {d_emu.max():.4f} mean {d_emu.mean():.5f} | vs fp32 max {d32.max():.4f} mean {d32.mean():.5f}"
          f" | emulation vs fp32 max {(emu - ref32).abs().max():.4f}")
    assert torch.isfinite(feat).all()
    # the bounds of test_encoder_bf16_vs_reference_and_oracle (the bf16-storage model stands in for the reference's autocast run)
    assert d_emu.max() < 2e-2 and d_emu.mean() < 3e-3
    assert d32.max() < max(3e-2, 2 * float((emu - ref32).abs().max()))
    assert d32.mean() < 6e-3
    assert (feat - dense).abs().max() < 2e-2, "token-0 last block and dense last block disagree"


@pytest.mark.parametrize("cfg,batch,pool", [(VITB16, 2, "cls"), (SMALL, 4, "cls"), (SMALL, 3, "mean")], ids=["vitb16_256_l2", "128x160p8x10", "128x160p8x10_mean"])
def test_encoder_gradients_257_tokens(cfg, batch, pool):
    """parameter, goal and frame gradients through the bf16 encoder within 2e-2 relative L2 of fp32 autograd on the oracle (as
    test_encoder_bf16_gradients and test_got_bf16_image_gradient)"""
    params, img, goal = _inputs(cfg, batch, 21)
    wout = torch.from_numpy(np.random.RandomState(29).standard_normal((batch, cfg.dim))).float()
    ps = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    g, x = goal.clone().requires_grad_(True), img.clone().requires_grad_(True)
    (O.got_forward(ps, x, g, cfg, prefix="", pool=pool) * wout).sum().backward()
    m = _got(cfg, params, pool).set_compute_dtype(torch.bfloat16)
    gd, xd = goal.cuda().requires_grad_(True), img.cuda().requires_grad_(True)
    (m(xd, gd) * wout.cuda()).sum().backward()
    ours = {k: v.grad for k, v in m.named_parameters()}
    errs = {}
    for k, ref in ((k, v.grad) for k, v in ps.items()):
        if ref is None or float(ref.abs().max()) == 0.0:
            assert ours[k] is None or float(ours[k].abs().max()) == 0.0, f"{k} should have no gradient"
            continue
        assert ours[k] is not None, f"{k}: no gradient"
        errs[k] = float((ours[k].cpu() - ref).norm() / ref.norm())
    errs["dgoal"] = float((gd.grad.cpu() - g.grad).norm() / g.grad.norm())
    errs["dimg"] = float((xd.grad.cpu() - x.grad).norm() / x.grad.norm())
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"N=257 {cfg.dim} {pool}: worst relative gradient error vs fp32 {worst}")
    assert worst[1] < 2e-2, {k: round(v, 4) for k, v in errs.items() if v > 2e-2}


def test_encoder_maps_257_tokens():
    """bf16 attention maps (all rows and goal rows) against an fp64 softmax of the bf16 model's q / k"""
    from test_gpu_attention_maps import _ref_maps_bf16
    params, img, goal = _inputs(SMALL, 3, 41)
    m = _got(SMALL, params).set_compute_dtype(torch.bfloat16)
    fa, ma = m.attention_maps(img.cuda(), goal.cuda(), rows="all")
    fg, mg = m.attention_maps(img.cuda(), goal.cuda(), rows="goal")
    ref = _ref_maps_bf16(params, img, goal, SMALL)
    ma, mg = ma.cpu().double(), mg.cpu().double()
    assert ma.shape[-2:] == (257, 257)
    assert float((ma - ref).abs().max()) < 2e-2 and float((mg - ref[..., 0, :]).abs().max()) < 2e-2
    assert float((mg - ma[..., 0, :]).abs().max()) < 1e-5
    assert float((ma.sum(-1) - 1).abs().max()) < 1e-5
    with torch.no_grad():
        assert torch.equal(fg.cpu(), m(img.cuda(), goal.cuda()).cpu())


def test_sac_policy_with_bf16_encoder_257_tokens():
    """a GoT SAC policy on the shipped 128x160 frames with 8x10 patches whose encoder (.trans) runs in bf16: forward close to the fp32
    oracle, backward gives finite parameter and frame gradients"""
    import dgvit_amd
    cfg = O.GoTConfig(image=(128, 160), patch=(8, 10), dim=64, depth=2, heads=4)
    params = O.make_params(O.policy_param_spec(cfg), 5)
    m = dgvit_amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    m.load_state_dict(params, strict=True)
    m = m.cuda().eval()
    m.trans.set_compute_dtype(torch.bfloat16)
    img, pstate, _, _ = O.make_inputs(cfg, 4, 5)
    x = img.cuda().requires_grad_(True)
    mean, log_std = m([x, pstate.cuda()])
    ((mean ** 2).mean() + (log_std ** 2).mean()).backward()
    rm, rl = O.policy_forward(params, img, pstate, cfg)
    assert float((mean.detach().cpu() - rm).abs().max()) < 5e-2 and float((log_std.detach().cpu() - rl).abs().max()) < 5e-2
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    k = "trans.transformer.layers.0.0.fn.to_qkv.weight"
    gq = dict(m.named_parameters())[k].grad
    assert gq is not None and bool(torch.isfinite(gq).all()) and float(gq.abs().max()) > 0


def test_encoder_full_size_vitb16_256():
    """ViT-B/16 on 256x256 frames (257 tokens) at full depth and a batch of 64 (768 items: the persistent forward): finite, unit RMS, and a frame's features are
    bitwise the same in a batch of 8 (96 items: the per-item kernel)"""
    import dgvit_amd
    cfg = O.GoTConfig(image=(256, 256), patch=(16, 16), dim=768, depth=12, heads=12, dim_head=64, mlp_dim=3072)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 5)
    params["layer_norm.g"] = torch.ones(cfg.dim)
    m = dgvit_amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=2, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads,
                      mlp_dim=cfg.mlp_dim, channels=1)
    m.load_state_dict(params, strict=True)
    m = m.cuda().eval().set_compute_dtype(torch.bfloat16)
    g = torch.Generator().manual_seed(0)
    img, goal = torch.rand(64, 256, 256, generator=g).cuda(), torch.randn(64, 768, generator=g).cuda()
    with torch.no_grad():
        full = m(img, goal)
        part = m(img[40:48], goal[40:48])
    assert torch.isfinite(full).all()
    torch.testing.assert_close(full.pow(2).mean(-1).sqrt(), torch.ones(64, device="cuda"), atol=1e-4, rtol=0)
    assert torch.equal(full[40:48], part)
