"""GPU: the bf16 configuration above 288 tokens (K / V-tiled bf16 attention, attention_bf16_long.hip; GoT.set_schedule(long_sequence_bf16=True)).
(1) the raw tiled kernels against fp64 softmax attention with the bounds of tests/test_gpu_bf16_288.py, at token counts on both sides of
every key-tile (32 / 64) and block (128 / 256) edge, with a leading query count, poisoned outputs and a poisoned delta scratch;
(2) large logits whose running maximum moves in the sixth 64-key tile; (3) agreement with the fused kernels up to 288 tokens;
(4) determinism and frame independence, bitwise; (5) the encoder at 321 and 577 tokens against the oracle, the flag's bit-identity at
257 tokens, maps, a SAC policy; (6) graph capture.  Before this change every call here failed: the symbols and the keyword were missing.

The bounds above 288 tokens were checked on the CPU first (tests/test_bf16_long_sequence_host.py::test_bounds_hold_for_the_restatement_at_1025_tokens:
an fp64 restatement with the kernels' bf16 roundings of P, dS and the outputs uses less than half of each bound at N = 1025)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O  # noqa: E402
from test_gpu_bf16_288 import DH, _got, _inputs, _qkv, _ref_fwd, _within  # noqa: E402

NS = [1, 31, 33, 64, 65, 127, 128, 129, 255, 257, 288, 289, 321, 577, 1025]


@pytest.fixture(scope="module")
def F():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd.functional


def _bf(t):
    return t.float().to(torch.bfloat16).cuda()


@functools.lru_cache(maxsize=None)
def _case(B, N, H):
    """(qkv, dout, out, lse, dqkv) in fp64, computed once per shape and shared (treated as read-only)"""
    qkv = _qkv(B, N, H, seed=1000 + N + B).requires_grad_(True)
    g = torch.Generator().manual_seed(N + 2)
    dout = torch.randn(B, N, H * DH, generator=g, dtype=torch.float64).float().to(torch.bfloat16).double()
    ref, lref = _ref_fwd(qkv, H)
    (ref * dout).sum().backward()
    return qkv.detach(), dout, ref.detach(), lref.detach(), qkv.grad


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


# ------------------------------------------------------------------------------------------------ (1) raw kernels vs fp64
@pytest.mark.parametrize("want_lse", [True, False], ids=["lse", "nolse"])
@pytest.mark.parametrize("N", NS)
def test_tiled_forward_matches_fp64(F, N, want_lse):
    B, H = (1, 1) if N == 1025 else (2, 3)
    qkv, _, ref, lref, _ = _case(B, N, H)
    out = _nan((B, N, H * DH), torch.bfloat16)
    res = F.op_attention_bf16_tiled(_bf(qkv), H, DH, want_lse=want_lse, out=out)
    out, lse = res if want_lse else (res, None)
    err = (out.double().cpu() - ref).abs() / (6e-3 + 2 ** -7 * ref.abs())
    print(f"forward N={N}: out {float(err.max()):.3f} x the bound")
    _within(out, ref, 6e-3, 2 ** -7, f"out N{N}")
    if want_lse:
        _within(lse, lref, 2e-4, 0.0, f"lse N{N}")


@pytest.mark.parametrize("N", [65, 321])
@pytest.mark.parametrize("nq", [1, 33, None])
def test_tiled_forward_leading_queries(F, N, nq):
    """rows < nq are computed against every key; rows >= nq of a NaN-poisoned out and lse stay NaN"""
    B, H = 2, 3
    nq = N if nq is None else nq
    qkv, _, ref, lref, _ = _case(B, N, H)
    out, lse = _nan((B, N, H * DH), torch.bfloat16), _nan((B, H, N), torch.float32)
    F.op_attention_bf16_tiled(_bf(qkv), H, DH, nq=nq, want_lse=True, out=out, lse=lse)
    _within(out[:, :nq], ref[:, :nq], 6e-3, 2 ** -7, f"out N{N} nq{nq}")
    _within(lse[..., :nq], lref[..., :nq], 2e-4, 0.0, f"lse N{N} nq{nq}")
    assert bool(torch.isnan(out[:, nq:]).all()) and bool(torch.isnan(lse[..., nq:]).all()), "rows >= nq were written"


@pytest.mark.parametrize("N", NS)
def test_tiled_backward_matches_fp64(F, N):
    B, H = 2, 3
    I = H * DH
    qkv, dout, _, _, r = _case(B, N, H)
    x = _bf(qkv)
    out, lse = F.op_attention_bf16_tiled(x, H, DH, want_lse=True)
    delta = _nan((B * H * N,), torch.float32)
    dqkv = F.op_attention_bwd_bf16_tiled(x, out, _bf(dout), lse, H, DH, delta=delta)
    assert bool(torch.isfinite(delta).all()), "the delta scratch is not fully written"
    dref = (out.double() * _bf(dout).double()).reshape(B, N, H, DH).sum(-1).permute(0, 2, 1).reshape(-1)
    assert float((delta.double() - dref).abs().max()) <= 1e-4 * (1.0 + float(dref.abs().max()))
    got = dqkv.double().cpu()
    for j, name in enumerate(("dq", "dk", "dv")):
        gj, rj = got[..., j * I:(j + 1) * I], r[..., j * I:(j + 1) * I]
        rel = float((gj - rj).norm()) / (1.5e-2 * float(rj.norm()) + 1e-3)
        print(f"backward N={N} {name}: {rel:.3f} x the relative-L2 bound")
        assert rel < 1.0, name
    _within(dqkv, r, 6e-2, 3e-2, f"dqkv N{N}")


# ------------------------------------------------------------------------------------------------ (2) large logits across tiles
def test_tiled_forward_large_logits_321(F):
    """the construction of test_attention_large_logits_288 with the dominant key in the last 64-key tile (key 320, the sixth tile's
    only key): the running maximum moves after the fifth tile, so the accumulator rescale runs on state carried across five tiles"""
    N, B, H = 321, 2, 2
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, N, 3 * H * DH, generator=g, dtype=torch.float64)
    qkv[..., :H * DH] *= 4.0
    qkv[:, 320:, H * DH:2 * H * DH] *= 6.0
    qkv = qkv.float().to(torch.bfloat16).double()
    out = F.op_attention_bf16_tiled(_bf(qkv), H, DH)
    ref, _ = _ref_fwd(qkv, H)
    _within(out, ref, 1.5e-2, 2 ** -7, "large logits")


# ------------------------------------------------------------------------------------------------ (3) agreement with the fused kernels
@pytest.mark.parametrize("N", [50, 197, 257, 288])
def test_tiled_kernels_agree_with_the_fused_ones(F, N):
    """both are within the fp64 bounds of the same reference (asserted for each); whether they are bitwise equal is reported"""
    B, H = 2, 3
    I = H * DH
    qkv, dout, ref, lref, r = _case(B, N, H)
    x, d = _bf(qkv), _bf(dout)
    ot, lt = F.op_attention_bf16_tiled(x, H, DH, want_lse=True)
    of, lf = F.op_attention_bf16(x, H, DH, want_lse=True)
    for o, l, name in ((ot, lt, "tiled"), (of, lf, "fused")):
        _within(o, ref, 6e-3, 2 ** -7, f"{name} out N{N}")
        _within(l, lref, 2e-4, 0.0, f"{name} lse N{N}")
    gt = F.op_attention_bwd_bf16_tiled(x, of, d, lf, H, DH)
    gf = F.op_attention_bwd_bf16(x, of, d, lf, H, DH)
    for gq, name in ((gt, "tiled"), (gf, "fused")):
        _within(gq, r, 6e-2, 3e-2, f"{name} dqkv N{N}")
        for j in range(3):
            gj, rj = gq.double().cpu()[..., j * I:(j + 1) * I], r[..., j * I:(j + 1) * I]
            assert float((gj - rj).norm()) < 1.5e-2 * float(rj.norm()) + 1e-3, (name, j)
    print(f"N={N}: forward bitwise equal {torch.equal(ot, of) and torch.equal(lt, lf)}, backward bitwise equal {torch.equal(gt, gf)}")


# ------------------------------------------------------------------------------------------------ (4) determinism, frame independence
def test_tiled_kernels_are_deterministic_and_frame_independent(F):
    N, B, H = 321, 5, 3
    x = _bf(_qkv(B, N, H, seed=77))
    d = _bf(_qkv(B, N, H, seed=78))[..., :H * DH].contiguous()
    a, la = F.op_attention_bf16_tiled(x, H, DH, want_lse=True)
    b, lb = F.op_attention_bf16_tiled(x, H, DH, want_lse=True)
    assert torch.equal(a, b) and torch.equal(la, lb), "forward not reproducible"
    g1 = F.op_attention_bwd_bf16_tiled(x, a, d, la, H, DH)
    g2 = F.op_attention_bwd_bf16_tiled(x, a, d, la, H, DH)
    assert torch.equal(g1, g2), "backward not reproducible"
    one, l1 = F.op_attention_bf16_tiled(x[3:4].contiguous(), H, DH, want_lse=True)
    assert torch.equal(one, a[3:4]) and torch.equal(l1, la[3:4]), "forward depends on the batch"
    go = F.op_attention_bwd_bf16_tiled(x[3:4].contiguous(), one, d[3:4].contiguous(), l1, H, DH)
    assert torch.equal(go, g1[3:4]), "backward depends on the batch"


# ------------------------------------------------------------------------------------------------ (5) the encoder
ENC321 = O.GoTConfig(image=(128, 160), patch=(8, 8), dim=64, depth=2, heads=2, dim_head=64, mlp_dim=128)
ENC577 = O.GoTConfig(image=(96, 96), patch=(4, 4), dim=64, depth=2, heads=2, dim_head=64, mlp_dim=128)
ENC = [(ENC321, 3), (ENC577, 2)]
ENC_IDS = ["321", "577"]


def _long(cfg, params, pool="cls", **schedule):
    return _got(cfg, params, pool).set_compute_dtype(torch.bfloat16).set_schedule(long_sequence_bf16=True, **schedule)


@pytest.mark.parametrize("cfg,batch", ENC, ids=ENC_IDS)
def test_encoder_forward_above_288_tokens(cfg, batch):
    """no-grad forward (token-0 last block: nq = 1) and dense last block against the bf16-storage oracle and the fp32 one"""
    assert cfg.tokens in (321, 577)
    params, img, goal = _inputs(cfg, batch, 31)
    m = _long(cfg, params)
    with torch.no_grad():
        feat = m(img.cuda(), goal.cuda()).cpu()
        dense = m.set_schedule(dense_last_block=True, long_sequence_bf16=True)(img.cuda(), goal.cuda()).cpu()
    emu = O.got_forward_bf16(params, img, goal, cfg, prefix="")
    ref32 = O.got_forward(params, img, goal, cfg, prefix="")
    d_emu, d32 = (feat - emu).abs(), (feat - ref32).abs()
    print(f"N={cfg.tokens}: vs emulation max {d_emu.max():.4f} mean {d_emu.mean():.5f} | vs fp32 max {d32.max():.4f} mean {d32.mean():.5f}")
    assert torch.isfinite(feat).all()
    assert d_emu.max() < 2e-2 and d_emu.mean() < 3e-3
    assert d32.max() < max(3e-2, 2 * float((emu - ref32).abs().max()))
    assert d32.mean() < 6e-3
    assert (feat - dense).abs().max() < 2e-2, "token-0 last block and dense last block disagree"


@pytest.mark.parametrize("cfg,batch,pool,schedule", [(ENC321, 3, "cls", {}), (ENC321, 2, "mean", {"wgrad_overlap": True}),
                                                     (ENC577, 2, "cls", {"dense_last_block": True}), (ENC577, 2, "mean", {})],
                         ids=["321-cls", "321-mean-overlap", "577-cls-dense", "577-mean"])
def test_encoder_gradients_above_288_tokens(cfg, batch, pool, schedule):
    """train-mode forward and backward: features against the bf16-storage oracle, parameter, goal and frame gradients within 2e-2
    relative L2 of fp32 autograd on the oracle"""
    params, img, goal = _inputs(cfg, batch, 21)
    wout = torch.from_numpy(np.random.RandomState(29).standard_normal((batch, cfg.dim))).float()
    ps = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    g, x = goal.clone().requires_grad_(True), img.clone().requires_grad_(True)
    (O.got_forward(ps, x, g, cfg, prefix="", pool=pool) * wout).sum().backward()
    m = _long(cfg, params, pool, **schedule)
    gd, xd = goal.cuda().requires_grad_(True), img.cuda().requires_grad_(True)
    feat = m(xd, gd)
    (feat * wout.cuda()).sum().backward()
    torch.cuda.synchronize()
    emu = O.got_forward_bf16(params, img, goal, cfg, prefix="", pool=pool)
    assert float((feat.detach().cpu() - emu).abs().max()) < 2e-2
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
    print(f"N={cfg.tokens} {pool}: worst relative gradient error vs fp32 {worst}")
    assert worst[1] < 2e-2, {k: round(v, 4) for k, v in errs.items() if v > 2e-2}


def test_flag_is_bit_identical_at_257_tokens():
    """N <= 288 with the flag set runs the fused kernels: forward, gradients and maps equal the unflagged model bit for bit"""
    cfg = O.GoTConfig(image=(128, 160), patch=(8, 10), dim=64, depth=2, heads=2, dim_head=64, mlp_dim=128)
    assert cfg.tokens == 257
    params, img, goal = _inputs(cfg, 3, 11)
    wout = torch.from_numpy(np.random.RandomState(3).standard_normal((3, cfg.dim))).float().cuda()

    def run(m):
        gd, xd = goal.cuda().requires_grad_(True), img.cuda().requires_grad_(True)
        f = m(xd, gd)
        (f * wout).sum().backward()
        with torch.no_grad():
            nf = m(img.cuda(), goal.cuda())
        fa, ma = m.attention_maps(img.cuda(), goal.cuda(), rows="all")
        fg, mg = m.attention_maps(img.cuda(), goal.cuda(), rows="goal")
        torch.cuda.synchronize()
        return [f.detach(), nf, gd.grad, xd.grad, fa, ma, fg, mg] + [p.grad for _, p in sorted(m.named_parameters()) if p.grad is not None]
    a = run(_got(cfg, params).set_compute_dtype(torch.bfloat16))
    b = run(_long(cfg, params))
    assert len(a) == len(b) > 20
    for i, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q), f"result {i} differs with the flag set"


def test_encoder_maps_321_tokens():
    from test_gpu_attention_maps import _ref_maps_bf16
    params, img, goal = _inputs(ENC321, 3, 41)
    m = _long(ENC321, params)
    fa, ma = m.attention_maps(img.cuda(), goal.cuda(), rows="all")
    fg, mg = m.attention_maps(img.cuda(), goal.cuda(), rows="goal")
    ref = _ref_maps_bf16(params, img, goal, ENC321)
    ma, mg = ma.cpu().double(), mg.cpu().double()
    assert ma.shape[-2:] == (321, 321)
    assert float((ma - ref).abs().max()) < 2e-2 and float((mg - ref[..., 0, :]).abs().max()) < 2e-2
    assert float((mg - ma[..., 0, :]).abs().max()) < 1e-5
    assert float((ma.sum(-1) - 1).abs().max()) < 1e-5
    with torch.no_grad():
        assert torch.equal(fg.cpu(), m(img.cuda(), goal.cuda()).cpu()), "the goal-row maps call does not return the forward's features"


def test_sac_policy_with_bf16_encoder_321_tokens():
    """a GoT SAC policy on the shipped 128x160 frames with 8x8 patches whose encoder (.trans) runs in bf16: forward close to the fp32
    oracle (the bound of test_sac_policy_with_bf16_encoder_257_tokens), backward gives finite parameter and frame gradients"""
    import dgvit_amd
    cfg = O.GoTConfig(image=(128, 160), patch=(8, 8), dim=64, depth=2, heads=4)
    assert cfg.tokens == 321
    params = O.make_params(O.policy_param_spec(cfg), 5)
    m = dgvit_amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    m.load_state_dict(params, strict=True)
    m = m.cuda().eval()
    m.trans.set_schedule(long_sequence_bf16=True).set_compute_dtype(torch.bfloat16)
    img, pstate, _, _ = O.make_inputs(cfg, 4, 5)
    x = img.cuda().requires_grad_(True)
    mean, log_std = m([x, pstate.cuda()])
    ((mean ** 2).mean() + (log_std ** 2).mean()).backward()
    rm, rl = O.policy_forward(params, img, pstate, cfg)
    assert float((mean.detach().cpu() - rm).abs().max()) < 5e-2 and float((log_std.detach().cpu() - rl).abs().max()) < 5e-2
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    gq = dict(m.named_parameters())["trans.transformer.layers.0.0.fn.to_qkv.weight"].grad
    assert gq is not None and bool(torch.isfinite(gq).all()) and float(gq.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ (6) graph capture
def test_captured_forward_replays_the_eager_one():
    """after one eager call the bf16 no-grad forward at 321 tokens is captured on a single stream and replays to the eager bits"""
    params, img, goal = _inputs(ENC321, 3, 53)
    m = _long(ENC321, params)
    img, goal = img.cuda(), goal.cuda()
    with torch.no_grad():
        eager = m(img, goal).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(img, goal)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = m(img, goal)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(static, eager)
