"""GPU: the K / V-tiled fp32 attention (attention_long.hip) and the long-sequence schedule flag (GoT.set_schedule(long_sequence=True)).

(1) the raw tiled kernels against an fp64 torch reference, below and above 288 tokens, with nq = 1; (2) agreement with the fused
kernels at N <= 288, and bit-identical GoT results with the flag at N <= 288; (3) the encoder at 321 / 358 / 785 tokens against the CPU
oracle; (4) transformer dropout at 321 tokens against the fp64 restatement of tests/layer_dropout_ref.py; (5) determinism and frame
independence; (6) graph capture.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O  # noqa: E402
import layer_dropout_ref as R  # noqa: E402

OUT_TOL = 1e-4
GRAD_RTOL = 2e-3
SEED = 0x5DEECE66D1234567


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


@pytest.fixture(scope="module")
def F(amd):
    return amd.functional


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def close(got, ref, atol, msg=""):
    np.testing.assert_allclose(got.detach().double().cpu().numpy(), ref.detach().double().cpu().numpy(), rtol=0, atol=atol, err_msg=msg)


def _attn_ref(qkv, H, dh):
    """fp64 attention: (out, base-2 lse)."""
    B, N, _ = qkv.shape
    I = H * dh
    q, k, v = (qkv[..., j * I:(j + 1) * I].reshape(B, N, H, dh).permute(0, 2, 1, 3) for j in range(3))
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    out = (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, N, I)
    return out, torch.logsumexp(s, -1) / math.log(2.0)


# ------------------------------------------------------------------------------------------------ (1) raw kernels vs fp64
RAW = [(2, 1, 3, 64), (2, 31, 1, 32), (1, 33, 3, 64), (2, 64, 1, 64), (1, 65, 3, 32), (2, 129, 3, 64), (1, 288, 1, 64), (2, 289, 3, 32),
       (2, 321, 1, 64), (1, 358, 3, 64), (2, 500, 3, 32), (1, 785, 3, 64), (1, 785, 1, 32), (1, 1025, 3, 64), (2, 1025, 1, 32)]


@pytest.mark.parametrize("B,N,H,dh", RAW)
def test_tiled_kernels_match_fp64(F, B, N, H, dh):
    qkv = rnd(B, N, 3 * H * dh, seed=N + dh)
    dout = rnd(B, N, H * dh, seed=N + 1)
    qr = qkv.clone().requires_grad_(True)
    ref, lse_ref = _attn_ref(qr, H, dh)
    ref.backward(dout)
    out, lse = F.op_attention_fwd_tiled(qkv.float().cuda(), H, dh)
    close(out, ref, 2e-5)
    close(lse, lse_ref, 2e-5)
    dqkv = F.op_attention_bwd_tiled(qkv.float().cuda(), out, dout.float().cuda(), lse, H, dh)
    close(dqkv, qr.grad, 1e-4)


@pytest.mark.parametrize("B,N,H,dh", [(2, 1, 2, 64), (2, 50, 2, 32), (1, 321, 3, 64), (2, 785, 2, 64), (1, 1025, 1, 32)])
def test_tiled_kernels_with_one_query(F, B, N, H, dh):
    """nq = 1 (the token-0-only last block): out / lse row 0, dq row 0 only (rows >= 1 untouched), dk / dv from every key."""
    I = H * dh
    qkv = rnd(B, N, 3 * I, seed=7 * N)
    dout = rnd(B, N, I, seed=7 * N + 1)
    dout[:, 1:] = 0.0
    qr = qkv.clone().requires_grad_(True)
    ref, lse_ref = _attn_ref(qr, H, dh)
    ref.backward(dout)
    out, lse = F.op_attention_fwd_tiled(qkv.float().cuda(), H, dh, nq=1)
    close(out[:, 0], ref[:, 0], 2e-5)
    close(lse[:, :, 0], lse_ref[:, :, 0], 2e-5)
    sentinel = torch.full((B, N, 3 * I), 7.0, device="cuda")
    dqkv = F.op_attention_bwd_tiled(qkv.float().cuda(), out, dout.float().cuda(), lse, H, dh, nq=1, dqkv=sentinel)
    close(dqkv[:, 0, :I], qr.grad[:, 0, :I], 1e-4)
    close(dqkv[:, :, I:], qr.grad[:, :, I:], 1e-4)
    assert bool((dqkv[:, 1:, :I] == 7.0).all()), "dq rows >= nq were written"


@pytest.mark.parametrize("N", [50, 321, 785])
def test_tiled_kernels_peaked_softmax(F, N):
    """Large logits (one key dominates each row): the running max must carry across the key tiles."""
    B, H, dh = 1, 2, 64
    qkv = rnd(B, N, 3 * H * dh, seed=3) * 6.0
    dout = rnd(B, N, H * dh, seed=4)
    qr = qkv.clone().requires_grad_(True)
    ref, lse_ref = _attn_ref(qr, H, dh)
    ref.backward(dout)
    out, lse = F.op_attention_fwd_tiled(qkv.float().cuda(), H, dh)
    close(out, ref, 5e-4)
    close(lse, lse_ref, 5e-4)
    dqkv = F.op_attention_bwd_tiled(qkv.float().cuda(), out, dout.float().cuda(), lse, H, dh)
    assert R.rel_err(dqkv.cpu().numpy(), qr.grad.numpy()) < 1e-4


# ------------------------------------------------------------------------------------------------ (2) below the limit
@pytest.mark.parametrize("N,H,dh", [(50, 2, 64), (257, 3, 64), (288, 2, 32)])
def test_tiled_kernels_agree_with_the_fused_ones(F, N, H, dh):
    B = 2
    qkv = rnd(B, N, 3 * H * dh, seed=N).float().cuda()
    dout = rnd(B, N, H * dh, seed=N + 1).float().cuda()
    o1, l1 = F.op_attention_fwd(qkv, H, dh)
    o2, l2 = F.op_attention_fwd_tiled(qkv, H, dh)
    close(o2, o1, 2e-5)
    close(l2, l1, 2e-5)
    close(F.op_attention_bwd_tiled(qkv, o1, dout, l1, H, dh), F.op_attention_bwd(qkv, o1, dout, l1, H, dh), 1e-4)


def _got(amd, cfg, pool="cls", dropout=0.0, emb_dropout=0.1):
    return R.build_got(amd, cfg, dropout, pool=pool, emb_dropout=emb_dropout)


def _inputs(cfg, B, seed):
    img, _, _, _ = O.make_inputs(cfg, B, seed)
    goal = torch.randn(B, cfg.dim, generator=torch.Generator().manual_seed(seed + 1))
    wout = torch.randn(B, cfg.dim, generator=torch.Generator().manual_seed(seed + 2))
    return img, goal, wout


def _run(m, img, goal, wout):
    for q in m.parameters():
        q.grad = None
    gg = goal.cuda().requires_grad_(True)
    feat = m(img.cuda(), gg)
    (feat * wout.cuda()).sum().backward()
    torch.cuda.synchronize()
    return feat.detach().cpu(), gg.grad.cpu(), {k: q.grad.cpu() for k, q in m.named_parameters() if q.grad is not None}


@pytest.mark.parametrize("image,patch,dense_last", [((84, 84), (12, 12), False), ((224, 224), (14, 14), False), ((224, 224), (14, 14), True)])
def test_flag_is_bit_identical_up_to_288_tokens(amd, image, patch, dense_last):
    cfg = O.GoTConfig(image=image, patch=patch, dim=64, depth=2, heads=2, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 31)
    img, goal, wout = _inputs(cfg, 3, 31)
    m = _got(amd, cfg)
    m.load_state_dict(params, strict=True)
    m = m.cuda().eval()
    a = _run(m.set_schedule(dense_last_block=dense_last), img, goal, wout)
    b = _run(m.set_schedule(dense_last_block=dense_last, long_sequence=True), img, goal, wout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


# ------------------------------------------------------------------------------------------------ (3) the encoder vs the CPU oracle
ENC = [  # image, patch, heads, dim_head, dim, pool, dense_last, B
    ((128, 160), (8, 8), 2, 64, 64, "cls", False, 3),      # 321 tokens, the shipped frames
    ((128, 160), (8, 8), 4, 32, 64, "cls", True, 2),
    ((136, 168), (8, 8), 1, 64, 64, "cls", False, 2),      # 358 tokens, heads == 1 and dim_head == dim: no output projection
    ((136, 168), (8, 8), 2, 32, 64, "mean", False, 2),
    ((224, 224), (8, 8), 4, 64, 64, "cls", False, 2),      # 785 tokens
    ((224, 224), (8, 8), 1, 32, 64, "mean", True, 2),
]


@pytest.mark.parametrize("image,patch,heads,dim_head,dim,pool,dense_last,B", ENC)
def test_encoder_above_288_tokens_matches_the_oracle(amd, image, patch, heads, dim_head, dim, pool, dense_last, B):
    cfg = O.GoTConfig(image=image, patch=patch, dim=dim, depth=2, heads=heads, dim_head=dim_head, mlp_dim=128)
    assert cfg.tokens > 288
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 41)
    img, goal, wout = _inputs(cfg, B, 41)
    m = _got(amd, cfg, pool=pool)
    m.load_state_dict(params, strict=True)
    m = m.cuda().eval().set_schedule(dense_last_block=dense_last, long_sequence=True)
    feat, dgoal, grads = _run(m, img, goal, wout)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    g2 = goal.clone().requires_grad_(True)
    ref = O.got_forward(p, img, g2, cfg, prefix="", pool=pool)
    (ref * wout).sum().backward()
    np.testing.assert_allclose(feat.numpy(), ref.detach().numpy(), rtol=0, atol=OUT_TOL)
    assert R.rel_err(dgoal.numpy(), g2.grad.numpy()) < GRAD_RTOL
    checked = 0
    for k, g in grads.items():
        if p[k].grad is None:
            continue
        err = R.rel_err(g.numpy(), p[k].grad.numpy())
        assert err < GRAD_RTOL, (k, err)
        checked += 1
    assert checked >= 12


# ------------------------------------------------------------------------------------------------ (4) transformer dropout
@pytest.mark.parametrize("heads,dim_head", [(2, 64), (2, 32)])
def test_dropout_above_288_tokens_matches_the_restatement(amd, heads, dim_head):
    """GoT(dropout=0.1) in train mode at 321 tokens against the fp64 restatement with the masks of the site table (site 0 indexed by
    ((b*H + h)*N + q)*ceil(N/4) + k/4, the general kernels' rule) drawn from the same seed."""
    cfg = O.GoTConfig(image=(128, 160), patch=(8, 8), dim=64, depth=2, heads=heads, dim_head=dim_head, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 43)
    B, p = 2, 0.1
    img, goal, wout = _inputs(cfg, B, 43)
    m = _got(amd, cfg, dropout=p)
    m.load_state_dict(params, strict=True)
    m = m.cuda().train().set_schedule(long_sequence=True)
    m.draw_dropout_seed = lambda: SEED
    feat, dgoal, grads = _run(m, img, goal, wout)
    masks = R.all_masks(cfg, B, SEED, 1.0 - p, 0.9)
    pd = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    g2 = goal.double().clone().requires_grad_(True)
    ref = R.got_forward_masked(pd, img.double(), g2, cfg, masks, keep=1.0 - p, emb_keep=0.9)
    (ref * wout.double()).sum().backward()
    np.testing.assert_allclose(feat.numpy(), ref.detach().numpy(), rtol=0, atol=OUT_TOL)
    assert R.rel_err(dgoal.numpy(), g2.grad.numpy()) < GRAD_RTOL
    for k, g in grads.items():
        if pd[k].grad is not None:
            err = R.rel_err(g.numpy(), pd[k].grad.numpy())
            assert err < GRAD_RTOL, (k, err)
    # the masks matter: without them the features differ by far more than the tolerance
    plain = O.got_forward({k: v.double() for k, v in params.items()}, img.double(), goal.double(), cfg, prefix="")
    assert float((feat.double() - plain).abs().max()) > 100 * OUT_TOL


# ------------------------------------------------------------------------------------------------ (5) determinism and invariance
def test_repeat_runs_are_bit_equal_and_overlap_matches(amd):
    cfg = O.GoTConfig(image=(128, 160), patch=(8, 8), dim=64, depth=2, heads=2, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 47)
    img, goal, wout = _inputs(cfg, 4, 47)
    m = _got(amd, cfg)
    m.load_state_dict(params, strict=True)
    m = m.cuda().eval().set_schedule(long_sequence=True)
    a = _run(m, img, goal, wout)
    b = _run(m, img, goal, wout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    c = _run(m.set_schedule(wgrad_overlap=True, long_sequence=True), img, goal, wout)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    for k in a[2]:
        assert R.rel_err(c[2][k].numpy(), a[2][k].numpy()) < 1e-6, k


@pytest.mark.parametrize("N,nq", [(321, 321), (785, 785), (785, 1)])
def test_a_frame_alone_equals_the_same_frame_in_a_batch(F, N, nq):
    H, dh, B, f = 3, 64, 8, 5
    qkv = rnd(B, N, 3 * H * dh, seed=N).float().cuda()
    dout = rnd(B, N, H * dh, seed=N + 1).float().cuda()
    o, l = F.op_attention_fwd_tiled(qkv, H, dh, nq=nq)
    d = F.op_attention_bwd_tiled(qkv, o, dout, l, H, dh, nq=nq, dqkv=torch.zeros_like(qkv))
    o1, l1 = F.op_attention_fwd_tiled(qkv[f:f + 1].contiguous(), H, dh, nq=nq)
    d1 = F.op_attention_bwd_tiled(qkv[f:f + 1].contiguous(), o1, dout[f:f + 1].contiguous(), l1, H, dh, nq=nq,
                                  dqkv=torch.zeros_like(qkv[f:f + 1]))
    torch.cuda.synchronize()
    assert torch.equal(o[f, :nq], o1[0, :nq]) and torch.equal(l[f, :, :nq], l1[0, :, :nq])
    assert torch.equal(d[f], d1[0])


# ------------------------------------------------------------------------------------------------ (6) graph capture
def test_captured_step_replays_the_eager_one(amd):
    from dgvit_amd import functional as F_
    cfg = O.GoTConfig(image=(128, 160), patch=(8, 8), dim=64, depth=2, heads=2, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 53)
    img, goal, wout = (t.cuda() for t in _inputs(cfg, 3, 53))
    m = _got(amd, cfg)
    m.load_state_dict(params, strict=True)
    m = m.cuda().eval().set_schedule(long_sequence=True)
    tab = m.param_table()

    def fb():
        gg = goal.clone().requires_grad_(True)
        f = F_.got_encoder(img, gg, m._cfg, tab)
        gr = torch.autograd.grad((f * wout).sum(), [gg, tab[4 + 2], tab[4 + 7]])
        return (f.detach(), *gr)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fb()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fb()
    graph.replay()
    torch.cuda.synchronize()
    eager = fb()
    torch.cuda.synchronize()
    for a, b in zip(static, eager):
        assert torch.equal(a, b)
