"""GPU: transformer-internal dropout of the fp32 encoder (GoT(dropout=p), GoalFormer.py:47, 49, 68, 78), forward and backward.

The masks are taken from the host restatement of tests/layer_dropout_ref.py (Philox4x32-10 + the site table of include/dgvit_hip.h)
and fed to an fp64 CPU model of the encoder; the module under test draws them itself from the one seed of the forward.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O  # noqa: E402
import layer_dropout_ref as R  # noqa: E402

OUT_TOL = 1e-4
GRAD_RTOL = 2e-3
SEED = 0x2545F4914F6CDD1D


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


def _module(amd, cfg, p, params, pool="cls", dense_last=False, overlap=False, seed=SEED):
    m = R.build_got(amd, cfg, p, pool=pool)
    m.load_state_dict(params, strict=True)
    m = m.cuda().train().set_schedule(dense_last_block=dense_last, wgrad_overlap=overlap)
    m.draw_dropout_seed = lambda: seed      # the forward's one seed, fixed
    return m


def _run_module(m, img, goal, wout):
    gg = goal.cuda().requires_grad_(True)
    feat = m(img.cuda(), gg)
    (feat * wout.cuda()).sum().backward()
    torch.cuda.synchronize()
    return feat.detach().cpu(), gg.grad.cpu(), {k: q.grad.cpu() for k, q in m.named_parameters() if q.grad is not None}


def _run_reference(cfg, params, img, goal, wout, p, pool="cls", seed=SEED, emb_p=0.1):
    B = img.shape[0]
    masks = R.all_masks(cfg, B, seed, 1.0 - p, 1.0 - emb_p)
    pd = {k: v.double().clone().requires_grad_(True) for k, v in params.items()}
    g2 = goal.double().clone().requires_grad_(True)
    ref = R.got_forward_masked(pd, img.double(), g2, cfg, masks, keep=1.0 - p, emb_keep=1.0 - emb_p, pool=pool)
    (ref * wout.double()).sum().backward()
    return ref.detach(), g2.grad, {k: v.grad for k, v in pd.items() if v.grad is not None}


def _inputs(cfg, B, seed):
    img, _, _, _ = O.make_inputs(cfg, B, seed)
    goal = torch.randn(B, cfg.dim, generator=torch.Generator().manual_seed(seed + 1))
    wout = torch.randn(B, cfg.dim, generator=torch.Generator().manual_seed(seed + 2))
    return img, goal, wout


def _check(feat, dgoal, grads, ref, rgoal, rgrads):
    np.testing.assert_allclose(feat.numpy(), ref.numpy(), rtol=0, atol=OUT_TOL)
    assert R.rel_err(dgoal.numpy(), rgoal.numpy()) < GRAD_RTOL
    for k, r in rgrads.items():
        if k in grads:
            err = R.rel_err(grads[k].numpy(), r.numpy())
            assert err < GRAD_RTOL, (k, err)


# ------------------------------------------------------------------------------------------------ (1) the mask on the device
def test_restatement_matches_the_emb_dropout_kernel_bit_for_bit(amd):
    from dgvit_amd import functional as F_
    B, N, D, keep = 3, 50, 64, 0.7
    x = torch.ones(B * N * D, device="cuda")
    F_.op_dropout_(x, SEED, keep)
    got = (x.cpu() != 0).double().reshape(B, N, D)
    assert torch.equal(got, R.mask("emb", 0, (B, N, D), SEED, keep))


# ------------------------------------------------------------------------------------------------ (3) parity against fp64
_CASES = {
    # name: (cfg, B, p, pool, dense_last, overlap)
    "c84_p01": (O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2, mlp_dim=128), 4, 0.1, "cls", False, False),
    "c84_p05": (O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2, mlp_dim=128), 4, 0.5, "cls", False, False),
    "c84_dense": (O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2, mlp_dim=128), 4, 0.3, "cls", True, False),
    "c224_n257": (O.GoTConfig(image=(224, 224), patch=(14, 14), dim=64, depth=2, heads=2, mlp_dim=128), 2, 0.2, "cls", False, False),
    "dim_head32": (O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2, dim_head=32, mlp_dim=128), 4, 0.3, "cls", False, False),
    "no_projection": (O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=1, dim_head=64, mlp_dim=128), 4, 0.3, "cls", False, False),
    "pool_mean": (O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2, mlp_dim=128), 4, 0.3, "mean", False, False),
    "wgrad_overlap": (O.GoTConfig(image=(84, 84), patch=(12, 12), dim=128, depth=2, heads=2, mlp_dim=256), 4, 0.3, "cls", False, True),
    # T = 32 * 65 = 2080 rows, K = 2048: the fc2 GEMM (2080 x 64 x 2048) takes k-slices (tests/test_abi_and_host.py: split shapes)
    "split_k": (O.GoTConfig(image=(96, 96), patch=(12, 12), dim=64, depth=2, heads=2, mlp_dim=2048), 32, 0.2, "cls", False, False),
}


@pytest.mark.parametrize("name", list(_CASES))
def test_train_mode_matches_the_fp64_restatement_with_the_same_masks(amd, name):
    cfg, B, p, pool, dense_last, overlap = _CASES[name]
    if name == "split_k":
        assert amd.load_library().dgvit_gemm_scratch_floats(0, B * cfg.tokens, cfg.dim, cfg.mlp_dim) > 0
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 11)
    img, goal, wout = _inputs(cfg, B, 11)
    m = _module(amd, cfg, p, params, pool=pool, dense_last=dense_last, overlap=overlap)
    got = _run_module(m, img, goal, wout)
    ref = _run_reference(cfg, params, img, goal, wout, p, pool=pool)
    _check(*got, *ref)


# ------------------------------------------------------------------------------------------------ (4) schedule invariance
def test_dense_and_token0_last_blocks_draw_the_same_masks(amd):
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=3, heads=2, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 13)
    img, goal, wout = _inputs(cfg, 6, 13)
    a = _run_module(_module(amd, cfg, 0.3, params, dense_last=False), img, goal, wout)
    b = _run_module(_module(amd, cfg, 0.3, params, dense_last=True), img, goal, wout)
    assert float((a[0] - b[0]).abs().max()) <= 1e-6
    assert R.rel_err(a[1].numpy(), b[1].numpy()) < 1e-5
    for k in a[2]:
        assert R.rel_err(a[2][k].numpy(), b[2][k].numpy()) < 1e-5, k


def test_no_grad_train_mode_forward_equals_the_grad_enabled_one(amd):
    """B = 2 is a block-path size (block.hip) for no-grad passes: with transformer dropout the GEMM schedule runs instead."""
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=4, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 17)
    img, goal, wout = _inputs(cfg, 2, 17)
    m = _module(amd, cfg, 0.25, params)
    with torch.no_grad():
        f0 = m(img.cuda(), goal.cuda()).cpu()
    f1 = _run_module(m, img, goal, wout)[0]
    assert float((f0 - f1).abs().max()) <= 1e-6
    ref = _run_reference(cfg, params, img, goal, wout, 0.25)[0]
    np.testing.assert_allclose(f0.numpy(), ref.numpy(), rtol=0, atol=OUT_TOL)


# ------------------------------------------------------------------------------------------------ (5) no regression
def test_eval_mode_and_zero_dropout_are_unchanged(amd):
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 19)
    img, goal, wout = _inputs(cfg, 5, 19)
    a = _module(amd, cfg, 0.3, params).eval()
    b = _module(amd, cfg, 0.0, params).eval()
    ra, rb = _run_module(a, img, goal, wout), _run_module(b, img, goal, wout)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1])
    for k in ra[2]:
        assert torch.equal(ra[2][k], rb[2][k]), k
    # train mode, dropout = 0: the new entry points with layer keep 1 are the old entry points
    from dgvit_amd import functional as F_
    from dgvit_amd._lib import dgvit_config
    lib = amd.load_library()
    t = _module(amd, cfg, 0.0, params)
    tab = F_._table([None if q is None else q.detach() for q in t.param_table()])
    cfgc = dgvit_config(*t._cfg)
    B = 5
    img_d, goal_d = img.cuda(), goal.cuda()
    nws = lib.dgvit_got_workspace_floats(ctypes.byref(cfgc), B, 1)
    outs = []
    for fn in ("v1", "v2"):
        ws = torch.empty(nws, device="cuda")
        feat = torch.empty(B, cfg.dim, device="cuda")
        args = [ctypes.byref(cfgc), tab, F_._ptr(img_d), F_._ptr(goal_d), F_._ptr(feat), F_._ptr(ws), nws, B, 1, 0.9]
        if fn == "v1":
            rc = lib.dgvit_got_forward(*args, SEED, None, F_._stream())
        else:
            rc = lib.dgvit_got_forward_v2(*args, 1.0, SEED, None, F_._stream())
        assert rc == 0
        torch.cuda.synchronize()
        outs.append(feat.cpu())
    assert torch.equal(outs[0], outs[1])
    # and the module's train step at dropout = 0 equals the functional call without a layer keep (the emb-dropout path)
    r1 = _run_module(t, img, goal, wout)
    gg = goal.cuda().requires_grad_(True)
    f2 = F_.got_encoder(img.cuda(), gg, t._cfg, t.param_table(), 0.9, SEED)
    assert torch.equal(r1[0], f2.detach().cpu())


def test_layer_keep_is_checked_by_the_abi(amd):
    from dgvit_amd import functional as F_
    from dgvit_amd._lib import dgvit_config
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=1, heads=2, mlp_dim=128)
    t = _module(amd, cfg, 0.0, O.make_params(O.got_param_spec(cfg, prefix=""), 1))
    lib = amd.load_library()
    cfgc = dgvit_config(*t._cfg)
    nws = lib.dgvit_got_workspace_floats(ctypes.byref(cfgc), 1, 0)
    ws, feat = torch.empty(nws, device="cuda"), torch.empty(1, cfg.dim, device="cuda")
    img, goal = torch.rand(1, 84, 84, device="cuda"), torch.randn(1, 64, device="cuda")
    for bad in (0.0, 1.5, -0.5):
        rc = lib.dgvit_got_forward_v2(ctypes.byref(cfgc), F_._table([None if q is None else q.detach() for q in t.param_table()]),
                                      F_._ptr(img), F_._ptr(goal), F_._ptr(feat), F_._ptr(ws), nws, 1, 0, 1.0, bad, 0, None, F_._stream())
        assert rc != 0 and b"layer_dropout_keep" in lib.dgvit_last_error()


# ------------------------------------------------------------------------------------------------ (6) graph capture
def test_captured_steps_draw_fresh_masks_and_follow_the_device_seed(amd):
    from dgvit_amd import functional as F_
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 23)
    img, goal, wout = (t.cuda() for t in _inputs(cfg, 4, 23))
    m = R.build_got(amd, cfg, 0.2)
    m.load_state_dict(params, strict=True)
    m = m.cuda().train()

    # (a) the module inside a capture draws its seed on the device: two replays give different features and gradients
    def step():
        for q in m.parameters():
            q.grad = None
        f = m(img, goal)
        (f * wout).sum().backward()
        return f.detach(), m.transformer.layers[0][1].fn.net[0].weight.grad
    gs = amd.GraphedStep(step, warmup=2)
    f1, g1 = (t.clone() for t in gs())
    f2, g2 = (t.clone() for t in gs())
    torch.cuda.synchronize()
    assert not torch.equal(f1, f2) and not torch.equal(g1, g2)

    # (b) a captured forward+backward reading its seed from device memory equals the eager step with that seed
    seed_t = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab = m.param_table()

    def fb(seed):
        gg = goal.clone().requires_grad_(True)
        f = F_.got_encoder(img, gg, m._cfg, tab, 0.9, seed, layer_dropout_keep=0.8)
        gr = torch.autograd.grad((f * wout).sum(), [gg, tab[4 + 7]])
        return f.detach(), gr[0], gr[1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fb(seed_t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fb(seed_t)
    s = 0x0123_4567_89AB_CDEF
    seed_t.fill_(s)
    graph.replay()
    torch.cuda.synchronize()
    eager = fb(s)
    torch.cuda.synchronize()
    for a, b in zip(static, eager):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ (7) the bench.py size
def test_headline_training_step_with_dropout(amd):
    """B = 512 frames of 84x84 @ 12, DGViT-small (d 256, 6 layers, 8 heads, MLP 2048), dropout 0.1, one Adam step: finite; frames 0 and
    511 match the fp64 restatement with their own masks."""
    from dgvit_amd.optim import FlatAdam
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=256, depth=6, heads=8, mlp_dim=2048)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 29)
    B = 512
    img, goal, wout = _inputs(cfg, B, 29)
    m = _module(amd, cfg, 0.1, params)
    opt = FlatAdam([m], lr=1e-4)
    gg = goal.cuda().requires_grad_(True)
    feat = m(img.cuda(), gg)
    (feat * wout.cuda()).sum().backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(feat).all() and torch.isfinite(gg.grad).all()
    assert all(torch.isfinite(q).all() for q in m.parameters())
    frames = [0, B - 1]
    masks = R.all_masks(cfg, B, SEED, 0.9, 0.9, frames=frames)
    pd = {k: v.double() for k, v in params.items()}
    g2 = goal[frames].double().requires_grad_(True)
    ref = R.got_forward_masked(pd, img[frames].double(), g2, cfg, masks, keep=0.9, emb_keep=0.9)
    (ref * wout[frames].double()).sum().backward()
    np.testing.assert_allclose(feat.detach().cpu()[frames].numpy(), ref.detach().numpy(), rtol=0, atol=OUT_TOL)
    assert R.rel_err(gg.grad.cpu()[frames].numpy(), g2.grad.numpy()) < GRAD_RTOL
