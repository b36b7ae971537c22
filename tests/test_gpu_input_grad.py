"""GPU: gradients with respect to the depth frame (img.requires_grad) through the GoT encoder (fp32 and bf16) and the CNN feature stack,
against fp64 autograd through the CPU oracle.  Every test here fails without the frame gradient: img.grad stays None (or the output has
no graph at all when the model is frozen)."""
import numpy as np
import pytest
import torch

from helpers import O
import layer_dropout_ref as R

pytestmark = pytest.mark.gpu

SEED = 1234
DIMG_RTOL = 2e-3      # relative L2 error of dimg against fp64 (the tolerance class of the gradient digests)
DIMG_MAXABS = 1e-4    # max-abs error relative to max |ref|


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


def _cfg(image, patch, dim=64, depth=2, heads=4, dim_head=64, mlp_dim=128):
    return O.GoTConfig(image=image, patch=patch, dim=dim, depth=depth, heads=heads, dim_head=dim_head, mlp_dim=mlp_dim)


def _got(amd, cfg, params, pool="cls", dropout=0.0, emb_dropout=0.0, train=False, **sched):
    m = amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=2, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads,
                mlp_dim=cfg.mlp_dim, channels=1, dim_head=cfg.dim_head, pool=pool, dropout=dropout, emb_dropout=emb_dropout)
    m.load_state_dict(params, strict=True)
    m = m.cuda().train(train)
    if sched:
        m.set_schedule(**sched)
    m.draw_dropout_seed = lambda: SEED
    return m


def _inputs(cfg, B, seed=3):
    img, _, _, _ = O.make_inputs(cfg, B, seed)
    goal = torch.randn(B, cfg.dim, generator=torch.Generator().manual_seed(seed + 1))
    w = torch.randn(B, cfg.dim, generator=torch.Generator().manual_seed(seed + 2))
    return img, goal, w


def _run(m, img, goal, w, goal_grad=True):
    """(dimg, dgoal, parameter gradients) of (m(img, goal) * w).sum() with img.requires_grad"""
    x = img.cuda().requires_grad_(True)
    g = goal.cuda().requires_grad_(goal_grad)
    for q in m.parameters():
        q.grad = None
    (m(x, g) * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert x.grad is not None, "no image gradient"
    return x.grad.cpu(), (g.grad.cpu() if goal_grad else None), {k: q.grad.cpu() for k, q in m.named_parameters() if q.grad is not None}


def _ref_dimg(cfg, params, img, goal, w, pool="cls", masks=None, keep=1.0, emb_keep=1.0):
    """fp64 autograd through the oracle (the masked restatement when masks are given)"""
    pd = {k: v.double() for k, v in params.items()}
    x = img.double().requires_grad_(True)
    if masks is None:
        out = O.got_forward(pd, x, goal.double(), cfg, prefix="", pool=pool)
    else:
        out = R.got_forward_masked(pd, x, goal.double(), cfg, masks, keep=keep, emb_keep=emb_keep, pool=pool)
    (out * w.double()).sum().backward()
    return x.grad


def _check(dimg, ref):
    assert dimg.shape == ref.shape
    err = R.rel_err(dimg.numpy(), ref.numpy())
    mx = float((dimg.double() - ref).abs().max())
    assert err <= DIMG_RTOL, err
    assert mx <= DIMG_MAXABS * float(ref.abs().max()), (mx, float(ref.abs().max()))


# ------------------------------------------------------------------------------------------------ fp32 encoder: shapes
@pytest.mark.parametrize("image,patch,B,sched", [
    ((128, 160), (16, 20), 3, {}),                              # shipped shape, pw % 4 == 0: float4 image stores
    ((84, 84), (12, 12), 4, {}),
    ((84, 84), (7, 7), 3, {}),                                  # pw = 7: the element-wise store path
    ((224, 224), (14, 14), 2, {}),                              # 257 tokens, pw = 14
    ((136, 168), (8, 8), 2, {"long_sequence": True}),           # 358 tokens on the tiled attention
], ids=["shipped", "84p12", "84p7", "224p14", "long358"])
def test_got_fp32_image_gradient_shapes(amd, image, patch, B, sched):
    cfg = _cfg(image, patch)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 11)
    img, goal, w = _inputs(cfg, B)
    dimg, _, _ = _run(_got(amd, cfg, params, **sched), img, goal, w)
    _check(dimg, _ref_dimg(cfg, params, img, goal, w))


@pytest.mark.parametrize("variant", ["mean", "noproj", "dense_last", "wgrad_overlap"])
def test_got_fp32_image_gradient_schedules(amd, variant):
    cfg = _cfg((84, 84), (12, 12), heads=1, dim_head=64) if variant == "noproj" else _cfg((84, 84), (12, 12))
    assert cfg.project_out == (variant != "noproj")
    pool = "mean" if variant == "mean" else "cls"
    sched = {"dense_last_block": True} if variant == "dense_last" else {"wgrad_overlap": True} if variant == "wgrad_overlap" else {}
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 12)
    img, goal, w = _inputs(cfg, 5)
    dimg, _, _ = _run(_got(amd, cfg, params, pool=pool, **sched), img, goal, w)
    _check(dimg, _ref_dimg(cfg, params, img, goal, w, pool=pool))


# ------------------------------------------------------------------------------------------------ train mode
@pytest.mark.parametrize("p", [0.0, 0.3], ids=["emb_dropout", "layer_dropout"])
def test_got_fp32_image_gradient_train_mode(amd, p):
    """emb-dropout 0.1 (and transformer dropout p): the HIP masks replayed into the fp64 restatement; dimg carries the emb mask"""
    cfg = _cfg((84, 84), (12, 12))
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 13)
    B = 4
    img, goal, w = _inputs(cfg, B)
    m = _got(amd, cfg, params, dropout=p, emb_dropout=0.1, train=True)
    dimg, _, _ = _run(m, img, goal, w)
    masks = R.all_masks(cfg, B, SEED, 1.0 - p, 0.9)
    ref = _ref_dimg(cfg, params, img, goal, w, masks=masks, keep=1.0 - p, emb_keep=0.9)
    _check(dimg, ref)
    # the masks reach the frame gradient: it differs from the eval-mode one
    m.eval()
    dimg_eval, _, _ = _run(m, img, goal, w)
    assert not torch.equal(dimg, dimg_eval)


# ------------------------------------------------------------------------------------------------ frozen model, nothing changes
def test_got_frozen_model_gives_only_the_image_gradient(amd):
    cfg = _cfg((128, 160), (16, 20))
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 14)
    img, goal, w = _inputs(cfg, 3)
    m = _got(amd, cfg, params).requires_grad_(False)
    calls = []
    m._grad_hook = lambda *a: calls.append(a)      # the gradient-ready hook (parallel.GradSync): nothing to hand it
    dimg, _, grads = _run(m, img, goal, w, goal_grad=False)
    assert not grads and all(q.grad is None for q in m.parameters())
    assert not calls
    _check(dimg, _ref_dimg(cfg, params, img, goal, w))


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_parameter_gradients_unchanged_by_the_image_gradient(amd, bf16):
    """the same backward with and without img.requires_grad: bitwise-equal parameter gradients and dgoal"""
    cfg = _cfg((84, 84), (12, 12), dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 15)
    img, goal, w = _inputs(cfg, 6)
    m = _got(amd, cfg, params, **({} if bf16 else {"wgrad_overlap": True}))
    if bf16:
        m.set_compute_dtype(torch.bfloat16)
    outs = []
    for want in (False, True):
        x = img.cuda().requires_grad_(want)
        g = goal.cuda().requires_grad_(True)
        for q in m.parameters():
            q.grad = None
        (m(x, g) * w.cuda()).sum().backward()
        torch.cuda.synchronize()
        assert (x.grad is not None) == want
        outs.append((g.grad.clone(), {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}))
    (g0, p0), (g1, p1) = outs
    assert torch.equal(g0, g1)
    assert p0.keys() == p1.keys() and len(p0) > 10
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k


def test_got_image_gradient_is_deterministic_and_frame_independent(amd):
    cfg = _cfg((128, 160), (16, 20))
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 16)
    img, goal, w = _inputs(cfg, 5)
    m = _got(amd, cfg, params)
    a, _, _ = _run(m, img, goal, w)
    b, _, _ = _run(m, img, goal, w)
    assert torch.equal(a, b)
    one, _, _ = _run(m, img[2:3], goal[2:3], w[2:3])
    assert torch.equal(one[0], a[2])


# ------------------------------------------------------------------------------------------------ bf16 configuration
@pytest.mark.parametrize("case", ["c5_l2", "odd"])
def test_got_bf16_image_gradient(amd, case):
    cfg, B = {
        "c5_l2": (O.GoTConfig(image=(224, 224), patch=(16, 16), dim=768, depth=2, heads=12, dim_head=64, mlp_dim=3072), 3),
        "odd": (O.GoTConfig(image=(40, 56), patch=(8, 8), dim=72, depth=2, heads=3, dim_head=64, mlp_dim=200), 5),
    }[case]
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 21)
    img, goal, w = _inputs(cfg, B)
    m = _got(amd, cfg, params).set_compute_dtype(torch.bfloat16)
    dimg, _, _ = _run(m, img, goal, w)
    assert dimg.dtype == torch.float32
    for fn in (O.got_forward, O.got_forward_bf16):
        x = img.clone().requires_grad_(True)
        (fn(params, x, goal, cfg, prefix="") * w).sum().backward()
        err = R.rel_err(dimg.numpy(), x.grad.numpy())
        assert err < 2e-2, (fn.__name__, err)


# ------------------------------------------------------------------------------------------------ CNN feature stack
@pytest.mark.parametrize("hw", [(128, 160), (61, 75)])
@pytest.mark.parametrize("kind", ["qnet", "policy"])
def test_cnn_image_gradient(amd, kind, hw):
    B = 3
    spec = O.cnn_qnet_param_spec() if kind == "qnet" else O.cnn_policy_param_spec()
    params = O.make_params(spec, 31)
    img, pstate, a, _ = O.make_inputs(O.GoTConfig(image=hw), B, 31)
    m = (amd.QNetwork(2, 2) if kind == "qnet" else amd.GaussianPolicy(2, 2))
    m.load_state_dict(params, strict=True)
    m = m.cuda()
    wts = [torch.randn(B, 2, generator=torch.Generator().manual_seed(s)) for s in (1, 2)]

    def loss(outs, ws):
        return sum((o * w_).sum() for o, w_ in zip(outs, ws))

    x = img.cuda().requires_grad_(True)
    ins = [x, pstate.cuda(), a.cuda()] if kind == "qnet" else [x, pstate.cuda()]
    loss(m(ins), [w_.cuda() for w_ in wts]).backward()
    pd = {k: v.double() for k, v in params.items()}
    xr = img.double().requires_grad_(True)
    outs = O.cnn_qnet_forward(pd, xr, pstate.double(), a.double()) if kind == "qnet" else O.cnn_policy_forward(pd, xr, pstate.double())
    loss(outs, [w_.double() for w_ in wts]).backward()
    assert x.grad is not None
    assert R.rel_err(x.grad.cpu().numpy(), xr.grad.numpy()) <= 1e-4


def test_cnn_frozen_network_gives_only_the_image_gradient(amd):
    B = 4
    params = O.make_params(O.cnn_qnet_param_spec(), 32)
    img, pstate, a, _ = O.make_inputs(O.GoTConfig(image=(128, 160)), B, 32)
    m = amd.QNetwork(2, 2)
    m.load_state_dict(params, strict=True)
    m = m.cuda().requires_grad_(False)
    x = img.cuda().requires_grad_(True)
    q1, _ = m([x, pstate.cuda(), a.cuda()])
    q1.sum().backward()
    assert all(q.grad is None for q in m.parameters())
    xr = img.double().requires_grad_(True)
    r1, _ = O.cnn_qnet_forward({k: v.double() for k, v in params.items()}, xr, pstate.double(), a.double())
    r1.sum().backward()
    assert R.rel_err(x.grad.cpu().numpy(), xr.grad.numpy()) <= 1e-4
    # deterministic: a second pass gives the same bits
    x2 = img.cuda().requires_grad_(True)
    m([x2, pstate.cuda(), a.cuda()])[0].sum().backward()
    assert torch.equal(x.grad, x2.grad)


# ------------------------------------------------------------------------------------------------ end to end (SAC networks)
def test_policy_sample_and_qnet_saliency_end_to_end(amd, monkeypatch):
    cfg = O.GoTConfig(image=(128, 160), patch=(16, 20), dim=64, depth=4, heads=4, mlp_dim=2048)
    B = 3
    img, pstate, act, _ = O.make_inputs(cfg, B, 41)
    noise = torch.randn(B, 2, generator=torch.Generator().manual_seed(5))
    from dgvit_amd import sac_networks
    monkeypatch.setattr(sac_networks, "_standard_normal", lambda mean: noise.to(mean.device))

    params = O.make_params(O.policy_param_spec(cfg), 41)
    pol = amd.GoTPolicy(2, 2, 4, 4, 64)
    pol.load_state_dict(params, strict=True)
    pol = pol.cuda().eval()
    x = img.cuda().requires_grad_(True)
    action, log_prob, _ = pol.sample([x, pstate.cuda()])
    (action.sum() + log_prob.sum()).backward()
    pd = {k: v.double() for k, v in params.items()}
    xr = img.double().requires_grad_(True)
    ra, rl, _ = O.policy_sample(pd, xr, pstate.double(), cfg, noise.double())
    (ra.sum() + rl.sum()).backward()
    _check(x.grad.cpu(), xr.grad)

    qparams = O.make_params(O.qnet_param_spec(cfg), 42)
    qn = amd.GoTQNetwork(2, 2, 4, 4, 64)
    qn.load_state_dict(qparams, strict=True)
    qn = qn.cuda().eval().requires_grad_(False)
    x = img.cuda().requires_grad_(True)
    q1, _ = qn([x, pstate.cuda(), act.cuda()])
    q1.sum().backward()
    xr = img.double().requires_grad_(True)
    r1, _ = O.qnet_forward({k: v.double() for k, v in qparams.items()}, xr, pstate.double(), act.double(), cfg)
    r1.sum().backward()
    _check(x.grad.cpu(), xr.grad)
