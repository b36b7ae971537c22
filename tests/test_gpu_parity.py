"""GPU: end-to-end parity of the product nn.Modules (HIP path through the C ABI) against
  (a) the golden vectors produced by the reference itself (tests/golden/*.npz), and
  (b) the CPU oracle on the same seeded inputs,
within the north-star tolerance of 1e-3 (fp32); the tests assert a 10x tighter 1e-4 on outputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O, load_fixture, fixture_cfg, got_case_inputs, check_grad_digest  # noqa: E402

OUT_TOL = 1e-4    # outputs (features are RMS-normalised, heads O(1)); north star allows 1e-3
GRAD_RTOL = 2e-3  # gradient digests (norm / sum / first 16 entries), relative to the parameter's gradient norm
GRAD_ATOL = 2e-5


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


def _load_state(module, params, strip=""):
    sd = {k[len(strip):] if strip and k.startswith(strip) else k: v for k, v in params.items()}
    module.load_state_dict(sd, strict=True)
    return module.cuda()


def _build_got(amd, cfg):
    return amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=cfg.num_classes, dim=cfg.dim, depth=cfg.depth,
                   heads=cfg.heads, mlp_dim=cfg.mlp_dim, channels=1, dim_head=cfg.dim_head)


@pytest.mark.parametrize("name", ["got_tiny_eval", "got_84p12", "got_84p14", "got_84p7", "got_84p6", "got_c5_l2"])
def test_got_golden_eval(amd, name):
    fx = load_fixture(name)
    cfg = fixture_cfg(fx)
    m = _load_state(_build_got(amd, cfg), O.make_params(O.got_param_spec(cfg, prefix=""), int(fx["meta/seed"]))).eval()
    img, goal, wout, _ = got_case_inputs(fx, cfg, False)
    goal = goal.cuda().requires_grad_(True)
    feat = m(img.cuda(), goal)
    np.testing.assert_allclose(feat.detach().cpu().numpy(), fx["feat"], rtol=0, atol=OUT_TOL)
    (feat * wout.cuda()).sum().backward()
    np.testing.assert_allclose(goal.grad.cpu().numpy(), fx["dgoal"], rtol=GRAD_RTOL, atol=1e-4)
    grads = {k: p.grad for k, p in m.named_parameters()}
    check_grad_digest(fx, "g", grads, rtol=GRAD_RTOL, atol=GRAD_ATOL)
    if "gfull/pos_embedding" in fx:
        for k, p in m.named_parameters():
            if f"gfull/{k}" in fx:
                ref = fx[f"gfull/{k}"]
                np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=GRAD_RTOL, atol=2e-5 * max(1.0, np.abs(ref).max()), err_msg=k)


@pytest.mark.parametrize("name", ["policy_native_shipped", "policy_native_small", "policy_c2"])
def test_policy_golden(amd, name):
    fx = load_fixture(name)
    cfg = fixture_cfg(fx)
    batch, seed = int(fx["meta/batch"]), int(fx["meta/seed"])
    m = amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    m = _load_state(m, O.make_params(O.policy_param_spec(cfg), seed)).eval()
    m = m.to("cuda")
    img, pstate, _, _ = O.make_inputs(cfg, batch, seed)
    mean, log_std = m([img.cuda(), pstate.cuda()])
    np.testing.assert_allclose(mean.detach().cpu().numpy(), fx["mean"], rtol=0, atol=OUT_TOL)
    np.testing.assert_allclose(log_std.detach().cpu().numpy(), fx["log_std"], rtol=0, atol=OUT_TOL)
    loss = (mean ** 2).mean() + (log_std ** 2).mean()
    np.testing.assert_allclose(loss.item(), float(fx["loss"]), rtol=1e-4)
    loss.backward()
    check_grad_digest(fx, "g", {k: p.grad for k, p in m.named_parameters()}, rtol=GRAD_RTOL, atol=GRAD_ATOL)
    # sample(): same N(0,1) stream as the reference run (torch.manual_seed + CPU generator is not what CUDA uses,
    # so inject the stored noise through the oracle formula instead and compare tanh(mean) which is noise-free)
    torch.manual_seed(seed)
    _, log_prob, tmean = m.sample([img.cuda(), pstate.cuda()])
    np.testing.assert_allclose(tmean.detach().cpu().numpy(), fx["tanh_mean"], rtol=0, atol=OUT_TOL)
    assert log_prob.shape == (batch, 1)


def test_detpolicy_golden(amd):
    fx = load_fixture("detpolicy_native_shipped")
    cfg = fixture_cfg(fx)
    batch, seed = int(fx["meta/batch"]), int(fx["meta/seed"])
    m = amd.DeterministicGoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim)
    m = _load_state(m, O.make_params(O.detpolicy_param_spec(cfg), seed)).eval().to("cuda")
    img, pstate, _, _ = O.make_inputs(cfg, batch, seed)
    mean = m([img.cuda(), pstate.cuda()])
    np.testing.assert_allclose(mean.detach().cpu().numpy(), fx["mean"], rtol=0, atol=OUT_TOL)
    (mean ** 2).mean().backward()
    check_grad_digest(fx, "g", {k: p.grad for k, p in m.named_parameters()}, rtol=GRAD_RTOL, atol=GRAD_ATOL)
    act, _, mean2 = m.sample([img.cuda(), pstate.cuda()])
    assert (act - mean2).abs().max().item() <= 0.25 + 1e-6


def test_sac_losses_golden(amd):
    """Critic loss and actor loss of DRL.py:396-410 through the HIP actor + HIP transformer critic."""
    fx = load_fixture("sac_c2")
    cfg = fixture_cfg(fx)
    batch, seed = int(fx["meta/batch"]), int(fx["meta/seed"])
    kw = dict(image_size=cfg.image, patch_size=cfg.patch)
    pol = _load_state(amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, **kw), O.make_params(O.policy_param_spec(cfg), seed)).eval().to("cuda")
    crt = _load_state(amd.GoTQNetwork(2, 2, cfg.depth, cfg.heads, cfg.dim, **kw), O.make_params(O.qnet_param_spec(cfg), seed + 1)).eval()
    img, pstate, act, tgt = (t.cuda() for t in O.make_inputs(cfg, batch, seed))
    q1, q2 = crt([img, pstate, act])
    np.testing.assert_allclose(q1.detach().cpu().numpy(), fx["q1"], rtol=0, atol=OUT_TOL)
    np.testing.assert_allclose(q2.detach().cpu().numpy(), fx["q2"], rtol=0, atol=OUT_TOL)
    qf = torch.nn.functional.mse_loss(q1, tgt.expand_as(q1)) + torch.nn.functional.mse_loss(q2, tgt.expand_as(q2))
    np.testing.assert_allclose(qf.item(), float(fx["qf_loss"]), rtol=1e-4)
    qf.backward()
    check_grad_digest(fx, "gc", {k: p.grad for k, p in crt.named_parameters()}, rtol=GRAD_RTOL, atol=GRAD_ATOL)
    crt.zero_grad()
    # actor loss with the reference's noise draw injected (rsample = mean + std * eps)
    mean, log_std = pol([img, pstate])
    eps = torch.from_numpy(fx["noise"]).cuda()
    std = log_std.exp()
    x_t = mean + std * eps
    y_t = torch.tanh(x_t)
    log_pi = (torch.distributions.Normal(mean, std).log_prob(x_t) - torch.log(1 - y_t.pow(2) + 1e-6)).sum(1, keepdim=True)
    np.testing.assert_allclose(y_t.detach().cpu().numpy(), fx["pi"], rtol=0, atol=OUT_TOL)
    q1p, q2p = crt([img, pstate, y_t])
    loss = ((0.2 * log_pi) - torch.min(q1p, q2p)).mean()
    np.testing.assert_allclose(loss.item(), float(fx["policy_loss"]), rtol=2e-4, atol=1e-5)
    loss.backward()
    check_grad_digest(fx, "ga", {k: p.grad for k, p in pol.named_parameters()}, rtol=GRAD_RTOL, atol=GRAD_ATOL)


def test_train_mode_dropout_matches_oracle_with_same_mask(amd):
    """Train-mode emb-dropout: extract the HIP Philox mask (dropout of ones with the same seed) and feed it
    to the oracle; forward and gradients must then agree (GoalFormer.py:163)."""
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2)
    B, seed = 3, 11
    params = O.make_params(O.got_param_spec(cfg, prefix=""), seed)
    m = _load_state(_build_got(amd, cfg), params).train()
    img, _, _, _ = O.make_inputs(cfg, B, seed)
    goal = torch.randn(B, cfg.dim, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(77)
    dseed = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(77)                       # module draws the same seed from the CPU generator
    gg = goal.cuda().requires_grad_(True)
    feat = m(img.cuda(), gg)
    feat.square().sum().backward()
    ones = torch.ones(B * cfg.tokens * cfg.dim, device="cuda")
    amd.functional.op_dropout_(ones, dseed, 0.9)
    mask = (ones != 0).float().reshape(B, cfg.tokens, cfg.dim).cpu()
    assert 0.85 < mask.mean().item() < 0.95
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    go = goal.clone().requires_grad_(True)
    ref = O.got_forward(p, img, go, cfg, drop_mask=mask, prefix="")
    ref.square().sum().backward()
    np.testing.assert_allclose(feat.detach().cpu().numpy(), ref.detach().numpy(), rtol=0, atol=OUT_TOL)
    np.testing.assert_allclose(gg.grad.cpu().numpy(), go.grad.numpy(), rtol=GRAD_RTOL, atol=1e-4)
    for k, prm in m.named_parameters():
        if prm.grad is not None:
            r = p[k].grad.numpy()
            np.testing.assert_allclose(prm.grad.cpu().numpy(), r, rtol=GRAD_RTOL, atol=3e-5 * max(1.0, np.abs(r).max()), err_msg=k)
    # two train-mode forwards differ (mask is live), eval-mode forwards are deterministic
    f2 = m(img.cuda(), goal.cuda())
    assert (f2 - feat).abs().max().item() > 1e-3
    m.eval()
    assert torch.equal(m(img.cuda(), goal.cuda()), m(img.cuda(), goal.cuda()))


@pytest.mark.parametrize("B", [1, 5, 64])
def test_batch_sizes_vs_oracle(amd, B):
    """Ragged batch sizes (B*N not a multiple of any tile) at the C2 model shape, against the oracle."""
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=256, depth=2, heads=8)
    params = O.make_params(O.policy_param_spec(cfg), 21)
    m = _load_state(amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch), params).eval().to("cuda")
    img, pstate, _, _ = O.make_inputs(cfg, B, 21)
    mean, log_std = m([img.cuda(), pstate.cuda()])
    rm, rl = O.policy_forward(params, img, pstate, cfg)
    np.testing.assert_allclose(mean.detach().cpu().numpy(), rm.numpy(), rtol=0, atol=OUT_TOL)
    np.testing.assert_allclose(log_std.detach().cpu().numpy(), rl.numpy(), rtol=0, atol=OUT_TOL)


def test_full_size_properties(amd):
    """BASELINE full size (B=512, 84x84@12, L6/H8/D256): size-independent properties.
    (1) frames are independent: any sub-batch gives the same rows; (2) RMSNorm'd features have unit RMS
    (g = 1); (3) gradients of a mean loss over the full batch equal the mean of two half-batch gradients."""
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=256, depth=6, heads=8)
    torch.manual_seed(0)
    m = amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch).to("cuda").eval()
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, 512, 3407))
    goal = amd.functional.linear(pstate, m.fc_embed.weight, m.fc_embed.bias)
    feat = m.trans(img, goal)
    rms = feat.square().mean(1).sqrt()
    np.testing.assert_allclose(rms.detach().cpu().numpy(), 1.0, atol=1e-4)
    sub = m.trans(img[100:133], goal[100:133])
    np.testing.assert_allclose(sub.detach().cpu().numpy(), feat[100:133].detach().cpu().numpy(), rtol=0, atol=2e-5)
    # oracle on a bounded sample of the same batch (seconds on CPU)
    params = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    ref = O.got_forward(params, img[:8].cpu(), goal[:8].detach().cpu(), cfg)
    np.testing.assert_allclose(feat[:8].detach().cpu().numpy(), ref.numpy(), rtol=0, atol=OUT_TOL)

    def grads(sl):
        m.zero_grad()
        mean, log_std = m([img[sl], pstate[sl]])
        ((mean ** 2).mean() + (log_std ** 2).mean()).backward()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    gf, ga, gb = grads(slice(0, 512)), grads(slice(0, 256)), grads(slice(256, 512))
    for k in gf:
        avg = 0.5 * (ga[k] + gb[k])
        scale = max(gf[k].abs().max().item(), 1e-6)
        assert (gf[k] - avg).abs().max().item() <= 2e-3 * scale + 1e-7, k


def test_last_block_token0_schedule_equals_dense(amd):
    """The last block computes Q / attention / to_out / feed-forward for token 0 only (GoalFormer.py:167 reads
    x[:, 0]); outputs and every gradient must equal the dense schedule (DGVIT_FLAG_DENSE_LAST_BLOCK, GoT.set_schedule)."""
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=256, depth=3, heads=8)
    params = O.make_params(O.policy_param_spec(cfg), 31)
    m = _load_state(amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch), params).eval().to("cuda")
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, 37, 31))

    def run():
        m.zero_grad()
        mean, log_std = m([img, pstate])
        ((mean ** 2).mean() + (log_std ** 2).mean()).backward()
        return mean.detach().clone(), log_std.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    m.trans.set_schedule(dense_last_block=True)
    md, ld, gd = run()
    m.trans.set_schedule(dense_last_block=False)
    mp_, lp_, gp_ = run()
    np.testing.assert_allclose(mp_.cpu().numpy(), md.cpu().numpy(), rtol=0, atol=2e-6)
    np.testing.assert_allclose(lp_.cpu().numpy(), ld.cpu().numpy(), rtol=0, atol=2e-6)
    assert gd.keys() == gp_.keys()
    for k in gd:
        scale = max(gd[k].abs().max().item(), 1e-8)
        assert (gd[k] - gp_[k]).abs().max().item() <= 2e-4 * scale + 1e-9, k


def test_wgrad_helper_stream_equals_single_stream(amd):
    """Opt-in overlap of weight-gradient GEMMs on the helper stream must not change any gradient (ordering is
    event based); run twice to exercise event-ring reuse."""
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=256, depth=3, heads=8)
    m = _load_state(amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch),
                    O.make_params(O.policy_param_spec(cfg), 41)).eval().to("cuda")
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, 96, 41))

    def run():
        m.zero_grad()
        mean, log_std = m([img, pstate])
        ((mean ** 2).mean() + (log_std ** 2).mean()).backward()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    ref = run()
    m.trans.set_schedule(wgrad_overlap=True)
    for _ in range(3):
        got = run()
        for k in ref:
            assert torch.equal(ref[k], got[k]), k   # same kernels, same order of summation: bit identical


def test_flat_adam_matches_torch_adam(amd):
    """dgvit_adam_step over flat buffers == torch.optim.Adam (DRL.py:126-168 uses it) for three steps, including the
    zero-copy pickup of the fused backward's flat gradient buffer and parameters without gradients."""
    import copy
    from dgvit_amd.optim import FlatAdam
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2)
    params = O.make_params(O.policy_param_spec(cfg), 51)
    kw = dict(image_size=cfg.image, patch_size=cfg.patch)
    a = _load_state(amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, **kw), params).eval().to("cuda")
    b = copy.deepcopy(a)
    oa = FlatAdam([a], lr=3e-3, weight_decay=0.01)
    ob = torch.optim.Adam(b.parameters(), lr=3e-3, weight_decay=0.01)
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, 16, 51))
    for it in range(3):
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad(set_to_none=True)
            mean, log_std = m([img, pstate])
            ((mean ** 2).mean() + (log_std ** 2).mean() * (it + 1)).backward()
            o.step()
    from dgvit_amd.optim import home_of
    home = home_of(a)
    enc = sum((p.numel() + 3) & ~3 for p in a.trans.param_table())
    assert home.zero_copy_elems == 3 * enc, "encoder gradients should have been consumed in place (zero copy) on every step"
    assert home.copied_elems < 3 * 40000, "only the head gradients are gathered"
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), rtol=2e-5, atol=2e-6, err_msg=k)
    assert torch.equal(a.trans.cls_token, b.trans.cls_token)     # never gets a gradient: untouched by both


def test_soft_update_flat(amd):
    from dgvit_amd.optim import flatten_parameters, soft_update
    torch.manual_seed(0)
    src = amd.GoTQNetwork(2, 2, 1, 2, 64).to("cuda")
    tgt = amd.GoTQNetwork(2, 2, 1, 2, 64).to("cuda")
    want = [t.detach().clone() * (1 - 0.005) + s.detach() * 0.005 for t, s in zip(tgt.parameters(), src.parameters())]
    flatten_parameters(src)
    flatten_parameters(tgt)
    soft_update(tgt, src, 0.005)
    for w, t in zip(want, tgt.parameters()):
        np.testing.assert_allclose(t.detach().cpu().numpy(), w.cpu().numpy(), rtol=1e-6, atol=1e-7)
    q1, _ = tgt([torch.rand(2, 128, 160, device="cuda"), torch.rand(2, 2, device="cuda"), torch.rand(2, 2, device="cuda")])
    assert torch.isfinite(q1).all()                     # the re-homed parameters still drive the HIP forward


def test_large_batch_indexing(amd):
    """B = 2048 frames (T = 102 400 token rows).  The largest single operand is the fc1 output, 102 400 x 2048 floats = 838 860 800
    bytes: no one buffer reaches 2^31 bytes here (the two layers' activations together do), so this test does not cross any of
    the size boundaries of DESIGN 3.21.
    Frame independence: rows of the big batch equal the same frames run as a small batch."""
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=256, depth=2, heads=8)
    torch.manual_seed(3)
    m = amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch).to("cuda").eval()
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, 2048, 9))
    mean, log_std = m([img, pstate])
    ((mean ** 2).mean() + (log_std ** 2).mean()).backward()
    g_big = m.trans.transformer.layers[1][1].fn.net[0].weight.grad.clone()
    assert torch.isfinite(g_big).all() and torch.isfinite(mean).all()
    with torch.no_grad():
        ms, _ = m([img[2040:2048], pstate[2040:2048]])
    np.testing.assert_allclose(ms.cpu().numpy(), mean[2040:2048].detach().cpu().numpy(), rtol=0, atol=2e-5)
    # gradient of the mean loss over 2048 frames == mean of the gradients of its four 512-frame quarters
    acc = torch.zeros_like(g_big)
    for q in range(4):
        m.zero_grad()
        a, b = m([img[q * 512:(q + 1) * 512], pstate[q * 512:(q + 1) * 512]])
        ((a ** 2).mean() + (b ** 2).mean()).backward()
        acc += m.trans.transformer.layers[1][1].fn.net[0].weight.grad / 4
    assert (acc - g_big).abs().max().item() <= 2e-3 * g_big.abs().max().item() + 1e-8


def test_choose_action_and_sample(amd):
    """GoTPolicy.choose_action (got_sac_network.py:205-220): numpy (H, W, 1) frame + (2,) goal -> numpy (2,) action."""
    cfg = O.GoTConfig(dim=64, depth=4, heads=4)
    params = O.make_params(O.policy_param_spec(cfg), 3407)
    m = _load_state(amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim), params).eval().to("cuda")
    img, pstate, _, _ = O.make_inputs(cfg, 1, 3407)
    frame = img[0].numpy()[:, :, None]                     # (128, 160, 1) as env_lab hands it over
    act_eval = m.choose_action(frame, pstate[0].numpy(), evaluate=True)
    rm, _ = O.policy_forward(params, img, pstate, cfg)
    assert act_eval.shape == (2,)
    np.testing.assert_allclose(act_eval, torch.tanh(rm)[0].numpy(), rtol=0, atol=OUT_TOL)
    act = m.choose_action(frame, pstate[0].numpy(), evaluate=False)
    assert act.shape == (2,) and np.all(np.abs(act) <= 1.0)
    a, logp, mean = m.sample([img.cuda(), pstate.cuda()])
    assert a.shape == (1, 2) and logp.shape == (1, 1) and torch.isfinite(logp).all()


def test_c_abi_error_codes(amd):
    """Workspace too small / null pointers / bad config come back as negative codes with a message, no crash."""
    import ctypes
    from dgvit_amd._lib import dgvit_config
    lib = amd.load_library()
    cfg = dgvit_config(84, 84, 12, 12, 64, 1, 2, 64, 2048)
    n = lib.dgvit_got_workspace_floats(ctypes.byref(cfg), 2, 1)
    ws = torch.empty(n, device="cuda")
    img, goal, feat = torch.rand(2, 84, 84, device="cuda"), torch.rand(2, 64, device="cuda"), torch.empty(2, 64, device="cuda")
    m = amd.GoT(image_size=(84, 84), patch_size=(12, 12), num_classes=2, dim=64, depth=1, heads=2, mlp_dim=2048).to("cuda")
    tbl = (ctypes.c_void_p * 15)(*[p.data_ptr() for p in m.param_table()])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.dgvit_got_forward(ctypes.byref(cfg), tbl, P(img), P(goal), P(feat), P(ws), n - 1, 2, 1, 1.0, 0, None, st) == -4
    assert b"workspace" in lib.dgvit_last_error()
    assert lib.dgvit_got_forward(ctypes.byref(cfg), tbl, None, P(goal), P(feat), P(ws), n, 2, 1, 1.0, 0, None, st) == -1
    assert lib.dgvit_got_forward(ctypes.byref(cfg), tbl, P(img), P(goal), P(feat), P(ws), n, 2, 1, 1.5, 0, None, st) == -1
    assert lib.dgvit_got_forward(ctypes.byref(cfg), tbl, P(img), P(goal), P(feat), P(ws), n, 2, 1, 1.0, 0, None, st) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(feat).all()
    with pytest.raises(amd.DgvitError, match="img must be"):
        m(torch.rand(2, 80, 84, device="cuda"), goal)
    with pytest.raises(amd.DgvitError, match="fp32"):
        m(img.double(), goal)


@pytest.mark.parametrize("name,kind", [("cnn_qnet_native", "qnet"), ("cnn_qnet_84", "qnet"), ("cnn_policy_native", "policy")])
def test_cnn_networks_golden(amd, name, kind):
    """HIP QNetwork (the shipped critic) / GaussianPolicy vs the reference's own outputs and gradients."""
    fx = load_fixture(name)
    image = tuple(int(v) for v in fx["meta/image"])
    batch, seed = int(fx["meta/batch"]), int(fx["meta/seed"])
    spec = O.cnn_qnet_param_spec() if kind == "qnet" else O.cnn_policy_param_spec()
    m = amd.QNetwork(2, 2) if kind == "qnet" else amd.GaussianPolicy(2, 2)
    assert [k for k, _ in m.named_parameters()] == [k for k, _, _ in spec]
    m = _load_state(m, O.make_params(spec, seed)).to("cuda")
    img, pstate, act, tgt = (t.cuda() for t in O.make_inputs(O.GoTConfig(image=image), batch, seed))
    if kind == "qnet":
        q1, q2 = m([img, pstate, act])
        np.testing.assert_allclose(q1.detach().cpu().numpy(), fx["q1"], rtol=0, atol=OUT_TOL)
        np.testing.assert_allclose(q2.detach().cpu().numpy(), fx["q2"], rtol=0, atol=OUT_TOL)
        loss = torch.nn.functional.mse_loss(q1, tgt.expand_as(q1)) + torch.nn.functional.mse_loss(q2, tgt.expand_as(q2))
    else:
        mean, log_std = m([img, pstate])
        np.testing.assert_allclose(mean.detach().cpu().numpy(), fx["mean"], rtol=0, atol=OUT_TOL)
        np.testing.assert_allclose(log_std.detach().cpu().numpy(), fx["log_std"], rtol=0, atol=OUT_TOL)
        loss = (mean ** 2).mean() + (log_std ** 2).mean()
    np.testing.assert_allclose(loss.item(), float(fx["loss"]), rtol=1e-4)
    loss.backward()
    check_grad_digest(fx, "g", {k: p.grad for k, p in m.named_parameters()}, rtol=GRAD_RTOL, atol=GRAD_ATOL)


def test_cnn_stack_vs_oracle_batch(amd):
    """Conv stack alone at a ragged batch against the oracle (F.conv2d on CPU), outputs and all conv gradients."""
    B = 37
    spec = O.cnn_qnet_param_spec()
    params = O.make_params(spec, 5)
    img, _, _, _ = O.make_inputs(O.GoTConfig(image=(84, 84)), B, 5)
    w = torch.randn(B, 256, generator=torch.Generator().manual_seed(2))
    p = {k: v.clone().requires_grad_(True) for k, v in params.items() if k.startswith("conv")}
    ref = O.cnn_features(p, img)
    (ref * w).sum().backward()
    names = ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "conv3.weight", "conv3.bias"]
    dev = [params[k].cuda().requires_grad_(True) for k in names]
    feat = amd.functional.cnn_features(img.cuda(), dev)
    (feat * w.cuda()).sum().backward()
    np.testing.assert_allclose(feat.detach().cpu().numpy(), ref.detach().numpy(), rtol=0, atol=2e-5)
    for k, t in zip(names, dev):
        r = p[k].grad.numpy()
        np.testing.assert_allclose(t.grad.cpu().numpy(), r, rtol=2e-3, atol=2e-5 * max(1.0, np.abs(r).max()), err_msg=k)


def test_device_replay_buffer(amd):
    """device-resident replay; sampled rows must be the stored transitions at the drawn indices,
    the ring must wrap, and the index draw must be uniform over the stored range."""
    from dgvit_amd.replay import DeviceReplayBuffer
    rb = DeviceReplayBuffer(32, obs_shape=(12, 10), seed=0)
    rs = np.random.RandomState(0)
    data = []
    for i in range(45):                                     # wraps the 32-slot ring
        tr = dict(obs=rs.rand(12, 10).astype(np.float32), pobs=rs.rand(2), act=rs.rand(2) * 2 - 1, rew=float(i),
                  next_obs=rs.rand(12, 10).astype(np.float32), next_pobs=rs.rand(2), done=float(i % 2))
        rb.add(**tr)
        data.append(tr)
    assert rb.get_stored_size() == 32
    batch = rb.sample(64)
    idx = batch["indexes"].cpu().numpy()
    assert batch["obs"].shape == (64, 12, 10) and batch["pobs"].shape == (64, 2) and batch["rew"].shape == (64, 1)
    assert batch["obs"].is_cuda
    for j, slot in enumerate(idx):
        src = data[slot if slot >= 45 - 32 else slot + 32]  # slot s holds transition s or s+32 after the wrap
        np.testing.assert_array_equal(batch["obs"][j].cpu().numpy(), src["obs"])
        np.testing.assert_array_equal(batch["next_obs"][j].cpu().numpy(), src["next_obs"])
        np.testing.assert_allclose(batch["act"][j].cpu().numpy(), src["act"].astype(np.float32))
        assert batch["rew"][j].item() == src["rew"] and batch["done"][j].item() == src["done"]
    counts = np.bincount(rb.sample_indices(64000).cpu().numpy(), minlength=32)
    assert counts.min() > 1700 and counts.max() < 2300     # uniform: 2000 +- 5 sigma(=44)
    # sampled frames feed the encoder directly
    m = amd.GoTPolicy(2, 2, 1, 2, 64, image_size=(12, 10), patch_size=(6, 5)).to("cuda").eval()
    mean, _ = m([batch["obs"], batch["pobs"]])
    assert torch.isfinite(mean).all()


def test_graphed_training_step(amd):
    """A whole step (encoder+heads fwd, bwd, FlatAdam capturable, soft update) recorded into a HIP graph must
    (a) reproduce eager training exactly in eval mode, (b) draw a fresh dropout mask on every replay in train mode."""
    import copy
    from dgvit_amd.optim import FlatAdam, flatten_parameters, soft_update
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2)
    kw = dict(image_size=cfg.image, patch_size=cfg.patch)
    base = _load_state(amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, **kw), O.make_params(O.policy_param_spec(cfg), 61)).to("cuda").eval()
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, 8, 61))

    def make(model):
        tgt = copy.deepcopy(model)
        flatten_parameters(tgt)
        opt = FlatAdam([model], lr=1e-3, capturable=True)

        def step():
            opt.zero_grad(set_to_none=True)
            mean, log_std = model([img, pstate])
            loss = (mean ** 2).mean() + (log_std ** 2).mean()
            loss.backward()
            opt.step()
            return loss.detach()
        return step, opt

    ma, mb = copy.deepcopy(base), copy.deepcopy(base)
    step_a, _ = make(ma)
    step_b, _ = make(mb)
    # 3 warm-up steps happen inside GraphedStep; run the same 3 eagerly on the other copy, then 4 more on both
    g = amd.GraphedStep(step_b, warmup=3)
    for _ in range(3 + 1):            # warm-up + the capture pass itself does not execute kernels
        pass
    for _ in range(3):
        step_a()
    for _ in range(4):
        la = step_a()
        lb = g()
    torch.cuda.synchronize()
    assert abs(la.item() - lb.item()) <= 1e-6 * max(1.0, abs(la.item()))
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=k)
    # train mode: the captured forward must not freeze the dropout mask
    mc = copy.deepcopy(base).train()
    out = {}

    def fwd():
        with torch.no_grad():
            out["m"], _ = mc([img, pstate])
        return out["m"]
    gf = amd.GraphedStep(fwd, warmup=2)
    a = gf().clone()
    b = gf().clone()
    assert (a - b).abs().max().item() > 1e-4, "dropout mask frozen into the graph"


def _random_cfgs():
    rs = np.random.RandomState(1234)
    out = []
    for i in range(14):
        ph, pw = int(rs.choice([2, 3, 4, 5, 6, 7, 8])), int(rs.choice([2, 3, 4, 5, 6, 8, 10]))
        gh, gw = int(rs.randint(1, 9)), int(rs.randint(1, 9))
        dim = int(rs.choice([4, 8, 12, 20, 36, 40, 64, 100, 132, 260]))
        heads = int(rs.choice([1, 2, 3, 5]))
        dh = int(rs.choice([32, 64]))
        if dh == 32 and gh * gw + 1 > 64:
            dh = 64
        mlp = int(rs.choice([4, 12, 36, 100, 256, 516]))
        depth = int(rs.choice([1, 2, 3]))
        batch = int(rs.choice([1, 2, 3, 7, 19]))
        out.append((O.GoTConfig(image=(gh * ph, gw * pw), patch=(ph, pw), dim=dim, depth=depth, heads=heads, dim_head=dh, mlp_dim=mlp), batch, 900 + i))
    return out


@pytest.mark.parametrize("cfg,batch,seed", _random_cfgs(), ids=lambda v: str(v) if not isinstance(v, O.GoTConfig) else f"{v.image}p{v.patch}D{v.dim}L{v.depth}H{v.heads}x{v.dim_head}M{v.mlp_dim}")
def test_random_shapes_vs_oracle(amd, cfg, batch, seed):
    """Property sweep: arbitrary image/patch grids (1..65 tokens), dims that are multiples of 4 but
    of no tile size, odd head counts and MLP widths, tiny batches -- outputs and every gradient against the oracle,
    train mode with the HIP dropout mask replayed into the oracle."""
    params = O.make_params(O.got_param_spec(cfg, prefix=""), seed)
    m = _load_state(_build_got(amd, cfg), params).train()
    img, _, _, _ = O.make_inputs(cfg, batch, seed)
    rs = np.random.RandomState(seed)
    goal = torch.from_numpy(rs.standard_normal((batch, cfg.dim))).float()
    wout = torch.from_numpy(rs.standard_normal((batch, cfg.dim))).float()
    torch.manual_seed(seed)
    dseed = int(torch.randint(0, 2 ** 62, (1,)).item())
    torch.manual_seed(seed)
    gg = goal.cuda().requires_grad_(True)
    feat = m(img.cuda(), gg)
    (feat * wout.cuda()).sum().backward()
    ones = torch.ones(batch * cfg.tokens * cfg.dim, device="cuda")
    amd.functional.op_dropout_(ones, dseed, 0.9)
    mask = (ones != 0).float().reshape(batch, cfg.tokens, cfg.dim).cpu()
    p = {k: v.clone().double().requires_grad_(True) for k, v in params.items()}
    go = goal.clone().double().requires_grad_(True)
    ref = O.got_forward(p, img.double(), go, cfg, drop_mask=mask.double(), prefix="")
    (ref * wout.double()).sum().backward()
    np.testing.assert_allclose(feat.detach().cpu().numpy(), ref.detach().numpy(), rtol=0, atol=2e-4)
    np.testing.assert_allclose(gg.grad.cpu().numpy(), go.grad.numpy(), rtol=3e-3, atol=3e-4 * max(1.0, go.grad.abs().max().item()))
    for k, prm in m.named_parameters():
        if prm.grad is None:
            assert p[k].grad is None, k
            continue
        r = p[k].grad.numpy()
        np.testing.assert_allclose(prm.grad.cpu().numpy(), r, rtol=3e-3, atol=3e-4 * max(1.0, np.abs(r).max()), err_msg=k)


def test_got_meanpool_golden(amd):
    """GoT(pool='mean') through the HIP path vs the reference (dense last block, token-mean, broadcast gradient)."""
    fx = load_fixture("got_tiny_meanpool")
    cfg = fixture_cfg(fx)
    m = amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=2, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads,
                mlp_dim=cfg.mlp_dim, channels=1, dim_head=cfg.dim_head, pool='mean')
    m = _load_state(m, O.make_params(O.got_param_spec(cfg, prefix=""), int(fx["meta/seed"]))).eval()
    img, goal, wout, _ = got_case_inputs(fx, cfg, False)
    goal = goal.cuda().requires_grad_(True)
    feat = m(img.cuda(), goal)
    np.testing.assert_allclose(feat.detach().cpu().numpy(), fx["feat"], rtol=0, atol=OUT_TOL)
    (feat * wout.cuda()).sum().backward()
    np.testing.assert_allclose(goal.grad.cpu().numpy(), fx["dgoal"], rtol=GRAD_RTOL, atol=1e-4)
    for k, p in m.named_parameters():
        if f"gfull/{k}" in fx:
            ref = fx[f"gfull/{k}"]
            np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=GRAD_RTOL, atol=2e-5 * max(1.0, np.abs(ref).max()), err_msg=k)


def test_empty_batch_like_reference(amd):
    """Zero frames.  The reference's GoTPolicy returns (0, 2) tensors and, after backward, zero gradients for every parameter on
    the path (None for cls_token / mlp_head); its GoTQNetwork raises RuntimeError (view(0, -1), got_sac_network.py:113).  Both
    checked by running the reference here; the HIP path must not launch on an empty problem and must behave the same."""
    m = amd.GoTPolicy(2, 2, 2, 2, 64).cuda().train()
    mean, log_std = m([torch.zeros(0, 128, 160, device="cuda"), torch.zeros(0, 2, device="cuda")])
    assert mean.shape == (0, 2) and log_std.shape == (0, 2)
    (mean.sum() + log_std.sum()).backward()
    none = sorted(k for k, p in m.named_parameters() if p.grad is None)
    assert none == sorted(["trans.cls_token", "trans.mlp_head.0.weight", "trans.mlp_head.0.bias", "trans.mlp_head.1.weight",
                           "trans.mlp_head.1.bias"])
    assert all(float(p.grad.abs().sum()) == 0.0 and p.grad.shape == p.shape for p in m.parameters() if p.grad is not None)
    a, lp, mu = m.sample([torch.zeros(0, 128, 160, device="cuda"), torch.zeros(0, 2, device="cuda")])
    assert a.shape == (0, 2) and lp.shape == (0, 1) and mu.shape == (0, 2)
    got = amd.GoT(image_size=(84, 84), patch_size=(12, 12), num_classes=2, dim=64, depth=1, heads=2, mlp_dim=64, channels=1).cuda()
    assert got(torch.zeros(0, 84, 84, device="cuda"), torch.zeros(0, 64, device="cuda")).shape == (0, 64)
    assert got.set_compute_dtype(torch.bfloat16)(torch.zeros(0, 84, 84, device="cuda"), torch.zeros(0, 64, device="cuda")).shape == (0, 64)
    q = amd.GoTQNetwork(2, 2, 2, 2, 64).cuda()
    with pytest.raises(RuntimeError):
        q([torch.zeros(0, 128, 160, device="cuda"), torch.zeros(0, 2, device="cuda"), torch.zeros(0, 2, device="cuda")])
    with pytest.raises(amd.DgvitError):          # still no CPU fallback, empty or not
        m([torch.zeros(0, 128, 160), torch.zeros(0, 2)])


def test_training_trajectory_matches_oracle(amd):
    """Drop-in training: four Adam steps of the actor (HIP forward + backward through the C ABI + the flat-buffer HIP Adam) against
    the oracle trained with torch.optim.Adam on the CPU from the same weights, inputs and targets (eval mode: no dropout draw).
    Losses agree step by step; parameters agree after the last step except where Adam's sign-like first updates amplify a
    rounding-level gradient difference (a handful of elements whose gradient is ~0)."""
    from dgvit_amd.optim import FlatAdam
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2)
    params = O.make_params(O.policy_param_spec(cfg), 77)
    m = _load_state(amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch), params).eval().to("cuda")
    opt = FlatAdam([m], lr=1e-3)
    ref = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ropt = torch.optim.Adam(list(ref.values()), lr=1e-3)
    img, pstate, _, _ = O.make_inputs(cfg, 16, 77)
    g = torch.Generator().manual_seed(77)
    tm, tl = torch.randn(16, 2, generator=g), torch.randn(16, 2, generator=g)
    losses = []
    for _ in range(4):
        ropt.zero_grad()
        rm, rl = O.policy_forward(ref, img, pstate, cfg)
        rloss = ((rm - tm) ** 2).mean() + ((rl - tl) ** 2).mean()
        rloss.backward()
        ropt.step()
        for p in m.parameters():
            p.grad = None
        mean, log_std = m([img.cuda(), pstate.cuda()])
        loss = ((mean - tm.cuda()) ** 2).mean() + ((log_std - tl.cuda()) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append((loss.item(), rloss.item()))
    for got, want in losses:
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), losses
    assert losses[-1][0] < losses[0][0]
    total = bad = 0
    for k, p in m.state_dict().items():
        d = (p.detach().cpu() - ref[k].detach()).abs()
        total += d.numel()
        bad += int((d > 1e-4).sum())
    assert bad <= max(8, total // 2000), (bad, total)
