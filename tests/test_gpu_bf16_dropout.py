"""GPU: transformer-internal dropout of the bf16 encoder (GoT(dropout=p) under set_schedule(dropout_bf16=True)), forward and backward.

The masks come from the host restatement of tests/layer_dropout_ref.py (Philox4x32-10 + the site table of include/dgvit_hip.h) --
the one the fp32 tests use: a bf16 and an fp32 model draw the same masks from one seed.  The mask tests (1 - 3) are exact: inputs
are chosen so that an output element is non-zero exactly where one mask element is 1.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O  # noqa: E402
import layer_dropout_ref as R  # noqa: E402

SEED = 0x2545F4914F6CDD1D
DH = 64
# the project's bf16 bounds (tests/test_gpu_bf16.py): features against an fp32-parameter reference, relative L2 per gradient tensor
FEAT_MAX, FEAT_MEAN, GRAD_REL = 3e-2, 6e-3, 2e-2


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


@pytest.fixture(scope="module")
def F(amd):
    return amd.functional


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def rb(t):
    return t.float().to(torch.bfloat16).double()


def dbf(t):
    return t.float().to(torch.bfloat16).cuda()


def _bf16(x):
    return float(torch.tensor(x, dtype=torch.float32).to(torch.bfloat16))


# ------------------------------------------------------------------------------------------------ (1) the row kernel, exact
@pytest.mark.parametrize("site,layer,B,N,W", [(R.SITE_OUT, 0, 3, 50, 64), (R.SITE_FF, 5, 2, 7, 72), (R.SITE_HIDDEN, 3, 2, 50, 200)])
def test_row_kernel_draws_the_restated_mask(F, site, layer, B, N, W):
    keep = 0.7
    m = R.mask(site, layer, (B, N, W), SEED, keep)
    want = (m * _bf16(1.0 / keep)).float()
    # in place, dense rows
    x = torch.ones(B, N, W, dtype=torch.bfloat16, device="cuda")
    assert F.op_drop_rows_bf16(x, keep, SEED, layer, site) is x
    assert torch.equal(x.float().cpu(), want)
    # B buffer rows that are the absolute rows b * N (the token-0 rows of the pruned last block)
    t0 = F.op_drop_rows_bf16(torch.ones(B, W, dtype=torch.bfloat16, device="cuda"), keep, SEED, layer, site, rs=N)
    assert torch.equal(t0.float().cpu(), want[:, 0])
    # into a destination whose rows are further apart than they are wide; the source and the gap stay as they are
    src = torch.ones(B * N, W, dtype=torch.bfloat16, device="cuda")
    buf = torch.full((B * N, W + 16), 3.0, dtype=torch.bfloat16, device="cuda")
    F.op_drop_rows_bf16(src, keep, SEED, layer, site, out=buf[:, :W])
    assert torch.equal(buf[:, :W].float().cpu(), want.reshape(B * N, W))
    assert bool((buf[:, W:] == 3.0).all()) and bool((src == 1.0).all())
    # the seed read from device memory gives the same bits
    sd = torch.tensor([SEED], dtype=torch.int64, device="cuda")
    assert torch.equal(F.op_drop_rows_bf16(torch.ones(B, N, W, dtype=torch.bfloat16, device="cuda"), keep, sd, layer, site), x)


# ------------------------------------------------------------------------------------------------ (2), (3) attention masks, exact
_MASK_SHAPES = [(2, 3, 2), (3, 50, 2), (2, 65, 3), (2, 129, 2), (1, 321, 2)]


@pytest.fixture(scope="module")
def attn_masks():
    """(B, N, H) -> the site-0 mask of layer 1 at keep 0.7, (B, H, N, N) bool: computed once for the forward and the backward test"""
    return {s: R.mask(R.SITE_ATTN, 1, (s[0], s[2], s[1], s[1]), SEED, 0.7).bool() for s in _MASK_SHAPES}


def _unit_rows(B, N, H, block):
    """(B, N, H*64) bf16: row r of 64-row block `block` is e_{r mod 64} in every head, every other row is zero"""
    x = torch.zeros(B, N, H, DH)
    r = torch.arange(block * 64, min(N, block * 64 + 64))
    x[:, r, :, r - block * 64] = 1.0
    return x.reshape(B, N, H * DH).to(torch.bfloat16).cuda()


@pytest.mark.parametrize("B,N,H", _MASK_SHAPES)
def test_forward_applies_the_restated_mask(F, attn_masks, B, N, H):
    """q = k = 0: uniform probabilities.  V[k] = e_{k mod 64} on one 64-key block: out[q, j] = mask[q, k0 + j] / (keep N)."""
    keep, layer, I = 0.7, 1, H * DH
    want = attn_masks[(B, N, H)]
    nqs = (N, 1) if N in (50, 321) else (N,)
    ref_lse = None
    for blk in range((N + 63) // 64):
        qkv = torch.zeros(B, N, 3 * I, dtype=torch.bfloat16, device="cuda")
        qkv[..., 2 * I:] = _unit_rows(B, N, H, blk)
        _, lse1 = F.op_attention_bf16_tiled(qkv, H, want_lse=True)
        for nq in nqs:
            out = torch.zeros(B, N, I, dtype=torch.bfloat16, device="cuda")
            lse = torch.full((B, H, N), -7.0, device="cuda")
            F.op_attention_bf16_tiled_drop(qkv, H, keep, SEED, layer, nq=nq, out=out, lse=lse)
            got = (out.float().cpu().reshape(B, N, H, DH) != 0).permute(0, 2, 1, 3)          # (b, h, q, j)
            nk = min(64, N - blk * 64)
            assert torch.equal(got[:, :, :nq, :nk], want[:, :, :nq, blk * 64:blk * 64 + nk]), (blk, nq)
            assert not bool(got[:, :, :, nk:].any()) and not bool(got[:, :, nq:].any())
            assert torch.equal(lse[:, :, :nq], lse1[:, :, :nq]), "lse is the undropped softmax's, bit for bit"
            assert bool((lse[:, :, nq:] == -7.0).all())
        ref_lse = lse1
    assert torch.allclose(ref_lse.cpu(), torch.full((B, H, N), math.log2(N)), atol=1e-5)


@pytest.mark.parametrize("B,N,H", _MASK_SHAPES)
def test_dkv_kernel_applies_the_restated_mask(F, attn_masks, B, N, H):
    """q = k = v = 0, dO[q] = e_{q mod 64} on one 64-query block: dV[k, j] = mask[q0 + j, k] / (keep N); dQ = dK = 0."""
    keep, layer, I = 0.7, 1, H * DH
    want = attn_masks[(B, N, H)]
    qkv = torch.zeros(B, N, 3 * I, dtype=torch.bfloat16, device="cuda")
    out, lse = F.op_attention_bf16_tiled_drop(qkv, H, keep, SEED, layer, want_lse=True)
    assert not bool(out.any())
    for blk in range((N + 63) // 64):
        dqkv = F.op_attention_bwd_bf16_tiled_drop(qkv, out, _unit_rows(B, N, H, blk), lse, H, keep, SEED, layer)
        dv = (dqkv[..., 2 * I:].float().cpu().reshape(B, N, H, DH) != 0).permute(0, 2, 3, 1)      # (b, h, j, k)
        nq = min(64, N - blk * 64)
        assert torch.equal(dv[:, :, :nq], want[:, :, blk * 64:blk * 64 + nq, :]), blk
        assert not bool(dv[:, :, nq:].any()) and not bool(dqkv[..., :2 * I].any())


# ------------------------------------------------------------------------------------------------ (4) random inputs against fp64
def _attention_ref(qkv, dout, mask, keep, H):
    B, N, _ = qkv.shape
    I = H * DH
    q, k, v = (qkv[..., j * I:(j + 1) * I].reshape(B, N, H, DH).permute(0, 2, 1, 3) for j in range(3))
    dots = (q @ k.transpose(-1, -2)) * DH ** -0.5
    ref = ((torch.softmax(dots, -1) * mask / keep) @ v).permute(0, 2, 1, 3).reshape(B, N, I)
    (ref * dout).sum().backward()
    return ref.detach(), torch.logsumexp(dots.detach(), -1) / math.log(2.0)


@pytest.mark.parametrize("keep", [0.7, 0.9])
@pytest.mark.parametrize("B,N,H", [(3, 50, 2), (2, 65, 3), (1, 321, 2)])
def test_attention_forward_and_backward_on_random_inputs(F, B, N, H, keep):
    """fp64 attention with the explicit mask, from the bf16-rounded operands.  Bounds: those of test_attention_bf16 and
    test_attention_bwd_bf16 in tests/test_gpu_bf16.py."""
    layer, I = 2, H * DH
    qkv = rb(rnd(B, N, 3 * I, seed=N)).requires_grad_(True)
    dout = rb(rnd(B, N, I, seed=N + 2))
    mask = R.mask(R.SITE_ATTN, layer, (B, H, N, N), SEED, keep)
    ref, ref_lse = _attention_ref(qkv, dout, mask, keep, H)
    dq = dbf(qkv.detach())
    out, lse = F.op_attention_bf16_tiled_drop(dq, H, keep, SEED, layer, want_lse=True)
    _, lse1 = F.op_attention_bf16_tiled(dq, H, want_lse=True)
    assert torch.equal(lse, lse1)
    err = (out.double().cpu() - ref).abs()
    print(f"attention drop B{B} N{N} H{H} keep {keep}: forward max err {float(err.max()):.2e}")
    np.testing.assert_allclose(out.double().cpu().numpy(), ref.numpy(), atol=6e-3, rtol=2 ** -7)
    np.testing.assert_allclose(lse.double().cpu().numpy(), ref_lse.numpy(), atol=2e-4, rtol=0)
    dqkv = F.op_attention_bwd_bf16_tiled_drop(dq, out, dbf(dout), lse, H, keep, SEED, layer).double().cpu()
    for j, name in enumerate(("dq", "dk", "dv")):
        gj, rj = dqkv[..., j * I:(j + 1) * I], qkv.grad[..., j * I:(j + 1) * I]
        print(f"  {name}: |err| {float((gj - rj).norm()):.3e} of |ref| {float(rj.norm()):.3e}")
        assert float((gj - rj).norm()) < 1.5e-2 * float(rj.norm()) + 1e-3, name
    assert torch.equal(F.op_attention_bf16_tiled_drop(dq, H, keep, SEED, layer), out), "not reproducible from launch to launch"


# ------------------------------------------------------------------------------------------------ (5) keep = 1 is the old entry
@pytest.mark.parametrize("B,N,H", [(3, 50, 2), (1, 321, 2)])
def test_keep_one_through_the_new_entries_equals_the_old_entries(F, B, N, H):
    I = H * DH
    qkv, dout = dbf(rnd(B, N, 3 * I, seed=1)), dbf(rnd(B, N, I, seed=2))
    out0, lse0 = F.op_attention_bf16_tiled(qkv, H, want_lse=True)
    out1, lse1 = F.op_attention_bf16_tiled_drop(qkv, H, 1.0, SEED, 0, want_lse=True)
    assert torch.equal(out0, out1) and torch.equal(lse0, lse1)
    d0 = F.op_attention_bwd_bf16_tiled(qkv, out0, dout, lse0, H)
    d1 = F.op_attention_bwd_bf16_tiled_drop(qkv, out0, dout, lse0, H, 1.0, SEED, 0)
    assert torch.equal(d0, d1)
    x = dbf(rnd(B * N, 72, seed=3))
    assert torch.equal(F.op_drop_rows_bf16(x.clone(), 1.0, SEED, 0, R.SITE_FF), x)


# ------------------------------------------------------------------------------------------------ encoder helpers
def _module(amd, cfg, p, params, pool="cls", seed=SEED, emb_dropout=0.1, **schedule):
    m = R.build_got(amd, cfg, p, pool=pool, emb_dropout=emb_dropout)
    m.load_state_dict(params, strict=True)
    m = m.cuda().train().set_schedule(dropout_bf16=True, **schedule).set_compute_dtype(torch.bfloat16)
    m.draw_dropout_seed = lambda: seed      # the forward's one seed, fixed
    return m


def _run_module(m, img, goal, wout):
    for q in m.parameters():
        q.grad = None
    gg = goal.cuda().requires_grad_(True)
    feat = m(img.cuda(), gg)
    (feat * wout.cuda()).sum().backward()
    torch.cuda.synchronize()
    return feat.detach().cpu(), gg.grad.cpu(), {k: q.grad.cpu() for k, q in m.named_parameters() if q.grad is not None}


def _run_reference(cfg, params, img, goal, wout, p, pool="cls", seed=SEED, emb_p=0.1):
    B = img.shape[0]
    masks = R.all_masks(cfg, B, seed, 1.0 - p, 1.0 - emb_p) if p > 0 else {R.SITE_EMB: R.mask(R.SITE_EMB, 0, (B, cfg.tokens, cfg.dim), seed, 1.0 - emb_p)}
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


def _errors(got, ref):
    """(features max abs, features mean abs, worst relative L2 of a gradient tensor and its name)"""
    feat, dgoal, grads = got
    rfeat, rgoal, rgrads = ref
    d = (feat.double() - rfeat).abs()
    errs = {"dgoal": R.rel_err(dgoal.numpy(), rgoal.numpy())}
    for k, r in rgrads.items():
        if k in grads and float(r.abs().max()) > 0:
            errs[k] = R.rel_err(grads[k].numpy(), r.numpy())
    worst = max(errs.items(), key=lambda kv: kv[1])
    return float(d.max()), float(d.mean()), worst[1], worst[0]


# ------------------------------------------------------------------------------------------------ (6) encoder parity against fp64
_C84 = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=3, heads=2, mlp_dim=128)
_CASES = {
    # name: (cfg, B, p, pool, schedule options)
    "c84_p01": (_C84, 4, 0.1, "cls", {}),
    "c84_p05": (_C84, 4, 0.5, "cls", {}),
    "pool_mean": (_C84, 4, 0.3, "mean", {}),
    "odd": (O.GoTConfig(image=(40, 56), patch=(8, 8), dim=72, depth=2, heads=3, mlp_dim=200), 5, 0.3, "cls", {}),
    "c224_n257": (O.GoTConfig(image=(224, 224), patch=(14, 14), dim=64, depth=2, heads=2, mlp_dim=128), 2, 0.2, "cls", {}),
    "long_n321": (O.GoTConfig(image=(128, 160), patch=(8, 8), dim=64, depth=2, heads=2, mlp_dim=128), 2, 0.2, "cls", {"long_sequence_bf16": True}),
    "wgrad_overlap": (_C84, 4, 0.3, "cls", {"wgrad_overlap": True}),
    "c5_l2": (O.GoTConfig(image=(224, 224), patch=(16, 16), dim=768, depth=2, heads=12, mlp_dim=3072), 3, 0.1, "cls", {}),
}


@pytest.mark.parametrize("name", list(_CASES))
def test_train_mode_matches_the_fp64_restatement_with_the_same_masks(amd, name):
    """Features, dgoal and every parameter gradient against R.got_forward_masked in fp64 with R.all_masks.  The case's errors at p = 0
    (the unchanged path: same weights, inputs and emb-dropout mask) are measured beside them and printed; DESIGN 3.33 tabulates both."""
    cfg, B, p, pool, schedule = _CASES[name]
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 11)
    img, goal, wout = _inputs(cfg, B, 11)
    e0 = _errors(_run_module(_module(amd, cfg, 0.0, params, pool=pool, **schedule), img, goal, wout),
                 _run_reference(cfg, params, img, goal, wout, 0.0, pool=pool))
    e = _errors(_run_module(_module(amd, cfg, p, params, pool=pool, **schedule), img, goal, wout),
                _run_reference(cfg, params, img, goal, wout, p, pool=pool))
    print(f"{name}: p = 0   features max {e0[0]:.2e} mean {e0[1]:.2e}, worst gradient {e0[2]:.2e} ({e0[3]})")
    print(f"{name}: p = {p} features max {e[0]:.2e} mean {e[1]:.2e}, worst gradient {e[2]:.2e} ({e[3]})")
    assert e[0] < FEAT_MAX and e[1] < FEAT_MEAN
    assert e[2] < GRAD_REL, e[3]


# ------------------------------------------------------------------------------------------------ (7) no-grad == grad-enabled
@pytest.mark.parametrize("dim,heads", [(64, 2), (128, 1)], ids=["inner>=dim", "inner<dim"])
def test_no_grad_train_mode_forward_equals_the_saving_forward_bitwise(amd, dim, heads):
    """test_no_grad_forward_equals_the_saving_forward_bitwise of tests/test_gpu_bf16.py in train mode at p = 0.25: the joint residual
    pass and the token-0 last block of the no-grad forward draw the bits of the dense, saving forward."""
    torch.manual_seed(11)
    m = amd.GoT(image_size=(48, 48), patch_size=(8, 8), num_classes=2, dim=dim, depth=3, heads=heads, mlp_dim=128, channels=1,
                dropout=0.25).cuda().train()
    m.set_schedule(dropout_bf16=True).set_compute_dtype(torch.bfloat16)
    m.draw_dropout_seed = lambda: SEED
    img, goal = torch.rand(5, 48, 48).cuda(), torch.rand(5, dim).cuda()
    with torch.no_grad():
        a = m(img, goal)
    b = m(img, goal.clone().requires_grad_(True))
    assert b.requires_grad and torch.equal(a, b.detach())
    m.draw_dropout_seed = lambda: SEED + 1
    with torch.no_grad():
        assert not torch.equal(m(img, goal), a)


# ------------------------------------------------------------------------------------------------ (8) unchanged paths
def test_eval_mode_and_zero_dropout_are_unchanged_by_the_keyword(amd):
    cfg = _C84
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 19)
    img, goal, wout = _inputs(cfg, 5, 19)

    def plain(p):
        m = R.build_got(amd, cfg, 0.0)
        m.load_state_dict(params, strict=True)
        m = m.cuda().train().set_compute_dtype(torch.bfloat16)      # (accepted without the keyword: p is raised afterwards)
        for attn, ff in m.transformer.layers:
            attn.fn.dropout.p = attn.fn.to_out[1].p = ff.fn.net[2].p = ff.fn.net[4].p = p
        m.draw_dropout_seed = lambda: SEED
        return m
    # eval mode at p = 0.3 against the model that never had a p (without the keyword p > 0 is refused in every mode); train mode at p = 0
    for a, b in ((_module(amd, cfg, 0.3, params).eval(), plain(0.0).eval()), (_module(amd, cfg, 0.0, params), plain(0.0))):
        ra, rb_ = _run_module(a, img, goal, wout), _run_module(b, img, goal, wout)
        assert torch.equal(ra[0], rb_[0]) and torch.equal(ra[1], rb_[1])
        assert set(ra[2]) == set(rb_[2])
        for k in ra[2]:
            assert torch.equal(ra[2][k], rb_[2][k]), k


# ------------------------------------------------------------------------------------------------ (9) determinism
def test_same_seed_same_bits_and_the_last_block_schedules_share_their_masks(amd):
    cfg = _C84
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 13)
    img, goal, wout = _inputs(cfg, 6, 13)
    m = _module(amd, cfg, 0.3, params)
    a, b = _run_module(m, img, goal, wout), _run_module(m, img, goal, wout)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    c = _run_module(_module(amd, cfg, 0.3, params, seed=SEED + 1), img, goal, wout)
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[1], c[1])
    # dense and token-0 last blocks under no_grad draw the same masks: the difference stays within the bound that
    # test_encoder_bf16_vs_reference_and_oracle (tests/test_gpu_bf16.py) puts on the same comparison at p = 0
    with torch.no_grad():
        pruned = m(img.cuda(), goal.cuda()).cpu()
        dense = _module(amd, cfg, 0.3, params, dense_last_block=True)(img.cuda(), goal.cuda()).cpu()
    print(f"dense vs token-0 last block at p = 0.3: max {float((pruned - dense).abs().max()):.2e}")
    assert float((pruned - dense).abs().max()) < 2e-2


# ------------------------------------------------------------------------------------------------ (10) graph capture
def test_captured_steps_draw_fresh_masks_and_follow_the_device_seed(amd, F):
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 23)
    img, goal, wout = (t.cuda() for t in _inputs(cfg, 4, 23))
    m = R.build_got(amd, cfg, 0.2)
    m.load_state_dict(params, strict=True)
    m = m.cuda().train().set_schedule(dropout_bf16=True).set_compute_dtype(torch.bfloat16)

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
        f = F.got_encoder_bf16(img, gg, m._cfg, tab, m._bf16_weights, 0.9, seed, layer_dropout_keep=0.8)
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


# ------------------------------------------------------------------------------------------------ (11) attention maps
@pytest.mark.parametrize("rows", ["goal", "all"])
def test_maps_are_taken_before_the_dropout_and_features_equal_forward(amd, rows):
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2, mlp_dim=128)      # N = 50
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 31)
    img, goal, _ = (t.cuda() for t in _inputs(cfg, 3, 31))
    m = _module(amd, cfg, 0.3, params, emb_dropout=0.0)
    feat, maps = m.attention_maps(img, goal, rows=rows)
    with torch.no_grad():
        fwd = m(img, goal)
    assert torch.equal(feat, fwd), "same seed: the maps call returns forward's features"
    _, eval_maps = m.eval().attention_maps(img, goal, rows=rows)
    assert torch.equal(maps[:, 0], eval_maps[:, 0]), "layer 0 sees the same input: its probabilities are those of eval mode"
    assert not torch.equal(maps[:, 1], eval_maps[:, 1]), "layer 1 sees a dropped stream"
    assert torch.allclose(maps.sum(-1), torch.ones_like(maps.sum(-1)), atol=1e-3), "probabilities, not dropped ones: rows sum to 1"


# ------------------------------------------------------------------------------------------------ (12) ABI checks
def test_layer_keep_is_checked_by_every_new_entry_point(amd, F):
    from dgvit_amd._lib import dgvit_config
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=1, heads=2, mlp_dim=128)
    t = _module(amd, cfg, 0.0, O.make_params(O.got_param_spec(cfg, prefix=""), 1))
    lib = amd.load_library()
    cfgc = dgvit_config(*t._cfg)
    c = ctypes.byref(cfgc)
    params = [q.detach() for q in t.param_table()]
    tab = F._table(params)
    wpack = t._bf16_weights.get(cfgc, params)
    nws, nsc = lib.dgvit_got_bf16_workspace_bytes(c, 1, 1), lib.dgvit_got_bf16_backward_scratch_bytes(c, 1)
    ws, sc = torch.empty(nws, dtype=torch.uint8, device="cuda"), torch.empty(nsc, dtype=torch.uint8, device="cuda")
    feat, dfeat = torch.empty(1, 64, device="cuda"), torch.ones(1, 64, device="cuda")
    maps = torch.empty(1, 1, 2, cfg.tokens, device="cuda")
    img, goal = torch.rand(1, 84, 84, device="cuda"), torch.randn(1, 64, device="cuda")
    grads = [torch.empty_like(q) for q in params]
    gtab = F._table(grads)
    p, st = F._ptr, F._stream()
    qkv = torch.zeros(1, 8, 3 * 2 * DH, dtype=torch.bfloat16, device="cuda")
    o, lse, delta = torch.zeros(1, 8, 2 * DH, dtype=torch.bfloat16, device="cuda"), torch.zeros(1, 2, 8, device="cuda"), torch.zeros(16, device="cuda")
    for bad in (0.0, 1.5, float("nan")):
        calls = {
            "forward": lambda: lib.dgvit_got_forward_bf16_v2(c, tab, p(wpack), p(img), p(goal), p(feat), p(ws), nws, 1, 1, 1.0, bad, 0, None, st),
            "maps": lambda: lib.dgvit_got_forward_maps_bf16_v2(c, tab, p(wpack), p(img), p(goal), p(feat), p(maps), 0, p(ws), nws, 1, 1.0, bad, 0,
                                                               None, st),
            "backward": lambda: lib.dgvit_got_backward_bf16_v3(c, tab, p(wpack), gtab, p(dfeat), None, None, p(img), p(ws), nws, p(sc), nsc, 1,
                                                               1.0, bad, 0, None, st),
            "backward_ev": lambda: lib.dgvit_got_backward_bf16_v3_ev(c, tab, p(wpack), gtab, p(dfeat), None, None, p(img), p(ws), nws, p(sc), nsc,
                                                                     1, 1.0, bad, 0, None, st, None),
        }
        for name, call in calls.items():
            assert call() != 0 and b"layer_keep" in lib.dgvit_last_error(), (name, bad)
        ops = {
            "attention_fwd": lambda: lib.dgvit_attention_forward_bf16_tiled_drop(p(qkv), p(o), p(lse), 1, 8, 2, DH, 8, bad, 0, None, 0, st),
            "attention_bwd": lambda: lib.dgvit_attention_backward_bf16_tiled_drop(p(qkv), p(o), p(o), p(lse), p(qkv), p(delta), 1, 8, 2, DH, bad, 0,
                                                                                  None, 0, st),
            "drop_rows": lambda: lib.dgvit_drop_rows_bf16(p(o), 128, p(o), 128, 8, 128, 1, bad, 0, None, 0, 1, st),
        }
        for name, call in ops.items():
            assert call() != 0 and b"keep" in lib.dgvit_last_error(), (name, bad)
    torch.cuda.synchronize()
    assert lib.dgvit_drop_rows_bf16(p(o), 128, p(o), 128, 8, 128, 1, 0.5, 0, None, 0, 0, st) != 0 and b"site" in lib.dgvit_last_error()
