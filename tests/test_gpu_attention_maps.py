"""GPU: attention maps (GoT.attention_maps, dgvit_got_forward_maps[_bf16], dgvit_attention_probs[_bf16]).

Kernel level against an fp64 softmax of the same q / k; the encoder against the oracle's tokens with each layer's LayerNorm, to_qkv and
softmax restated from oracle primitives; the maps call's features against the forward's; the network methods against GoT's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O, load_fixture, fixture_cfg, got_case_inputs  # noqa: E402

MAP_TOL = 1e-4     # encoder maps against the fp64 restatement
OUT_TOL = 1e-4     # features (as tests/test_gpu_parity.py)
BLOCK_TOL = 2e-5   # the small-batch block path against the GEMM schedule (tests/test_gpu_round4.py)


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


def _softmax_ref(qkv, H, dh):
    """(B, H, N, N) fp64 softmax(q k^T dh^-1/2) of a (B, N, 3*H*dh) qkv (any dtype)"""
    B, N, _ = qkv.shape
    I = H * dh
    x = qkv.double()
    q, k = (x[..., j * I:(j + 1) * I].reshape(B, N, H, dh).permute(0, 2, 1, 3) for j in range(2))
    return torch.softmax((q @ k.transpose(-1, -2)) * dh ** -0.5, dim=-1)


def _ref_maps(p, img, goal, cfg, prefix="", pool="cls"):
    """(feat, maps (B, L, H, N, N)) in fp64: the oracle's tokens, then each layer's LayerNorm -> to_qkv -> softmax (GoalFormer.py:72-77)"""
    p = {k: v.double() for k, v in p.items()}
    feat, toks = O.got_forward(p, img.double(), goal.double(), cfg, prefix=prefix, return_tokens=True, pool=pool)
    maps = []
    for i in range(cfg.depth):
        lp = f"{prefix}transformer.layers.{i}."
        h = O.layer_norm(toks[i], p[lp + "0.norm.weight"], p[lp + "0.norm.bias"])
        maps.append(_softmax_ref(O.linear(h, p[lp + "0.fn.to_qkv.weight"]), cfg.heads, cfg.dim_head))
    return feat, torch.stack(maps, 1)


def _ref_maps_bf16(p, img, goal, cfg):
    """maps of O.got_forward_bf16's model (its storage roundings restated here; fp64 arithmetic): the softmax of the bf16 q / k"""
    rb, lin = O.rb, O.linear
    p = {k: v.double() for k, v in p.items()}
    x = lin(rb(O.patchify(img.double(), cfg)), rb(p["to_patch_embedding.1.weight"]), p["to_patch_embedding.1.bias"])
    x = torch.cat([goal.double().unsqueeze(1), x], dim=1) + p["pos_embedding"][:, :cfg.tokens]
    B, N, _ = x.shape
    H, dh = cfg.heads, cfg.dim_head
    I = H * dh
    maps = []
    for i in range(cfg.depth):
        lp = f"transformer.layers.{i}."
        h = rb(O.layer_norm(x, p[lp + "0.norm.weight"], p[lp + "0.norm.bias"]))
        qkv = rb(lin(h, rb(p[lp + "0.fn.to_qkv.weight"])))
        maps.append(_softmax_ref(qkv, H, dh))
        q, k, v = (qkv[..., j * I:(j + 1) * I].reshape(B, N, H, dh).permute(0, 2, 1, 3) for j in range(3))
        dots = (q @ k.transpose(-1, -2)) * dh ** -0.5
        e = torch.exp(dots - dots.amax(-1, keepdim=True))
        out = rb(((rb(e) @ v) / e.sum(-1, keepdim=True)).permute(0, 2, 1, 3).reshape(B, N, I))
        x = rb(lin(out, rb(p[lp + "0.fn.to_out.0.weight"]), p[lp + "0.fn.to_out.0.bias"])) + x
        h = rb(O.layer_norm(x, p[lp + "1.norm.weight"], p[lp + "1.norm.bias"]))
        a = rb(O.gelu_exact(lin(h, rb(p[lp + "1.fn.net.0.weight"]), p[lp + "1.fn.net.0.bias"])))
        x = rb(lin(a, rb(p[lp + "1.fn.net.3.weight"]), p[lp + "1.fn.net.3.bias"])) + x
    return torch.stack(maps, 1)


def _got(amd, cfg, params, pool="cls", dropout=0.0, emb_dropout=0.0):
    m = amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=2, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads,
                mlp_dim=cfg.mlp_dim, channels=1, dim_head=cfg.dim_head, pool=pool, dropout=dropout, emb_dropout=emb_dropout)
    m.load_state_dict(params, strict=True)
    return m.cuda().eval()


def _maps(m, img, goal, rows):
    f, a = m.attention_maps(img.cuda(), goal.cuda(), rows=rows)
    assert not f.requires_grad and not a.requires_grad
    return f.cpu(), a.cpu()


def _forward(m, img, goal):
    with torch.no_grad():
        return m(img.cuda(), goal.cuda()).cpu()


def _close(a, b, tol, msg=""):
    d = float((a.double() - b.double()).abs().max()) if a.numel() else 0.0
    assert d <= tol, f"{msg}: max |diff| {d:.3g} > {tol:.3g}"


def _rows_sum_to_one(maps, tol=1e-5):
    _close(maps.double().sum(-1), torch.ones(maps.shape[:-1], dtype=torch.float64), tol, "row sums")


# ------------------------------------------------------------------------------------------------ kernel level
KERNEL_N = [1, 2, 50, 63, 64, 197, 257, 288, 321, 785]


@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("N", KERNEL_N)
def test_probs_kernel_fp32(amd, N, dh):
    from dgvit_amd import functional as F
    B, H = 2, 3
    g = torch.Generator().manual_seed(N * 7 + dh)
    qkv = (torch.randn(B, N, 3 * H * dh, generator=g) * 0.6).cuda()
    _, lse = F.op_attention_fwd(qkv, H, dh) if N <= 288 else F.op_attention_fwd_tiled(qkv, H, dh)
    ref = _softmax_ref(qkv.cpu(), H, dh)
    goal = F.op_attention_probs(qkv, lse, H, dh, rows="goal").cpu()
    full = F.op_attention_probs(qkv, lse, H, dh, rows="all").cpu()
    assert goal.shape == (B, H, N) and full.shape == (B, H, N, N)
    _close(full, ref, 1e-6, f"all rows N={N} dh={dh}")
    _close(goal, ref[:, :, 0], 1e-6, f"goal row N={N} dh={dh}")
    _rows_sum_to_one(full)
    _rows_sum_to_one(goal)


@pytest.mark.parametrize("N", [1, 2, 50, 63, 64, 197, 224])      # (the bf16 attention's limit is 224 tokens)
def test_probs_kernel_bf16(amd, N):
    from dgvit_amd import functional as F
    B, H, dh = 2, 3, 64
    g = torch.Generator().manual_seed(N * 11)
    qkv = (torch.randn(B, N, 3 * H * dh, generator=g) * 0.6).to(torch.bfloat16).cuda()
    _, lse = F.op_attention_bf16(qkv, H, dh, want_lse=True)
    ref = _softmax_ref(qkv.cpu(), H, dh)              # the same bf16 inputs: only fp32 arithmetic differs
    goal = F.op_attention_probs_bf16(qkv, lse, H, dh, rows="goal").cpu()
    full = F.op_attention_probs_bf16(qkv, lse, H, dh, rows="all").cpu()
    _close(full, ref, 1e-5, f"bf16 all rows N={N}")
    _close(goal, ref[:, :, 0], 1e-5, f"bf16 goal row N={N}")
    _rows_sum_to_one(full)
    _rows_sum_to_one(goal)


# ------------------------------------------------------------------------------------------------ encoder vs oracle
@pytest.mark.parametrize("name,pool", [("got_84p12", "cls"), ("got_tiny_meanpool", "mean"), ("got_tiny_h1_mask", "cls")])
def test_encoder_maps_against_the_oracle(amd, name, pool):
    fx = load_fixture(name)
    cfg = fixture_cfg(fx)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), int(fx["meta/seed"]))
    img, goal, _, _ = got_case_inputs(fx, cfg, False)
    m = _got(amd, cfg, params, pool=pool)
    ref_feat, ref = _ref_maps(params, img, goal, cfg, pool=pool)
    fg, mg = _maps(m, img, goal, "goal")
    fa, ma = _maps(m, img, goal, "all")
    B, L, H, N = img.shape[0], cfg.depth, cfg.heads, cfg.tokens
    assert mg.shape == (B, L, H, N) and ma.shape == (B, L, H, N, N)
    _close(ma, ref, MAP_TOL, "all rows")
    _close(mg, ref[..., 0, :], MAP_TOL, "goal rows")
    _close(fg, ref_feat, OUT_TOL, "features (goal call)")
    _close(fa, ref_feat, OUT_TOL, "features (all call)")
    if name == "got_84p12":
        np.testing.assert_allclose(fg.numpy(), fx["feat"], rtol=0, atol=OUT_TOL)
    _rows_sum_to_one(ma)


def test_policy_maps_against_the_oracle(amd):
    fx = load_fixture("policy_native_shipped")
    cfg = fixture_cfg(fx)
    batch, seed = int(fx["meta/batch"]), int(fx["meta/seed"])
    params = O.make_params(O.policy_param_spec(cfg), seed)
    m = amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    m.load_state_dict(params, strict=True)
    m = m.to("cuda").eval()
    img, pstate, _, _ = O.make_inputs(cfg, batch, seed)
    goal = O.linear(pstate.double(), params["fc_embed.weight"].double(), params["fc_embed.bias"].double())
    ref_feat, ref = _ref_maps(params, img, goal, cfg, prefix="trans.")
    f, mg = m.attention_maps([img.cuda(), pstate.cuda()])
    _close(mg.cpu(), ref[..., 0, :], MAP_TOL, "policy goal rows")
    _close(f.cpu(), ref_feat, OUT_TOL, "policy features")


# ------------------------------------------------------------------------------------------------ schedules agree
def _shipped(amd, seed=5):
    cfg = O.GoTConfig(image=(128, 160), patch=(16, 20), dim=64, depth=4, heads=4, mlp_dim=2048)
    return cfg, O.make_params(O.got_param_spec(cfg, prefix=""), seed)


@pytest.mark.parametrize("B", [1, 2, 32, 64])
def test_features_equal_forward_and_goal_rows_equal_row_zero(amd, B):
    """B = 1, 2: the forward takes the small-batch block path, the maps call the GEMM schedule (2e-5); B = 32 is held to the same
    bound; B = 64: both take the GEMM schedule (bitwise for rows='goal'; rows='all' equals the forward with the dense last block)."""
    cfg, params = _shipped(amd)
    img, _, _, _ = O.make_inputs(cfg, B, 9)
    goal = torch.randn(B, cfg.dim, generator=torch.Generator().manual_seed(B))
    m = _got(amd, cfg, params)
    ref = _forward(m, img, goal)
    fg, mg = _maps(m, img, goal, "goal")
    fa, ma = _maps(m, img, goal, "all")
    if B == 64:
        assert torch.equal(fg, ref)
    else:
        _close(fg, ref, BLOCK_TOL, "features vs block path")
    _close(fa, ref, BLOCK_TOL, "features (dense last block)")
    if B == 64:
        with torch.no_grad():
            dense = m.set_schedule(dense_last_block=True)(img.cuda(), goal.cuda()).cpu()
        m.set_schedule()
        assert torch.equal(fa, dense), "rows='all' runs forward's dense-last-block schedule"
    _close(mg, ma[..., 0, :], 1e-6, "goal rows vs row 0")
    _rows_sum_to_one(mg)


def test_long_sequence_maps(amd):
    """321 and 785 tokens on the K/V-tiled attention against the restated oracle; at N <= 288 the flag changes nothing, bitwise."""
    for image, patch in (((160, 128), (8, 8)), ((224, 224), (8, 8))):
        cfg = O.GoTConfig(image=image, patch=patch, dim=64, depth=2, heads=2, mlp_dim=128)
        assert cfg.tokens in (321, 785)
        params = O.make_params(O.got_param_spec(cfg, prefix=""), 3)
        img, _, _, _ = O.make_inputs(cfg, 2, 4)
        goal = torch.randn(2, cfg.dim, generator=torch.Generator().manual_seed(1))
        m = _got(amd, cfg, params).set_schedule(long_sequence=True)
        ref_feat, ref = _ref_maps(params, img, goal, cfg)
        fg, mg = _maps(m, img, goal, "goal")
        fa, ma = _maps(m, img, goal, "all")
        _close(ma, ref, MAP_TOL, f"N={cfg.tokens} all rows")
        _close(mg, ref[..., 0, :], MAP_TOL, f"N={cfg.tokens} goal rows")
        _close(fg, ref_feat, OUT_TOL, f"N={cfg.tokens} features")
        assert torch.equal(fg, _forward(m, img, goal))
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=4, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 3)
    img, _, _, _ = O.make_inputs(cfg, 3, 4)
    goal = torch.randn(3, cfg.dim)
    m = _got(amd, cfg, params)
    plain = [_maps(m, img, goal, r) for r in ("goal", "all")]
    m.set_schedule(long_sequence=True)
    flagged = [_maps(m, img, goal, r) for r in ("goal", "all")]
    for (fa, ma), (fb, mb) in zip(plain, flagged):
        assert torch.equal(fa, fb) and torch.equal(ma, mb)


def test_bf16_maps(amd):
    fx = load_fixture("got_c5_l2_bf16")
    cfg = fixture_cfg(fx)
    batch, seed = int(fx["meta/batch"]), int(fx["meta/seed"])
    params = O.make_params(O.got_param_spec(cfg, prefix=""), seed)
    img, _, _, _ = O.make_inputs(cfg, batch, seed)
    goal = torch.from_numpy(np.random.RandomState(seed + 7).standard_normal((batch, cfg.dim))).float()
    m = _got(amd, cfg, params)
    f32_feat, f32_all = _maps(m, img, goal, "all")
    m.set_compute_dtype(torch.bfloat16)
    fg, mg = _maps(m, img, goal, "goal")
    fa, ma = _maps(m, img, goal, "all")
    assert torch.equal(fg, _forward(m, img, goal)), "goal-row call runs forward's bf16 schedule"
    ref = _ref_maps_bf16(params, img, goal, cfg)
    _close(ma, ref, 2e-2, "bf16 all rows vs the bf16 restatement")         # the bound of test_encoder_bf16_vs_reference_and_oracle
    _close(mg, ref[..., 0, :], 2e-2, "bf16 goal rows vs the bf16 restatement")
    _close(ma, f32_all, 5e-2, "bf16 maps vs fp32 maps")                     # bf16 storage of every GEMM operand upstream
    _close(mg, ma[..., 0, :], 1e-5, "bf16 goal rows vs row 0")
    _rows_sum_to_one(ma)
    _rows_sum_to_one(mg)


@pytest.mark.parametrize("bf16", [False, True])
def test_empty_batch(amd, bf16):
    cfg, params = _shipped(amd)
    m = _got(amd, cfg, params)
    if bf16:
        m.set_compute_dtype(torch.bfloat16)
    for rows, shape in (("goal", (0, 4, 4, cfg.tokens)), ("all", (0, 4, 4, cfg.tokens, cfg.tokens))):
        f, a = m.attention_maps(torch.zeros(0, 128, 160).cuda(), torch.zeros(0, 64).cuda(), rows=rows)
        assert f.shape == (0, 64) and a.shape == shape


# ------------------------------------------------------------------------------------------------ train mode, determinism
def test_train_mode_features_equal_forward(amd):
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=4, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 2)
    img, _, _, _ = O.make_inputs(cfg, 6, 2)
    goal = torch.randn(6, cfg.dim)
    m = _got(amd, cfg, params, dropout=0.1, emb_dropout=0.1).train()
    for rows in ("goal", "all"):
        torch.manual_seed(77)
        f, a = _maps(m, img, goal, rows)
        torch.manual_seed(77)
        ref = _forward(m, img, goal)
        if rows == "goal":
            assert torch.equal(f, ref)
        else:
            _close(f, ref, BLOCK_TOL, "train mode, dense last block")
        _rows_sum_to_one(a)


def test_frame_alone_equals_frame_in_batch_and_repeats(amd):
    cfg = O.GoTConfig(image=(128, 160), patch=(16, 20), dim=64, depth=2, heads=4, mlp_dim=128)
    params = O.make_params(O.got_param_spec(cfg, prefix=""), 16)
    img, _, _, _ = O.make_inputs(cfg, 5, 1)
    goal = torch.randn(5, cfg.dim)
    m = _got(amd, cfg, params)
    for rows in ("goal", "all"):
        _, batch = _maps(m, img, goal, rows)
        _, again = _maps(m, img, goal, rows)
        assert torch.equal(batch, again)
        _, alone = _maps(m, img[2:3], goal[2:3], rows)
        assert torch.equal(alone[0], batch[2])


# ------------------------------------------------------------------------------------------------ networks
def test_network_methods_equal_got(amd):
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=4, mlp_dim=2048)
    img, pstate, _, _ = O.make_inputs(cfg, 5, 8)
    a = torch.randn(5, 2)
    for cls in (amd.GoTPolicy, amd.DeterministicGoTPolicy, amd.GoTQNetwork):
        torch.manual_seed(0)
        net = cls(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch).to("cuda").eval()
        with torch.no_grad():
            goal = torch.nn.functional.linear(pstate.cuda(), net.fc_embed.weight, net.fc_embed.bias)
            if cls is amd.GoTQNetwork:
                goal = torch.relu(goal)
        for rows in ("goal", "all"):
            f0, m0 = net.trans.attention_maps(img.cuda(), goal, rows=rows)
            inps = [[img.cuda(), pstate.cuda()]] + ([[img.cuda(), pstate.cuda(), a.cuda()]] if cls is amd.GoTQNetwork else [])
            for inp in inps:
                f1, m1 = net.attention_maps(inp, rows=rows)
                _close(f1.cpu(), f0.cpu(), 1e-6, f"{cls.__name__} features")
                _close(m1.cpu(), m0.cpu(), 1e-6, f"{cls.__name__} maps")
