"""GPU: the bf16 encoder with patch areas that are not multiples of 8 (14x14: ViT-S/B/14 at 224x224; 7x7, 6x6, 3x5, 3x4).

The rows of the bf16 patch operands are padded to ldp = up8(pd) elements with a zero tail (the patch GEMM needs K and both row strides
% 8 == 0).  Forward against the oracle's bf16-storage model and its fp32 model, gradients against fp32 autograd on the oracle, with the
bounds of tests/test_gpu_bf16_288.py; the pad columns through the C ABI with caller buffers full of NaN patterns; weight repacking;
maps and the SAC policy.  (Patch areas that ARE multiples of 8 run the kernels and launches they ran before: DESIGN section 3.22 compares
the assembly; tests/test_bf16_patch_area_host.py holds their size queries to the earlier build's numbers.)  Before this change every
call with such a patch failed with `bf16 path: dim, mlp_dim and patch pixels must be multiples of 8`."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O  # noqa: E402


def _cfg(image, patch, dim, heads, mlp, depth=2):
    return O.GoTConfig(image=image, patch=patch, dim=dim, depth=depth, heads=heads, dim_head=64, mlp_dim=mlp)


# name -> (config, batch).  pd / ldp / tokens and the branch each shape reaches:
SHAPES = {
    "28p7": (_cfg((28, 28), (7, 7), 64, 2, 128), 5),              # 49 / 56 / 17: odd width, one-pixel kernel, unaligned weight rows
    "12x16p3x4": (_cfg((12, 16), (3, 4), 64, 2, 128), 5),         # 12 / 16 / 17: the four-pixel kernel, pd < 16
    "30x50p3x5": (_cfg((30, 50), (3, 5), 64, 2, 128), 4),         # 15 / 16 / 101: one pad column
    "84p14": (_cfg((84, 84), (14, 14), 128, 2, 256), 4),          # 196 / 200 / 37
    "84p6": (_cfg((84, 84), (6, 6), 128, 2, 256), 3),             # 36 / 40 / 197
    "vitb14_224_l2": (_cfg((224, 224), (14, 14), 768, 12, 3072), 2),   # 196 / 200 / 257: the 288-row attention plan
    "vits14_224_l2": (_cfg((224, 224), (14, 14), 384, 6, 1536), 3),    # 196 / 200 / 257
}


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


@pytest.fixture(scope="module", autouse=True)
def padded_patch_build():
    """every test here is about a library that pads patch areas: one 7x7 bf16 forward, or the library's own refusal"""
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    cfg, batch = SHAPES["28p7"]
    params, img, goal = _inputs(cfg, batch, 1)
    with torch.no_grad():
        assert torch.isfinite(_got(cfg, params).set_compute_dtype(torch.bfloat16)(img.cuda(), goal.cuda())).all()


_REFS = {}


def _refs(name):
    """(params, img, goal, emulation, fp32 reference) of a shape, computed once"""
    if name not in _REFS:
        cfg, batch = SHAPES[name]
        params, img, goal = _inputs(cfg, batch, 31)
        _REFS[name] = (params, img, goal, O.got_forward_bf16(params, img, goal, cfg, prefix=""), O.got_forward(params, img, goal, cfg, prefix=""))
    return _REFS[name]


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("name", list(SHAPES))
def test_forward(name):
    cfg, batch = SHAPES[name]
    assert (cfg.patch[0] * cfg.patch[1]) % 8 != 0
    params, img, goal, emu, ref32 = _refs(name)
    m = _got(cfg, params).set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        feat = m(img.cuda(), goal.cuda()).cpu()
        dense = m.set_schedule(dense_last_block=True)(img.cuda(), goal.cuda()).cpu()
    d_emu, d32 = (feat - emu).abs(), (feat - ref32).abs()
    print(f"{name}: vs emulation max {d_emu.max():.4f} mean {d_emu.mean():.5f} | vs fp32 max {d32.max():.4f} mean {d32.mean():.5f}"
          f" | emulation vs fp32 max {(emu - ref32).abs().max():.4f} | token-0 vs dense {(feat - dense).abs().max():.5f}")
    assert torch.isfinite(feat).all()
    # the bounds of tests/test_gpu_bf16_288.py::test_encoder_forward_257_tokens
    assert d_emu.max() < 2e-2 and d_emu.mean() < 3e-3
    assert d32.max() < max(3e-2, 2 * float((emu - ref32).abs().max()))
    assert d32.mean() < 6e-3
    assert (feat - dense).abs().max() < 2e-2, "token-0 last block and dense last block disagree"


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("name,pool", [("28p7", "cls"), ("28p7", "mean"), ("12x16p3x4", "cls"), ("30x50p3x5", "cls"), ("84p14", "cls"),
                                       ("84p6", "cls"), ("vitb14_224_l2", "cls"), ("vits14_224_l2", "cls")])
def test_gradients(name, pool):
    """parameter, goal and frame gradients within 2e-2 relative L2 of fp32 autograd on the oracle (the bound of
    test_encoder_gradients_257_tokens); the patch weight's gradient has the parameter's shape (D, pd), not the padded (D, ldp)"""
    cfg, batch = SHAPES[name]
    batch = min(batch, 4)
    params, img, goal = _inputs(cfg, batch, 21)
    wout = torch.from_numpy(np.random.RandomState(29).standard_normal((batch, cfg.dim))).float()
    ps = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    g, x = goal.clone().requires_grad_(True), img.clone().requires_grad_(True)
    (O.got_forward(ps, x, g, cfg, prefix="", pool=pool) * wout).sum().backward()
    m = _got(cfg, params, pool).set_compute_dtype(torch.bfloat16)
    gd, xd = goal.cuda().requires_grad_(True), img.cuda().requires_grad_(True)
    (m(xd, gd) * wout.cuda()).sum().backward()
    ours = {k: v.grad for k, v in m.named_parameters()}
    pd = cfg.patch[0] * cfg.patch[1]
    assert tuple(ours["to_patch_embedding.1.weight"].shape) == (cfg.dim, pd)
    errs = {}
    for k, ref in ((k, v.grad) for k, v in ps.items()):
        if ref is None or float(ref.abs().max()) == 0.0:
            assert ours[k] is None or float(ours[k].abs().max()) == 0.0, f"{k} should have no gradient"
            continue
        assert ours[k] is not None, f"{k}: no gradient"
        assert ours[k].shape == ref.shape, k
        errs[k] = float((ours[k].cpu() - ref).norm() / ref.norm())
    errs["dgoal"] = float((gd.grad.cpu() - g.grad).norm() / g.grad.norm())
    errs["dimg"] = float((xd.grad.cpu() - x.grad).norm() / x.grad.norm())
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"{name} {pool}: worst relative gradient error vs fp32 {worst}; patch weight {errs['to_patch_embedding.1.weight']:.5f}")
    assert worst[1] < 2e-2, {k: round(v, 4) for k, v in errs.items() if v > 2e-2}


# ------------------------------------------------------------------------------------------------ pad columns
def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _abi_forward(lib, cfg, batch, table, img, goal, fill, save, runs=1):
    """pack + forward through the C ABI with caller-owned arena and workspace, both filled with the byte `fill` before the pack and
    before the first forward; the features of each of `runs` forwards on the same workspace"""
    from dgvit_amd import _lib
    c = _lib.dgvit_config(cfg.image[0], cfg.image[1], cfg.patch[0], cfg.patch[1], cfg.dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.mlp_dim)
    nwp = lib.dgvit_got_bf16_weight_elems(ctypes.byref(c))
    nws = lib.dgvit_got_bf16_workspace_bytes(ctypes.byref(c), batch, save)
    assert nwp > 0 and nws > 0, lib.dgvit_last_error()
    arena = torch.full((nwp * 2,), fill, dtype=torch.uint8, device="cuda")
    ws = torch.full((nws,), fill, dtype=torch.uint8, device="cuda")
    _lib.check(lib.dgvit_got_pack_weights_bf16(ctypes.byref(c), table, _p(arena), nwp, save, _st()), "dgvit_got_pack_weights_bf16")
    feats = []
    for _ in range(runs):
        feat = torch.full((batch, cfg.dim), float("nan"), device="cuda")
        rc = lib.dgvit_got_forward_bf16(ctypes.byref(c), table, _p(arena), _p(img), _p(goal), _p(feat), _p(ws), nws, batch, save, 1.0, 0, None,
                                        _st())
        _lib.check(rc, "dgvit_got_forward_bf16")
        torch.cuda.synchronize()
        feats.append(feat)
    return feats, arena.view(torch.bfloat16)


@pytest.mark.parametrize("save", [0, 1], ids=["nograd", "save"])
@pytest.mark.parametrize("name", ["28p7", "12x16p3x4", "30x50p3x5"])
def test_pad_columns_do_not_depend_on_what_the_buffers_held(name, save):
    """pd = 49, 12, 15.  The workspace and the arena are the caller's memory: with every byte 0xFF (bf16 and fp32 NaN patterns) before
    the pack and before the forward, the features are finite and bitwise those of zero-filled buffers -- the pad columns of the patches
    are written by every forward (the weight's zero tail alone would not do: NaN x 0 is NaN) and those of the patch weight by the
    pack.  A second forward on the same workspace, now holding the first one's activations, gives the same bits."""
    import dgvit_amd
    lib = dgvit_amd.load_library()
    cfg, batch = SHAPES[name]
    params, img, goal = _inputs(cfg, batch, 13)
    m = _got(cfg, params)
    tab = [p.detach().contiguous() for p in m.param_table()]
    table = (ctypes.c_void_p * len(tab))(*[p.data_ptr() for p in tab])
    img, goal = img.cuda().contiguous(), goal.cuda().contiguous()
    (clean,), arena0 = _abi_forward(lib, cfg, batch, table, img, goal, 0x00, save)
    (dirty, again), arena1 = _abi_forward(lib, cfg, batch, table, img, goal, 0xFF, save, runs=2)
    assert torch.isfinite(clean).all() and torch.isfinite(dirty).all()
    assert torch.equal(clean, dirty), "features depend on what the caller's buffers held"
    assert torch.equal(dirty, again), "second forward on the used workspace differs"
    # the patch weight in the arena: D rows of ldp, the fp32 master rounded to bf16, then zeros
    pd = cfg.patch[0] * cfg.patch[1]
    ldp = (pd + 7) & ~7
    w = arena1[:cfg.dim * ldp].view(cfg.dim, ldp)
    assert torch.equal(w[:, :pd], tab[1].to(torch.bfloat16)) and bool((w[:, pd:].view(torch.int16) == 0).all())
    assert torch.equal(arena0[:cfg.dim * ldp], arena1[:cfg.dim * ldp])
    with torch.set_grad_enabled(bool(save)):    # and the call did the real thing: the module's features in the same mode, bit for bit
        assert torch.equal(m.set_compute_dtype(torch.bfloat16)(img, goal).detach(), clean)


# ------------------------------------------------------------------------------------------------ weights
def test_repack_follows_parameter_writes_and_frozen_weights_give_the_same_bits():
    import dgvit_amd
    cfg, batch = SHAPES["28p7"]
    params, img, goal, emu, _ = _refs("28p7")
    m = _got(cfg, params).set_compute_dtype(torch.bfloat16)
    x, g = img.cuda(), goal.cuda()
    k = "to_patch_embedding.1.weight"
    with torch.no_grad():
        f0 = m(x, g)
        frozen = m.freeze_bf16_weights()(x, g)
        packs = m._bf16_weights.packs
        assert torch.equal(frozen, f0) and torch.equal(m(x, g), f0) and m._bf16_weights.packs == packs, "frozen weights: one pack, same bits"
        m.freeze_bf16_weights(False)
        # an in-place write behind autograd's back: the default repack before every forward follows it
        new = {**params, k: params[k] * 0.5 + 0.25 * torch.from_numpy(np.random.RandomState(3).standard_normal(tuple(params[k].shape))).float()}
        dict(m.named_parameters())[k].data.copy_(new[k].cuda())
        f1 = m(x, g)
        emu1 = O.got_forward_bf16(new, img, goal, cfg, prefix="")
        assert float((emu1 - emu).abs().max()) > 5e-2, "the write should move the features"
        assert float((f1.cpu() - emu1).abs().max()) < 2e-2
        # frozen: the package's own writers invalidate (load_state_dict, notify_parameters_changed)
        m.freeze_bf16_weights()
        assert torch.equal(m(x, g), f1)
        m.load_state_dict(params, strict=True)
        assert torch.equal(m(x, g), f0), "load_state_dict must repack the padded patch weight"
        dict(m.named_parameters())[k].data.copy_(new[k].cuda())
        dgvit_amd.functional.notify_parameters_changed(m)
        assert torch.equal(m(x, g), f1), "notify_parameters_changed must repack the padded patch weight"


# ------------------------------------------------------------------------------------------------ maps and the SAC networks
def test_attention_maps_28p7():
    """bf16 maps (goal rows and all rows) against an fp64 softmax of the bf16 model's q / k, as test_encoder_maps_257_tokens"""
    from test_gpu_attention_maps import _ref_maps_bf16
    cfg, batch = SHAPES["28p7"]
    params, img, goal = _inputs(cfg, batch, 41)
    m = _got(cfg, params).set_compute_dtype(torch.bfloat16)
    fg, mg = m.attention_maps(img.cuda(), goal.cuda(), rows="goal")
    fa, ma = m.attention_maps(img.cuda(), goal.cuda(), rows="all")
    ref = _ref_maps_bf16(params, img, goal, cfg)
    ma, mg = ma.cpu().double(), mg.cpu().double()
    assert mg.shape == (batch, cfg.depth, cfg.heads, 17) and ma.shape[-2:] == (17, 17)
    assert float((ma - ref).abs().max()) < 2e-2 and float((mg - ref[..., 0, :]).abs().max()) < 2e-2
    assert float((mg - ma[..., 0, :]).abs().max()) < 1e-5
    assert float((mg.sum(-1) - 1).abs().max()) < 1e-5
    with torch.no_grad():
        assert torch.equal(fg.cpu(), m(img.cuda(), goal.cuda()).cpu())


def test_sac_policy_with_bf16_encoder_28p7():
    """GoTPolicy on 28x28 frames with 7x7 patches, encoder in bf16: sample() and attention_maps(rows='goal') work, tanh(mean) is close
    to the fp32 oracle, the maps are those of the bf16 model, the backward gives finite gradients"""
    import dgvit_amd
    from test_gpu_attention_maps import _ref_maps_bf16
    cfg = O.GoTConfig(image=(28, 28), patch=(7, 7), dim=64, depth=2, heads=4)
    params = O.make_params(O.policy_param_spec(cfg), 5)
    m = dgvit_amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    m.load_state_dict(params, strict=True)
    m = m.cuda().eval()
    m.trans.set_compute_dtype(torch.bfloat16)
    img, pstate, _, _ = O.make_inputs(cfg, 4, 5)
    x = img.cuda().requires_grad_(True)
    action, log_prob, mean_t = m.sample([x, pstate.cuda()])
    (action.sum() + log_prob.sum()).backward()
    rm, _ = O.policy_forward(params, img, pstate, cfg)
    assert action.shape == (4, 2) and bool(torch.isfinite(action).all()) and bool(torch.isfinite(log_prob).all())
    assert float(action.abs().max()) <= 1.0
    assert float((mean_t.detach().cpu() - torch.tanh(rm)).abs().max()) < 5e-2     # (the bound of test_sac_policy_with_bf16_encoder_257_tokens)
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    gw = m.trans.to_patch_embedding[1].weight.grad
    assert gw is not None and tuple(gw.shape) == (64, 49) and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
    feat, maps = m.attention_maps([img.cuda(), pstate.cuda()], rows="goal")
    goal = torch.nn.functional.linear(pstate, params["fc_embed.weight"], params["fc_embed.bias"])
    ref = _ref_maps_bf16({k[len("trans."):]: v for k, v in params.items() if k.startswith("trans.")}, img, goal, cfg)
    assert maps.shape == (4, cfg.depth, cfg.heads, 17)
    assert float((maps.cpu().double() - ref[..., 0, :]).abs().max()) < 2e-2
