"""GPU: the CNN critic (QNetwork) and actor (GaussianPolicy) on channel-last frame stacks, conv1 with K input channels:
im2col for any channel count, the (B, H, W, K) frame gradient, conv1 through the implicit-GEMM window loader for K % 4 == 0, and the
``_v2`` / ``_v3`` entry points of the C ABI.

The reference is tests/cnn_stack_ref.py: fp64 conv2d on ``stack.permute(0, 3, 1, 2)`` with autograd, on data whose forward sums are
exact in fp32 (no pre-activation sits on a ReLU kink; tests/test_cnn_frame_channels_host.py checks the data).  Tolerances are the
existing CNN ones.  Every test but the K = 1 ones fails without the feature: ``frame_channels`` is a TypeError and the symbols do not
exist."""
import pytest
import torch

from helpers import knobs
import cnn_stack_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64            # floats on each side of a guarded buffer (256 bytes: the buffer itself stays 16-byte aligned)
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


def _net(amd, kind, K, params=None, **kw):
    m = amd.QNetwork(2, 2, **kw) if kind == "qnet" else amd.GaussianPolicy(2, 2, **kw)
    m.load_state_dict(params if params is not None else R.exact_params(kind, K), strict=True)
    return m.cuda()


def _run(m, kind, stack, B, grad_stack=True):
    """(outs, stack gradient, parameter gradients by name) of the reference's loss on the device"""
    pstate, a = (t.cuda() for t in R.small_inputs(B))
    x = stack.cuda().requires_grad_(grad_stack)
    for q in m.parameters():
        q.grad = None
    outs = m([x, pstate, a]) if kind == "qnet" else m([x, pstate])
    R.loss(outs, [w.cuda() for w in R.out_weights(B, 2)]).backward()
    torch.cuda.synchronize()
    return [o.detach() for o in outs], x.grad, {k: q.grad for k, q in m.named_parameters()}


def _conv_params(p, grad=True):
    return [p[k].cuda().requires_grad_(grad) for k in R.CONV]


# ------------------------------------------------------------------------------------------------ 1. parity with fp64
@pytest.mark.parametrize("kind", ["qnet", "policy"])
@pytest.mark.parametrize("hw, K, B", R.CASES, ids=str)
def test_networks_on_frame_stacks_match_fp64(amd, kind, hw, K, B):
    ref = R.reference(kind, hw, K, B)
    m = _net(amd, kind, K, frame_channels=K)
    stack = R.exact_stack(B, hw, K)
    outs, dstack, grads = _run(m, kind, stack, B)
    with torch.no_grad():
        feat = m._features(stack.cuda())
    assert feat.shape == (B, 256) and dstack.shape == (B, *hw, K) and dstack.is_contiguous()
    R.check_close(feat, ref["feat"], "features")
    for i, (o, r) in enumerate(zip(outs, ref["outs"])):
        assert o.shape == r.shape
        R.check_close(o, r, f"output {i}")
    assert set(grads) == set(ref["grads"])
    for k, g in grads.items():
        assert g.shape == ref["grads"][k].shape
        R.check_grad(g, ref["grads"][k], k)
    err = R.rel_l2(dstack, ref["dstack"])
    assert err <= R.DIMG_TOL, f"frame gradient: relative L2 {err:.3e}"
    if hw[0] % 2 == 0:      # an even height: the last row lies in no 5 x 5 stride-2 window
        assert float(ref["dstack"][:, -1].abs().max()) == 0.0
        assert not bool(dstack[:, -1].any()), "the gradient of a row that no window covers must be exactly 0"
        assert bool(dstack[:, -2].any())


# ------------------------------------------------------------------------------------------------ 2. channel order
@pytest.mark.parametrize("K, c", [(3, 0), (3, 1), (3, 2), (8, 0), (8, 5), (8, 7), (5, 3), (16, 15)])
def test_channel_c_of_the_stack_meets_channel_c_of_conv1(amd, K, c):
    """a stack whose only non-zero channel is c: the K-channel network equals the single-channel network with conv1.weight[:, c:c+1]
    on that frame; the other channels' frame gradients (their frames are zero, their weights are not) equal the fp64 reference's"""
    hw, B, kind = (30, 37), 3, "qnet"
    p = R.exact_params(kind, K)
    stack = torch.zeros(B, *hw, K)
    stack[..., c] = R.exact_stack(B, hw, K)[..., c]
    outs, dstack, grads = _run(_net(amd, kind, K, p, frame_channels=K), kind, stack, B)
    p1 = dict(p, **{"conv1.weight": p["conv1.weight"][:, c:c + 1].contiguous()})
    outs1, dframe, grads1 = _run(_net(amd, kind, 1, p1), kind, stack[..., c].contiguous(), B)
    for i, (o, o1) in enumerate(zip(outs, outs1)):
        R.check_close(o, o1, f"output {i}")
    for k in grads:
        R.check_grad(grads[k][:, c:c + 1] if k == "conv1.weight" else grads[k], grads1[k], k)
    assert R.rel_l2(dstack[..., c], dframe) <= R.DIMG_TOL
    # fp64 on the same stack
    pd = {k: v.double().requires_grad_(True) for k, v in p.items()}
    xr = stack.double().requires_grad_(True)
    pstate, a = (t.double() for t in R.small_inputs(B))
    R.loss(R.forward(kind, pd, xr, pstate, a), R.out_weights(B, 2)).backward()
    for j in range(K):
        assert R.rel_l2(dstack[..., j], xr.grad[..., j]) <= R.DIMG_TOL, f"frame gradient of channel {j}"
    others = [j for j in range(K) if j != c]
    assert all(float(xr.grad[..., j].abs().max()) > 0 for j in others)
    R.check_grad(grads["conv1.weight"], pd["conv1.weight"].grad, "conv1.weight")
    assert not bool(grads["conv1.weight"][:, others].any()), "the weight gradient of a channel whose frames are zero is exactly 0"


# ------------------------------------------------------------------------------------------------ 3. K = 1 is untouched
def _raw_old(lib, img, params, dfeat, want_dimg=True):
    """features, gradients and frame gradient through dgvit_cnn_forward / dgvit_cnn_backward_v2 (the single-frame entry points)"""
    from dgvit_amd.functional import _ptr, _stream, _table
    B, H, W = img.shape
    nws, nf, nb = (int(f(B, H, W)) for f in (lib.dgvit_cnn_workspace_floats, lib.dgvit_cnn_forward_scratch_floats,
                                             lib.dgvit_cnn_backward_scratch_floats))
    ws, scf, scb = (torch.empty(n, device="cuda") for n in (nws, nf, nb))
    feat, grads = torch.empty(B, 256, device="cuda"), [torch.empty_like(p) for p in params]
    dimg = torch.empty_like(img) if want_dimg else None
    assert lib.dgvit_cnn_forward(_ptr(img), _table(params), _ptr(feat), _ptr(ws), nws, _ptr(scf), nf, B, H, W, _stream()) == 0
    assert lib.dgvit_cnn_backward_v2(_ptr(img), _table(params), _table(grads), _ptr(dfeat), _ptr(dimg), _ptr(ws), nws, _ptr(scb), nb,
                                     B, H, W, _stream()) == 0
    torch.cuda.synchronize()
    return feat, grads, dimg


@pytest.mark.parametrize("B", [3, 33])
def test_single_frames_are_untouched(amd, B):
    """frame_channels=1 is the plain constructor, bit for bit; cnn_features on (B, H, W) equals the single-frame entry points of the
    raw ABI, bit for bit"""
    from dgvit_amd import functional as F
    hw, kind = (61, 75), "qnet"
    p = R.exact_params(kind, 1, seed=3)
    p.update({k: torch.randn(v.shape, generator=torch.Generator().manual_seed(i)) * 0.1 for i, (k, v) in enumerate(p.items())
              if k.startswith("conv")})                    # ordinary weights: rounding in every sum, so a changed order would show
    frames = torch.rand(B, *hw, generator=torch.Generator().manual_seed(B))
    for kind in ("qnet", "policy"):
        pk = R.exact_params(kind, 1, seed=3)
        pk.update({k: p[k] for k in R.CONV})
        a = _run(_net(amd, kind, 1, pk, frame_channels=1), kind, frames, B)
        b = _run(_net(amd, kind, 1, pk), kind, frames, B)
        assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1])
        assert set(a[2]) == set(b[2]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
        assert a[1].shape == (B, *hw)
    dev = _conv_params(p)
    x = frames.cuda().requires_grad_(True)
    dfeat = torch.randn(B, 256, generator=torch.Generator().manual_seed(9)).cuda()
    feat = F.cnn_features(x, dev)
    (feat * dfeat).sum().backward()
    rfeat, rgrads, rdimg = _raw_old(amd.load_library(), frames.cuda(), [t.detach() for t in dev], dfeat)
    assert torch.equal(feat.detach(), rfeat) and torch.equal(x.grad, rdimg)
    for k, t, g in zip(R.CONV, dev, rgrads):
        assert torch.equal(t.grad, g), k


# ------------------------------------------------------------------------------------------------ 4. conv1 through the window loader
@pytest.mark.parametrize("K", [4, 8, 16])
@pytest.mark.parametrize("hw, B", [((61, 75), 33), ((30, 37), 3)], ids=str)
def test_conv1_through_the_window_loader_equals_im2col(amd, K, hw, B):
    """K % 4 == 0: conv1's forward reads its 5 x 5 x K windows through the GEMM's A-tile loader, as conv2 / conv3 do; same k order, so
    features and every gradient equal the im2col schedule bit for bit (k-slices off, as in test_conv_forward_gather_equals_im2col)"""
    from dgvit_amd import functional as F
    p = R.exact_params("qnet", K, seed=4)
    p.update({k: torch.randn(p[k].shape, generator=torch.Generator().manual_seed(i)) * 0.1 for i, k in enumerate(R.CONV)})
    stack = torch.rand(B, *hw, K, generator=torch.Generator().manual_seed(K + B))
    dfeat = torch.randn(B, 256, generator=torch.Generator().manual_seed(1)).cuda()

    def run(on):
        with knobs(conv_gather=on, gemm_split=0):
            dev = _conv_params(p)
            x = stack.cuda().requires_grad_(True)
            feat = F.cnn_features(x, dev)
            (feat * dfeat).sum().backward()
            torch.cuda.synchronize()
            return [feat.detach(), x.grad] + [t.grad for t in dev]

    a, b = run(1), run(0)
    assert torch.isfinite(a[0]).all() and bool(a[0].any())
    for name, x, y in zip(["features", "frame gradient"] + R.CONV, a, b):
        assert torch.equal(x, y), name


# ------------------------------------------------------------------------------------------------ 5. raw ABI with guard words
def _guarded(n, fill=float("nan")):
    """(whole buffer, the n-float view between two GUARD-float fences)"""
    whole = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    whole[GUARD:GUARD + n] = fill
    return whole, whole[GUARD:GUARD + n]


def _fences_intact(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


def _raw_v2(lib, stack, params, dfeat, grads_wanted=(True,) * 6, want_dimg=True, short=0):
    """dgvit_cnn_forward_v2 / dgvit_cnn_backward_v3 with fences around every buffer the library writes; workspace and scratch start as
    NaN (the column buffer's padded tail among them).  Returns (feat, grads, dimg, fences intact)"""
    from dgvit_amd.functional import _ptr, _stream, _table
    B, H, W, C = stack.shape
    nws, nf, nb = (int(f(B, H, W, C)) for f in (lib.dgvit_cnn_workspace_floats_v2, lib.dgvit_cnn_forward_scratch_floats_v2,
                                                lib.dgvit_cnn_backward_scratch_floats_v2))
    bufs = {"ws": _guarded(nws), "scf": _guarded(nf), "scb": _guarded(nb), "feat": _guarded(B * 256)}
    if want_dimg:
        bufs["dimg"] = _guarded(stack.numel())
    for i, (p, want) in enumerate(zip(params, grads_wanted)):
        if want:
            bufs[f"g{i}"] = _guarded(p.numel())
    v = {k: b[1] for k, b in bufs.items()}
    grads = [v.get(f"g{i}") for i in range(6)]
    rc = lib.dgvit_cnn_forward_v2(_ptr(stack), _table(params), _ptr(v["feat"]), _ptr(v["ws"]), nws, _ptr(v["scf"]), nf - short, B, H, W, C,
                                  _stream())
    if short:
        rcb = lib.dgvit_cnn_backward_v3(_ptr(stack), _table(params), _table(grads), _ptr(dfeat), _ptr(v.get("dimg")), _ptr(v["ws"]), nws,
                                        _ptr(v["scb"]), nb - short, B, H, W, C, _stream())
        return rc, rcb
    assert rc == 0, lib.dgvit_last_error()
    rc = lib.dgvit_cnn_backward_v3(_ptr(stack), _table(params), _table(grads), _ptr(dfeat), _ptr(v.get("dimg")), _ptr(v["ws"]), nws,
                                   _ptr(v["scb"]), nb, B, H, W, C, _stream())
    assert rc == 0, lib.dgvit_last_error()
    torch.cuda.synchronize()
    intact = {k: _fences_intact(whole, view.numel()) for k, (whole, view) in bufs.items()}
    feat = v["feat"].view(B, 256)
    return feat, [None if g is None else g.view_as(p) for g, p in zip(grads, params)], v["dimg"].view_as(stack) if want_dimg else None, intact


@pytest.mark.parametrize("K", [3, 4, 16])
def test_raw_abi_stays_inside_what_the_sizing_functions_return(amd, K):
    hw, B = (30, 37), 3
    lib = amd.load_library()
    p = R.exact_params("qnet", K)
    params = _conv_params(p, grad=False)
    stack = R.exact_stack(B, hw, K).cuda()
    pd = [p[k].double().requires_grad_(True) for k in R.CONV]
    xr = stack.double().cpu().requires_grad_(True)
    w = torch.randn(B, 256, generator=torch.Generator().manual_seed(2))
    ref = R.features(dict(zip(R.CONV, pd)), xr)
    (ref * w.double()).sum().backward()
    feat, grads, dimg, intact = _raw_v2(lib, stack, params, w.cuda())
    assert all(intact.values()), f"written outside its buffer: {[k for k, ok in intact.items() if not ok]}"
    # NaN anywhere in workspace or scratch before the call (the column rows' padded tail included) reaches no output
    assert all(bool(torch.isfinite(t).all()) for t in [feat, dimg] + grads)
    R.check_close(feat, ref, "features")
    for k, g, r in zip(R.CONV, grads, pd):
        R.check_grad(g, r.grad, k)
    assert R.rel_l2(dimg, xr.grad) <= R.DIMG_TOL
    assert not bool(dimg[:, -1].any())
    # a scratch one float short
    assert _raw_v2(lib, stack, params, w.cuda(), short=1) == (-4, -4)        # DGVIT_ERR_WORKSPACE
    assert b"too small" in lib.dgvit_last_error()


# ------------------------------------------------------------------------------------------------ 6. frozen parameters, determinism
@pytest.mark.parametrize("K", [3, 8])
def test_frozen_network_forms_only_the_frame_gradient(amd, K):
    hw, B, kind = (61, 75), 3, "qnet"
    ref = R.reference(kind, hw, K, B)
    m = _net(amd, kind, K, frame_channels=K).requires_grad_(False)
    stack = R.exact_stack(B, hw, K)
    outs, dstack, grads = _run(m, kind, stack, B)
    assert all(g is None for g in grads.values())
    assert dstack.shape == stack.shape and R.rel_l2(dstack, ref["dstack"]) <= R.DIMG_TOL
    again = _run(m, kind, stack, B)
    assert torch.equal(dstack, again[1]) and all(torch.equal(x, y) for x, y in zip(outs, again[0])), "a second pass gives the same bits"
    # the empty batch keeps working: an empty result, zero gradients of the parameters' own shapes
    m.requires_grad_(True)
    q1, q2 = m([torch.zeros(0, *hw, K, device="cuda"), torch.zeros(0, 2, device="cuda"), torch.zeros(0, 2, device="cuda")])
    assert q1.shape == (0, 2)
    (q1.sum() + q2.sum()).backward()
    assert m.conv1.weight.grad.shape == (16, K, 5, 5) and not bool(m.conv1.weight.grad.any())


@pytest.mark.parametrize("K", [3, 4])
def test_null_gradient_slots_are_skipped_and_the_rest_keeps_its_bits(amd, K):
    hw, B = (30, 37), 3
    lib = amd.load_library()
    params = _conv_params(R.exact_params("qnet", K), grad=False)
    stack = R.exact_stack(B, hw, K).cuda()
    dfeat = torch.randn(B, 256, generator=torch.Generator().manual_seed(3)).cuda()
    feat, full, dimg, _ = _raw_v2(lib, stack, params, dfeat)
    subsets = [tuple(j != i for j in range(6)) for i in range(6)] + [(False,) * 6, (True, False) * 3, (False, True) * 3, (True,) * 6]
    for wanted in subsets:
        for want_dimg in (True, False):
            if not want_dimg and wanted not in ((True,) * 6, (False, True) * 3):
                continue
            f2, g2, d2, intact = _raw_v2(lib, stack, params, dfeat, wanted, want_dimg)
            f3, g3, d3, _ = _raw_v2(lib, stack, params, dfeat, wanted, want_dimg)
            assert all(intact.values()) and torch.equal(f2, feat) and torch.equal(f3, feat), wanted
            assert (d2 is None) == (not want_dimg) and (d2 is None or (torch.equal(d2, dimg) and torch.equal(d3, dimg))), wanted
            for i, want in enumerate(wanted):
                assert (g2[i] is not None) == want, (wanted, i)
                if not want:
                    continue
                assert torch.equal(g2[i], g3[i]), f"{wanted}: a second pass gives other bits in slot {i}"
                if i % 2 == 1 and not wanted[i - 1]:
                    # a bias gradient without its weight gradient is the column-sum kernel alone, not the sums fused into the
                    # weight-gradient GEMM: another order of the same sum
                    R.check_grad(g2[i], full[i], f"{wanted}: slot {i}")
                else:
                    assert torch.equal(g2[i], full[i]), (wanted, i)


# ------------------------------------------------------------------------------------------------ 7. end to end
def test_ring_samples_and_pushed_stacks_go_through_the_cnn_networks(amd):
    from dgvit_amd.replay import DeviceReplayBuffer, FrameStack
    E, K, shape, T = 2, 3, (29, 29), 6
    g = torch.Generator().manual_seed(11)
    buf = DeviceReplayBuffer(32, obs_shape=shape, seed=1, num_envs=E)
    fs = FrameStack(num_envs=E, obs_shape=shape, frames=K, device="cuda")
    pol = _net(amd, "policy", K, frame_channels=K)
    qn = _net(amd, "qnet", K, frame_channels=K)
    obs = torch.randint(0, 4, (E, *shape), generator=g).float().cuda()
    for t in range(T):
        pstate = torch.rand(E, 2, generator=g).cuda()
        pushed = fs.push(obs, reset=None if t else True)
        assert pushed.shape == (E, *shape, K)
        with torch.no_grad():
            action, log_prob, mean = pol.sample([pushed, pstate])
        assert action.shape == (E, 2) and log_prob.shape == (E, 1) and all(bool(torch.isfinite(v).all()) for v in (action, log_prob, mean))
        nxt = torch.randint(0, 4, (E, *shape), generator=g).float().cuda()
        buf.add_vec(obs=obs, pobs=pstate, act=action, rew=torch.zeros(E, 1, device="cuda"), next_obs=nxt,
                    next_pobs=torch.rand(E, 2, generator=g).cuda(), done=torch.zeros(E, 1, device="cuda"))
        obs = nxt
    batch = buf.sample(8, frame_stack=K)
    assert batch["obs"].shape == (8, *shape, K) and batch["obs"].is_contiguous()
    q1, q2 = qn([batch["obs"], batch["pobs"], batch["act"]])
    mean, log_std = pol([batch["next_obs"], batch["next_pobs"]])
    assert q1.shape == q2.shape == (8, 2) and mean.shape == log_std.shape == (8, 2)
    assert all(bool(torch.isfinite(v).all()) for v in (q1, q2, mean, log_std))
    (q1.sum() + q2.sum()).backward()
    assert qn.conv1.weight.grad.shape == (16, K, 5, 5) and bool(torch.isfinite(qn.conv1.weight.grad).all())
    # parity of q1 with fp64 on the sampled bytes
    pd = {k: v.double() for k, v in R.exact_params("qnet", K).items()}
    r1, _ = R.forward("qnet", pd, batch["obs"].double().cpu(), batch["pobs"].double().cpu(), batch["act"].double().cpu())
    R.check_close(q1, r1, "q1")
