"""GPU: the last block with K and V folded into token 0's query (csrc/last_block.hip).

Operator level: dgvit_goal_attention_forward / _backward against torch fp64 on the same fp32 inputs, with the error of the unfolded
route the library already has (K / V by the fp32 GEMM, then the one-query attention) as the yardstick: the folded result may err by at
most twice that, per output, both scaled by the output's largest magnitude.  Encoder level: the default schedule against
dense_last_block=True at the tolerances of test_gpu_parity.py::test_last_block_token0_schedule_equals_dense; the fallbacks; bit-equal
reruns and graph replay; the diagnostic knob."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from helpers import O

pytestmark = pytest.mark.gpu

OUT_ATOL = 2e-6     # outputs against the dense schedule            (test_last_block_token0_schedule_equals_dense)
GRAD_REL = 2e-4     # gradients, relative to the gradient's max     (the same test)


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ operator level
def _op_inputs(B, N, H, dh, D):
    g = torch.Generator().manual_seed(7919 * B + 131 * N + 17 * H + dh + D)
    I = H * dh
    x = torch.randn(B, N, D, generator=g)
    ln_w = 1.0 + 0.1 * torch.randn(D, generator=g)
    ln_b = 0.1 * torch.randn(D, generator=g)
    xn = torch.nn.functional.layer_norm(x, (D,), ln_w, ln_b)
    w = O.make_params([("to_qkv.weight", (3 * I, D), "xavier")], 31)["to_qkv.weight"]
    q = xn[:, 0] @ w[:I].T                                   # token 0's query, an input of both routes
    dout = torch.randn(B, I, generator=g)
    return xn.contiguous(), w.contiguous(), q.contiguous(), dout


def _ref64(xn, w, q, dout, H, dh):
    B, N, D = xn.shape
    I = H * dh
    xn64, w64, q64 = xn.double().requires_grad_(True), w.double().requires_grad_(True), q.double().requires_grad_(True)
    k = (xn64 @ w64[I:2 * I].T).view(B, N, H, dh)
    v = (xn64 @ w64[2 * I:].T).view(B, N, H, dh)
    s = torch.einsum("bhd,bnhd->bhn", q64.view(B, H, dh), k) * dh ** -0.5
    o = torch.einsum("bhn,bnhd->bhd", s.softmax(-1), v).reshape(B, I)
    o.backward(dout.double())
    return {"o": o.detach(), "dq": q64.grad, "dxn": xn64.grad, "dwkv": w64.grad[I:]}


def _folded(lib, xn, w, q, dout, H, dh):
    B, N, D = xn.shape
    I = H * dh
    xn, w, q, dout = (t.cuda() for t in (xn, w, q, dout))
    u, r = torch.full((B, H, D), 7.0, device="cuda"), torch.full((B, H, D), 7.0, device="cuda")
    p, o = torch.full((B, H, N), 7.0, device="cuda"), torch.full((B, I), 7.0, device="cuda")
    assert lib.dgvit_goal_attention_forward(_ptr(xn), _ptr(w), _ptr(q), I, _ptr(o), I, _ptr(u), _ptr(r), _ptr(p), B, N, H, dh, D,
                                            _stream()) == 0, lib.dgvit_last_error()
    dq, dxn = torch.full((B, I), 7.0, device="cuda"), torch.full((B, N, D), 7.0, device="cuda")
    dwkv = torch.full((2 * I, D), 7.0, device="cuda")
    nsc = lib.dgvit_goal_attention_scratch_floats(B, H, D)
    assert nsc == 2 * B * H * D
    sc = torch.empty(nsc, device="cuda")
    assert lib.dgvit_goal_attention_backward(_ptr(xn), _ptr(w), _ptr(q), I, _ptr(dout), I, _ptr(u), _ptr(r), _ptr(p), _ptr(dq), I, _ptr(dxn),
                                             _ptr(dwkv), _ptr(sc), nsc, B, N, H, dh, D, _stream()) == 0, lib.dgvit_last_error()
    torch.cuda.synchronize()
    np.testing.assert_allclose(p.sum(-1).cpu().numpy(), 1.0, rtol=0, atol=1e-5)
    return {"o": o.cpu(), "dq": dq.cpu(), "dxn": dxn.cpu(), "dwkv": dwkv.cpu()}


def _unfolded(amd, xn, w, q, dout, H, dh):
    """K / V by the library's fp32 GEMM, the one-query attention kernels, and the GEMMs' data / weight gradients"""
    from dgvit_amd import functional as F
    B, N, D = xn.shape
    I = H * dh
    with amd.diagnostic_library() as lib:
        x2 = xn.cuda().view(B * N, D).requires_grad_(True)
        wkv = w[I:].cuda().requires_grad_(True)
        kv = F.linear(x2, wkv)
        qkv = torch.zeros(B, N, 3 * I, device="cuda")
        qkv[:, :, I:] = kv.detach().view(B, N, 2 * I)
        qkv[:, 0, :I] = q.cuda()
        out, lse = torch.zeros(B, N, I, device="cuda"), torch.zeros(B, H, N, device="cuda")
        assert lib.dgvit_attention_forward_queries(_ptr(qkv), _ptr(out), _ptr(lse), B, N, H, dh, 1, _stream()) == 0, lib.dgvit_last_error()
        do = torch.zeros(B, N, I, device="cuda")
        do[:, 0] = dout.cuda()
        dqkv = torch.zeros_like(qkv)
        assert lib.dgvit_attention_backward_queries(_ptr(qkv), _ptr(out), _ptr(do), _ptr(lse), _ptr(dqkv), B, N, H, dh, 1,
                                                    _stream()) == 0, lib.dgvit_last_error()
        kv.backward(dqkv[:, :, I:].reshape(B * N, 2 * I).contiguous())
        torch.cuda.synchronize()
        return {"o": out[:, 0].cpu(), "dq": dqkv[:, 0, :I].cpu(), "dxn": x2.grad.view(B, N, D).cpu(), "dwkv": wkv.grad.cpu()}


@pytest.mark.parametrize("H,dh,D", [(8, 64, 256), (4, 64, 64), (4, 32, 64), (1, 64, 64)])
@pytest.mark.parametrize("N", [2, 21, 50, 81])
@pytest.mark.parametrize("B", [1, 5, 37, 65])
def test_goal_attention_against_fp64_within_twice_the_unfolded_error(amd, B, N, H, dh, D):
    xn, w, q, dout = _op_inputs(B, N, H, dh, D)
    ref = _ref64(xn, w, q, dout, H, dh)
    fold = _folded(amd.load_library(), xn, w, q, dout, H, dh)
    unf = _unfolded(amd, xn, w, q, dout, H, dh)
    fails = []
    for k in ("o", "dq", "dxn", "dwkv"):
        scale = ref[k].abs().max().item()
        ef = (fold[k].double() - ref[k]).abs().max().item() / scale
        eu = (unf[k].double() - ref[k]).abs().max().item() / scale
        print(f"goal_attention B={B} N={N} H={H} dh={dh} D={D} {k}: max|{k}|={scale:.3e} folded {ef:.3e} unfolded {eu:.3e} ratio {ef / max(eu, 1e-30):.2f}")
        assert eu < 1e-4, (k, eu)      # the yardstick itself is a correct fp32 route
        if not ef <= 2.0 * eu:
            fails.append((k, ef, eu))
    assert not fails, fails


def test_goal_attention_refuses_what_it_cannot_run(amd):
    lib = amd.load_library()
    t = torch.zeros(64, device="cuda")
    args = lambda N, dh, D: (_ptr(t), _ptr(t), _ptr(t), 64, _ptr(t), 64, _ptr(t), _ptr(t), None, 1, N, 1, dh, D, _stream())
    assert lib.dgvit_goal_attention_forward(*args(1 << 20, 64, 64)) != 0 and b"LDS" in lib.dgvit_last_error()
    assert lib.dgvit_goal_attention_forward(*args(4, 48, 64)) != 0
    assert lib.dgvit_goal_attention_forward(*args(4, 64, 66)) != 0
    assert lib.dgvit_goal_attention_scratch_floats(0, 1, 64) < 0


# ------------------------------------------------------------------------------------------------ encoder level
def _launches(lib, fn):
    """profile counters (launches per kind; kind 0 = fp32 GEMM) of fn()"""
    from dgvit_amd import _lib
    torch.cuda.synchronize()
    lib.dgvit_profile_sampling(1)
    assert lib.dgvit_profile_start(8192) == 0
    fn()
    torch.cuda.synchronize()
    kinds = _lib.PROFILE_KINDS
    ms, work, cnt = (ctypes.c_double * kinds)(), (ctypes.c_double * kinds)(), (ctypes.c_longlong * kinds)()
    assert lib.dgvit_profile_stop(ms, work, cnt) == 0
    return list(cnt)


def _folds(amd, m, batch, lkeep=1.0, maps=0):
    from dgvit_amd._lib import dgvit_config
    trans = getattr(m, "trans", m)
    return amd.load_library().dgvit_got_last_block_folds(ctypes.byref(dgvit_config(*trans._cfg)), batch, lkeep, maps)


def _policy(amd, cfg, seed):
    m = amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    m.load_state_dict(O.make_params(O.policy_param_spec(cfg), seed), strict=True)
    return m.cuda().eval()


def _got(amd, cfg, seed, pool="cls", dropout=0.0, train=False):
    m = amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=cfg.num_classes, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads,
                mlp_dim=cfg.mlp_dim, channels=1, dim_head=cfg.dim_head, pool=pool, dropout=dropout)
    m.load_state_dict(O.make_params(O.got_param_spec(cfg, prefix=""), seed), strict=True)
    m = m.cuda().train(train)
    m.draw_dropout_seed = lambda: 1234
    return m


def _policy_step(m, img, pstate):
    m.zero_grad()
    mean, log_std = m([img, pstate])
    ((mean ** 2).mean() + (log_std ** 2).mean()).backward()
    torch.cuda.synchronize()
    return [mean.detach().clone(), log_std.detach().clone()], {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def _got_step(m, img, goal, w, image_grad=False):
    for q in m.parameters():
        q.grad = None
    x = img.clone().requires_grad_(image_grad)
    g = goal.clone().requires_grad_(True)
    feat = m(x, g)
    (feat * w).sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    grads["<goal>"] = g.grad.clone()
    if image_grad:
        grads["<image>"] = x.grad.clone()
    return [feat.detach().clone()], grads


def _assert_same(got, want, what=""):
    (outs, grads), (outs_d, grads_d) = got, want
    for a, b in zip(outs, outs_d):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=OUT_ATOL, err_msg=what)
    assert grads.keys() == grads_d.keys()
    for k in grads_d:
        scale = max(grads_d[k].abs().max().item(), 1e-8)
        err = (grads_d[k] - grads[k]).abs().max().item()
        assert err <= GRAD_REL * scale + 1e-9, (what, k, err, scale)


def _got_inputs(cfg, B, seed):
    img, _, _, _ = O.make_inputs(cfg, B, seed)
    goal = torch.randn(B, cfg.dim, generator=torch.Generator().manual_seed(seed + 1))
    w = torch.randn(B, cfg.dim, generator=torch.Generator().manual_seed(seed + 2))
    return img.cuda(), goal.cuda(), w.cuda()


C3 = dict(image=(84, 84), patch=(12, 12), dim=256, depth=2, heads=8)
POLICY_CASES = {
    "c3_b1": (O.GoTConfig(**C3), 1),
    "c3_b37": (O.GoTConfig(**C3), 37),
    "shipped_b5": (O.GoTConfig(), 5),                                   # L4 / H4 / D64 on 128 x 160: LayerNorms in the GEMM epilogues
    "noproj_b5": (O.GoTConfig(depth=2, heads=1, dim=64), 5),            # GoTPolicy(2, 2, 2, 1, 64): to_out = Identity
}


@pytest.mark.parametrize("overlap", [False, True], ids=["one_stream", "wgrad_overlap"])
@pytest.mark.parametrize("case", list(POLICY_CASES))
def test_policy_folded_last_block_equals_dense(amd, case, overlap):
    cfg, B = POLICY_CASES[case]
    m = _policy(amd, cfg, 31)
    assert _folds(amd, m, B) == 1
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, B, 31))
    m.trans.set_schedule(dense_last_block=True, wgrad_overlap=overlap)
    dense = _policy_step(m, img, pstate)
    m.trans.set_schedule(dense_last_block=False, wgrad_overlap=overlap)
    _assert_same(_policy_step(m, img, pstate), dense, case)
    with torch.no_grad():                                               # a no-grad forward keeps the K / V GEMM; it equals dense as before
        m.trans.set_schedule(dense_last_block=True, wgrad_overlap=overlap)
        want = m([img, pstate])
        m.trans.set_schedule(dense_last_block=False, wgrad_overlap=overlap)
        got = m([img, pstate])
    for a, b in zip(got, want):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=0, atol=OUT_ATOL)


@pytest.mark.parametrize("overlap", [False, True], ids=["one_stream", "wgrad_overlap"])
@pytest.mark.parametrize("case", ["c3_b37", "shipped_b5", "noproj_b5"])
def test_got_folded_last_block_equals_dense_with_the_frame_gradient(amd, case, overlap):
    cfg, B = POLICY_CASES[case]
    m = _got(amd, cfg, 33)
    img, goal, w = _got_inputs(cfg, B, 33)
    m.set_schedule(dense_last_block=True, wgrad_overlap=overlap)
    dense = _got_step(m, img, goal, w, image_grad=True)
    m.set_schedule(dense_last_block=False, wgrad_overlap=overlap)
    _assert_same(_got_step(m, img, goal, w, image_grad=True), dense, case)


def test_folded_last_block_drops_three_gemm_launches_and_the_knob_agrees(amd):
    """Through the diagnostic library: fold off and fold on agree at the encoder tolerances, and the fold removes exactly the K / V GEMM
    of the forward and the dW_kv and dkv W_kv GEMMs of the backward (profile kind 0)."""
    cfg, B = POLICY_CASES["c3_b37"]
    m = _policy(amd, cfg, 35)
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, B, 35))
    res, cnt = {}, {}
    with amd.diagnostic_library() as lib:
        try:
            for on in (0, 1):
                lib.dgvit_set_last_block_fold(on)
                _policy_step(m, img, pstate)
                cnt[on] = _launches(lib, lambda: res.__setitem__(on, _policy_step(m, img, pstate)))
        finally:
            lib.dgvit_set_last_block_fold(1)
    _assert_same(res[1], res[0], "knob")
    assert cnt[0][0] - cnt[1][0] == 3, (cnt[0], cnt[1])
    # the product library runs what the diagnostic library runs with the knob at its default
    assert _launches(amd.load_library(), lambda: _policy_step(m, img, pstate))[0] == cnt[1][0]


def _gemm_launches_per_knob(amd, fn):
    cnt = {}
    with amd.diagnostic_library() as lib:
        try:
            for on in (0, 1):
                lib.dgvit_set_last_block_fold(on)
                fn()
                cnt[on] = _launches(lib, fn)[0]
        finally:
            lib.dgvit_set_last_block_fold(1)
    return cnt


@pytest.mark.parametrize("variant", ["lds_budget", "pool_mean", "layer_dropout", "maps", "no_grad"])
def test_fallbacks_keep_the_kv_gemm_and_equal_dense(amd, variant):
    """Where the fold does not apply the K / V GEMM launch is still there (as many kind-0 launches with the knob on as with it off) and
    the result equals the dense schedule."""
    if variant == "lds_budget":         # 257 tokens x 256 floats = 263 KB per frame
        cfg, B = O.GoTConfig(image=(224, 224), patch=(14, 14), dim=256, depth=2, heads=8, mlp_dim=256), 2
    else:   # (64 frames: a no-grad forward of this size runs the GEMM schedule, not the two-launch blocks)
        cfg, B = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=4, mlp_dim=128), 64 if variant == "no_grad" else 5
    pool = "mean" if variant == "pool_mean" else "cls"
    p = 0.3 if variant == "layer_dropout" else 0.0
    m = _got(amd, cfg, 37, pool=pool, dropout=p, train=variant == "layer_dropout")
    img, goal, w = _got_inputs(cfg, B, 37)
    if variant != "no_grad":        # (the query speaks for training forwards and maps calls)
        assert _folds(amd, m, B, lkeep=1.0 - p, maps=int(variant == "maps")) == 0
    if variant in ("lds_budget", "maps"):
        assert _folds(amd, _got(amd, O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=4, mlp_dim=128), 37), B) == 1
    if variant == "maps":
        run = lambda: [t.clone() for t in m.attention_maps(img, goal, rows="goal")]
        m.set_schedule(dense_last_block=True)
        want = run()
        m.set_schedule(dense_last_block=False)
        got = run()
        np.testing.assert_allclose(got[0].cpu().numpy(), want[0].cpu().numpy(), rtol=0, atol=OUT_ATOL)
        np.testing.assert_allclose(got[1].cpu().numpy(), want[1].cpu().numpy(), rtol=0, atol=OUT_ATOL)
        cnt = _gemm_launches_per_knob(amd, run)
    elif variant == "no_grad":
        def run():
            with torch.no_grad():
                return m(img, goal).clone()
        m.set_schedule(dense_last_block=True)
        want = run()
        m.set_schedule(dense_last_block=False)
        got = run()
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=OUT_ATOL)
        assert torch.equal(got, m.attention_maps(img, goal, rows="goal")[0])      # bit for bit the features of a maps call
        cnt = _gemm_launches_per_knob(amd, run)
    else:
        m.set_schedule(dense_last_block=True)
        dense = _got_step(m, img, goal, w)
        m.set_schedule(dense_last_block=False)
        _assert_same(_got_step(m, img, goal, w), dense, variant)
        cnt = _gemm_launches_per_knob(amd, lambda: _got_step(m, img, goal, w))
    assert cnt[0] == cnt[1] and cnt[1] > 0, cnt


def test_two_runs_give_the_same_bits(amd):
    cfg, B = POLICY_CASES["c3_b37"]
    m = _policy(amd, cfg, 39)
    m.trans.set_schedule(wgrad_overlap=True)
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, B, 39))
    (o1, g1), (o2, g2) = _policy_step(m, img, pstate), _policy_step(m, img, pstate)
    assert all(torch.equal(a, b) for a, b in zip(o1, o2))
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_graph_replay_of_a_train_step_equals_eager(amd):
    """B = 32: (a) a captured forward + backward replays to the bits of the eager one; (b) a captured training step (with FlatAdam)
    tracks eager training as test_gpu_parity.py::test_graphed_training_step asks."""
    from dgvit_amd.optim import FlatAdam
    cfg = O.GoTConfig(**C3)
    base = _policy(amd, cfg, 41)
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, 32, 41))
    assert _folds(amd, base, 32) == 1
    m = copy.deepcopy(base)
    eager_out, eager = _policy_step(m, img, pstate)

    def fb():
        m.zero_grad(set_to_none=False)
        mean, log_std = m([img, pstate])
        ((mean ** 2).mean() + (log_std ** 2).mean()).backward()
        return mean.detach()
    g = amd.GraphedStep(fb, warmup=2)
    mean = g().clone()
    torch.cuda.synchronize()
    assert torch.equal(mean, eager_out[0])
    for k, p in m.named_parameters():
        if p.grad is not None:
            assert torch.equal(p.grad, eager[k]), k

    def make(model):
        opt = FlatAdam([model], lr=1e-3, capturable=True)

        def step():
            opt.zero_grad(set_to_none=True)
            mean, log_std = model([img, pstate])
            loss = (mean ** 2).mean() + (log_std ** 2).mean()
            loss.backward()
            opt.step()
            return loss.detach()
        return step
    ma, mb = copy.deepcopy(base), copy.deepcopy(base)
    step_a, step_b = make(ma), make(mb)
    gs = amd.GraphedStep(step_b, warmup=3)
    for _ in range(3):
        step_a()
    for _ in range(3):
        la, lb = step_a(), gs()
    torch.cuda.synchronize()
    assert abs(la.item() - lb.item()) <= 1e-6 * max(1.0, abs(la.item()))
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=k)
