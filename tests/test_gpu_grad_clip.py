"""GPU: gradient-norm clipping on the flat buffers -- the four C entry points, FlatAdam(max_grad_norm=...) and
optim.clip_grad_norm_ against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.

Reference for norms: fp64 on the host from the same fp32 gradients.  Tolerance for a returned norm: 1e-6 relative -- the sum is formed
in double and rounded once to fp32 (2^-24, about 6e-8); the margin covers the square root and the 1e-6 term."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O, need_device_memory  # noqa: E402

NORM_RTOL = 1e-6
ADAM_TOL = dict(rtol=2e-5, atol=2e-6)      # test_flat_adam_matches_torch_adam's


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


def _P():
    from dgvit_amd import _lib as L
    return L.GRAD_NORM_PARTIALS


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan_scratch():
    """partials and the two output floats, pre-filled with NaN bit patterns: nothing may rely on zeroed scratch"""
    buf = torch.full((_P() + 1,), float("nan"), dtype=torch.float64, device="cuda")
    return buf, buf[_P():].view(torch.float32)


def _measure(bufs, max_norm, scratch=None):
    """dgvit_grad_sqnorm_partials over ``bufs`` (accumulate 0, 1, 1, ...) + dgvit_grad_clip_coef -> (scratch, out)"""
    from dgvit_amd import _lib as L
    lib = L.load()
    buf, out = scratch if scratch is not None else _nan_scratch()
    for k, g in enumerate(bufs):
        L.check(lib.dgvit_grad_sqnorm_partials(_p(g), g.numel(), _p(buf), int(k > 0), _stream()), "dgvit_grad_sqnorm_partials")
    L.check(lib.dgvit_grad_clip_coef(_p(buf), max_norm, _p(out), _stream()), "dgvit_grad_clip_coef")
    return buf, out


def _wide(n, seed):
    """N(0,1) times a per-element scale spanning 1e-6 ... 1e3"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, device="cuda", generator=gen) * 9.0 - 6.0)
    return torch.randn(n, device="cuda", generator=gen) * mag


def _norm64(tensors):
    return math.sqrt(sum(float((t.detach().double().cpu() ** 2).sum()) for t in tensors))


def _sizes():
    full = 4 * _P() * 256
    return [4, 1020, 1024, 1028, full - 4, full, full + 4, 2 * full + 12]


# ------------------------------------------------------------------------------------------------ 1. C ABI, sizes
@pytest.mark.parametrize("which", range(8))
def test_norm_at_the_grid_edges(amd, which):
    """one float4, the workgroup edges, exactly one grid pass, the grid-stride tail; NaN-filled scratch; twice bit-identical"""
    n = _sizes()[which]
    g = _wide(n, 100 + which)
    ref = _norm64([g])
    buf, out = _measure([g], 1.0)
    assert not torch.isnan(buf[:_P()]).any(), "a partial slot was not written"
    got = out[0].item()
    print(f"n={n} norm {got!r} ref {ref!r} rel {abs(got - ref) / ref:.3e}")
    assert abs(got - ref) <= NORM_RTOL * ref
    first = (buf.clone(), out.clone())
    buf2, out2 = _measure([g], 1.0)
    assert torch.equal(first[0][:_P()], buf2[:_P()]) and torch.equal(first[1].view(torch.int32), out2.view(torch.int32))
    _measure([g], 1.0, scratch=(buf, out))           # and re-using a scratch that holds the previous result
    assert torch.equal(first[0][:_P()], buf[:_P()]) and torch.equal(first[1].view(torch.int32), out.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 2. accumulate
def test_accumulate_gives_the_norm_of_the_concatenation(amd):
    bufs = [_wide(n, 200 + i) for i, n in enumerate((1028, 4 * _P() * 256 + 4, 4100))]
    ref = _norm64(bufs)
    _, out = _measure(bufs, 1.0)
    got = out[0].item()
    print(f"norm {got!r} ref {ref!r} rel {abs(got - ref) / ref:.3e}")
    assert abs(got - ref) <= NORM_RTOL * ref
    _, single = _measure([torch.cat(bufs)], 1.0)
    assert abs(single[0].item() - ref) <= NORM_RTOL * ref


# ------------------------------------------------------------------------------------------------ 3. coefficient
@pytest.mark.parametrize("frac", [0.25, 0.7, 0.013, 0.999])
def test_coefficient_is_torchs_expression_bit_for_bit(amd, frac):
    g = _wide(4100, 300)
    max_norm = float(torch.tensor(frac * _norm64([g]), dtype=torch.float32))      # representable in fp32: the C ABI takes a float
    _, out = _measure([g], max_norm)
    want = max_norm / (out[0:1].clone() + 1e-6)                                    # torch's line, in fp32 on the device
    print(f"frac {frac} coef {out[1].item()!r} torch {want.item()!r}")
    assert want.dtype == torch.float32 and want.item() < 1.0
    assert torch.equal(out[1:2].view(torch.int32), want.view(torch.int32))


def test_coefficient_clamps_and_propagates_non_finite_norms(amd):
    g = _wide(4100, 301)
    _, out = _measure([g], 100.0 * _norm64([g]))
    assert out[1].item() == 1.0
    bad = g.clone()
    bad[1234] = float("nan")
    _, out = _measure([bad], 1.0)
    assert math.isnan(out[0].item()) and math.isnan(out[1].item())
    bad[1234] = float("inf")
    _, out = _measure([bad], 1.0)
    assert out[0].item() == math.inf and out[1].item() == 0.0


# ------------------------------------------------------------------------------------------------ 4. scaled Adam
@pytest.mark.parametrize("scale", [0.37, 1.0])
@pytest.mark.parametrize("step_on_device", [False, True])
def test_scaled_adam_equals_adam_on_a_prescaled_gradient(amd, scale, step_on_device):
    from dgvit_amd import _lib as L
    lib = L.load()
    n = 4100
    gen = torch.Generator(device="cuda").manual_seed(400)
    init = [torch.randn(n, device="cuda", generator=gen), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    a, b = [t.clone() for t in init], [t.clone() for t in init]
    s = torch.tensor([scale], dtype=torch.float32, device="cuda")
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    for t in (1, 2, 3):
        g = _wide(n, 400 + t)
        g2 = g * s                                        # torch fp32: one rounding per element
        step_dev.fill_(t)
        sp = _p(step_dev) if step_on_device else None
        hyper = (n, 3e-3, 0.9, 0.999, 1e-3, 0.01, t, sp)
        L.check(lib.dgvit_adam_step_scaled(_p(a[0]), _p(g), _p(a[1]), _p(a[2]), *hyper, _p(s), _stream()), "dgvit_adam_step_scaled")
        L.check(lib.dgvit_adam_step(_p(b[0]), _p(g2 if scale != 1.0 else g), _p(b[1]), _p(b[2]), *hyper, _stream()), "dgvit_adam_step")
        for x, y, name in zip(a, b, "pmv"):
            assert torch.equal(x, y), f"{name} differs at step {t}"
    assert not torch.equal(a[0], init[0])


# ------------------------------------------------------------------------------------------------ 5. scale kernel
@pytest.mark.parametrize("which", range(3))
def test_scale_by_device_scalar_is_torchs_product(amd, which):
    from dgvit_amd import _lib as L
    n = [4, 1028, 4 * _P() * 256 + 4][which]
    x = _wide(n, 500 + which)
    s = torch.tensor([0.3137], dtype=torch.float32, device="cuda")
    want = x * s
    L.check(L.load().dgvit_scale_by_device_scalar(_p(x), n, _p(s), _stream()), "dgvit_scale_by_device_scalar")
    assert torch.equal(x, want)


# ------------------------------------------------------------------------------------------------ 6. FlatAdam(max_grad_norm) against torch
def _policy(amd, seed=51):
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2)
    m = amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    m.load_state_dict(O.make_params(O.policy_param_spec(cfg), seed), strict=True)
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, 16, seed))
    return m.cuda().eval(), img, pstate


def _loss(m, img, pstate, it):
    mean, log_std = m([img, pstate])
    return (mean ** 2).mean() + (log_std ** 2).mean() * (it + 1)


def _grads(params):
    return [p.grad for p in params if p.grad is not None]


HYPER = dict(lr=3e-3, weight_decay=0.01, eps=1e-3)


def test_flat_adam_with_max_grad_norm_matches_clip_then_torch_adam(amd):
    from dgvit_amd.optim import FlatAdam, home_of
    base, img, pstate = _policy(amd)
    probe = copy.deepcopy(base)
    _loss(probe, img, pstate, 0).backward()
    norm0 = _norm64(_grads(probe.parameters()))
    max_norm = 0.25 * norm0                       # a quarter of the first step's unclipped norm
    a, b, c, d, e = (copy.deepcopy(base) for _ in range(5))
    oa = FlatAdam([a], max_grad_norm=max_norm, **HYPER)
    ob = torch.optim.Adam(b.parameters(), **HYPER)             # reference: torch clip, then torch Adam
    oc = torch.optim.Adam(c.parameters(), **HYPER)             # NOT clipped: must end up somewhere else
    od = FlatAdam([d], max_grad_norm=100.0 * norm0, **HYPER)   # never clips
    oe = FlatAdam([e], **HYPER)
    assert oa.last_grad_norm is None
    for it in range(3):
        for m, o in ((a, oa), (b, ob), (c, oc), (d, od), (e, oe)):
            o.zero_grad(set_to_none=True)
            _loss(m, img, pstate, it).backward()
        ref_b = _norm64(_grads(b.parameters()))
        assert ref_b > max_norm, "this step would not clip"
        before = [(p, p.grad.clone()) for p in a.parameters() if p.grad is not None]
        ref_a = _norm64([g for _, g in before])
        torch.nn.utils.clip_grad_norm_(b.parameters(), max_norm)
        for o in (oa, ob, oc, od, oe):
            o.step()
        got = oa.last_grad_norm
        assert got.dim() == 0 and got.is_cuda and got.dtype == torch.float32
        print(f"step {it}: last_grad_norm {got.item()!r} fp64 of the same gradients {ref_a!r} reference's {ref_b!r}")
        assert abs(got.item() - ref_a) <= NORM_RTOL * ref_a
        if it == 0:                               # identical parameters, identical kernels: the reference's norm too
            assert abs(got.item() - ref_b) <= NORM_RTOL * ref_b
        for p, g in before:
            assert torch.equal(p.grad, g), ".grad was modified by the clipped step"
    home = home_of(a)
    enc = sum((p.numel() + 3) & ~3 for p in a.trans.param_table())
    assert home.zero_copy_elems == 3 * enc, "encoder gradients should have been consumed in place (zero copy), once per step"
    far = total = 0
    for (k, pa), (_, pb), (_, pc) in zip(a.named_parameters(), b.named_parameters(), c.named_parameters()):
        xa, xb, xc = (t.detach().cpu().numpy() for t in (pa, pb, pc))
        np.testing.assert_allclose(xa, xb, err_msg=k, **ADAM_TOL)
        if pb.grad is not None:
            far += int((np.abs(xc - xb) > 100 * (ADAM_TOL["atol"] + ADAM_TOL["rtol"] * np.abs(xb))).sum())
            total += xb.size
    print(f"unclipped torch Adam differs from the clipped reference beyond 100 x tolerance in {far} of {total} entries")
    assert far >= total / 2, "clipping hardly changes the result: the comparison above shows nothing"
    for (k, pd), (_, pe) in zip(d.named_parameters(), e.named_parameters()):
        assert torch.equal(pd, pe), f"{k}: a coefficient of 1 must leave the step bit-identical"
    assert od.last_grad_norm.item() > 0


# ------------------------------------------------------------------------------------------------ 7. sub-sets and several homes
def test_clipped_step_over_a_module_and_loose_tensors(amd):
    from dgvit_amd.optim import FlatAdam

    def make():
        torch.manual_seed(7)
        lin = torch.nn.Linear(8, 4).cuda()
        log_alpha = torch.zeros(1, device="cuda", requires_grad=True)
        unused = torch.nn.Parameter(torch.ones(5, device="cuda"))          # never gets a gradient
        return lin, log_alpha, unused

    base, img, pstate = _policy(amd, 52)
    x = torch.randn(16, 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(8))
    pa, (lin_a, la_a, un_a) = copy.deepcopy(base), make()
    pb, (lin_b, la_b, un_b) = copy.deepcopy(base), make()

    def loss(pol, lin, la, it):
        return _loss(pol, img, pstate, it) + (lin(x) ** 2).mean() * 3.0 + (la * 2.5 * (it + 1)).sum()

    list_a = [*lin_a.parameters(), la_a, un_a]
    list_b = [*pb.parameters(), *lin_b.parameters(), la_b, un_b]
    loss(pa, lin_a, la_a, 0).backward()
    max_norm = 0.25 * _norm64(_grads([*pa.parameters(), *list_a]))
    oa = FlatAdam([pa, *list_a], max_grad_norm=max_norm, **HYPER)
    ob = torch.optim.Adam(list_b, **HYPER)
    for it in range(3):
        oa.zero_grad(set_to_none=True)
        ob.zero_grad(set_to_none=True)
        loss(pa, lin_a, la_a, it).backward()
        loss(pb, lin_b, la_b, it).backward()
        ref = _norm64(_grads(list_b))
        theirs = torch.nn.utils.clip_grad_norm_(list_b, max_norm)
        oa.step()
        ob.step()
        print(f"step {it}: last_grad_norm {oa.last_grad_norm.item()!r} fp64 {ref!r} torch {theirs.item()!r}")
        if it == 0:                               # identical parameters, identical kernels: the norm torch saw
            assert abs(oa.last_grad_norm.item() - ref) <= NORM_RTOL * ref
        ref_a = _norm64(_grads([*pa.parameters(), *list_a]))      # (.grad is left as it was by the clipped step)
        assert abs(oa.last_grad_norm.item() - ref_a) <= NORM_RTOL * ref_a
    assert un_a.grad is None and torch.equal(un_a, un_b)
    mine = [*pa.parameters(), *lin_a.parameters(), la_a]
    torchs = [*pb.parameters(), *lin_b.parameters(), la_b]
    for i, (x_a, x_b) in enumerate(zip(mine, torchs)):
        np.testing.assert_allclose(x_a.detach().cpu().numpy(), x_b.detach().cpu().numpy(), err_msg=str(i), **ADAM_TOL)
    assert not torch.equal(la_a.detach(), torch.zeros_like(la_a))


# ------------------------------------------------------------------------------------------------ 8. stand-alone clip_grad_norm_
def test_clip_grad_norm_matches_torchs(amd):
    from dgvit_amd.optim import FlatAdam, clip_grad_norm_, home_of
    base, img, pstate = _policy(amd, 53)
    a, b = copy.deepcopy(base), copy.deepcopy(base)
    _loss(a, img, pstate, 0).backward()
    _loss(b, img, pstate, 0).backward()
    ref = _norm64(_grads(b.parameters()))
    max_norm = 0.25 * ref
    mine = clip_grad_norm_(a, max_norm)
    theirs = torch.nn.utils.clip_grad_norm_(b.parameters(), max_norm)
    print(f"norm {mine.item()!r} fp64 {ref!r} torch {theirs.item()!r}")
    assert mine.dim() == 0 and mine.is_cuda
    assert abs(mine.item() - ref) <= NORM_RTOL * ref
    scaled = 0
    for (k, x), (_, y) in zip(a.named_parameters(), b.named_parameters()):
        assert (x.grad is None) == (y.grad is None), k
        if x.grad is not None:
            np.testing.assert_allclose(x.grad.cpu().numpy(), y.grad.cpu().numpy(), rtol=1e-6, atol=0, err_msg=k)
            scaled += 1
    assert scaled > 20
    after = _norm64(_grads(a.parameters()))
    assert abs(after - max_norm * ref / (ref + 1e-6)) <= 1e-6 * max_norm      # three fp32 roundings in the coefficient, 6e-8 each
    # the encoder's gradients are still views of one buffer, and an unclipped FlatAdam step still consumes them in place
    table = a.trans.param_table()
    assert len({p.grad.untyped_storage().data_ptr() for p in table}) == 1
    # below max_norm: every gradient bit-equal
    keep = [(p, p.grad.clone()) for p in a.parameters() if p.grad is not None]
    again = clip_grad_norm_(a.parameters(), 100.0 * ref)
    assert abs(again.item() - after) <= NORM_RTOL * after
    for p, g in keep:
        assert torch.equal(p.grad, g)
    opt = FlatAdam([a], **HYPER)
    home = home_of(a)
    zero_copy = home.zero_copy_elems
    opt.step()
    assert home.zero_copy_elems - zero_copy == sum((p.numel() + 3) & ~3 for p in table)
    # the reference's step on the clipped gradients agrees
    ob = torch.optim.Adam(b.parameters(), **HYPER)
    ob.step()
    for (k, x), (_, y) in zip(a.named_parameters(), b.named_parameters()):
        np.testing.assert_allclose(x.detach().cpu().numpy(), y.detach().cpu().numpy(), err_msg=k, **ADAM_TOL)


def test_clip_grad_norm_error_if_nonfinite(amd):
    from dgvit_amd.optim import clip_grad_norm_
    p = torch.nn.Parameter(torch.ones(8, device="cuda"))
    p.grad = torch.full((8,), float("inf"), device="cuda")
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_([p], 1.0, error_if_nonfinite=True)
    assert torch.isinf(p.grad).all()                       # raised before anything was scaled
    q = torch.nn.Parameter(torch.ones(3, device="cuda"))   # 3 elements: a padded slot
    q.grad = torch.tensor([3.0, 0.0, 4.0], device="cuda")
    n = clip_grad_norm_(q, 1.0, foreach=True)
    assert n.item() == 5.0
    np.testing.assert_allclose(q.grad.cpu().numpy(), np.array([0.6, 0.0, 0.8], dtype=np.float32), rtol=1e-6)


# ------------------------------------------------------------------------------------------------ 9. graph
def test_graphed_step_with_clipping(amd):
    from dgvit_amd.optim import FlatAdam
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2)
    base = amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    base.load_state_dict(O.make_params(O.policy_param_spec(cfg), 61), strict=True)
    base = base.cuda().eval()
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, 8, 61))

    def loss_of(model):
        mean, log_std = model([img, pstate])
        return (mean ** 2).mean() + (log_std ** 2).mean()

    probe = copy.deepcopy(base)
    loss_of(probe).backward()
    max_norm = 0.25 * _norm64(_grads(probe.parameters()))

    def make(model):
        opt = FlatAdam([model], lr=1e-3, capturable=True, max_grad_norm=max_norm)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = loss_of(model)
            loss.backward()
            opt.step()
            return loss.detach()
        return step, opt

    ma, mb = copy.deepcopy(base), copy.deepcopy(base)
    step_a, opt_a = make(ma)
    step_b, opt_b = make(mb)
    g = amd.GraphedStep(step_b, warmup=3)        # 3 warm-up steps inside; the capture pass itself executes nothing
    for _ in range(3):
        step_a()
    norms, coefs = [], []
    for _ in range(4):
        la = step_a()
        lb = g()
        norms.append(opt_b.last_grad_norm.item())
        coefs.append(opt_b._clip.coef.item())
    torch.cuda.synchronize()
    print(f"replayed norms {norms} coefficients {coefs} eager norm {opt_a.last_grad_norm.item()!r}")
    assert abs(la.item() - lb.item()) <= 1e-6 * max(1.0, abs(la.item()))
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=k)
    assert norms[-1] != norms[-2] and coefs[-1] != coefs[-2], "the coefficient was frozen into the graph"


# ------------------------------------------------------------------------------------------------ 10. past 2^31 elements
def test_norm_and_scale_past_2_31_elements(amd):
    """one 8.6 GB buffer: a 32-bit element index would miss the tail"""
    from dgvit_amd import _lib as L
    need_device_memory(12 * 10 ** 9 - (1 << 30))           # skips below 12 GB free
    n = (1 << 31) + (1 << 20)
    x = torch.full((n,), 2.0 ** -12, dtype=torch.float32, device="cuda")
    x[-4:] = 3.0
    exact = math.sqrt((n - 4) * 2.0 ** -24 + 36.0)
    _, out = _measure([x], 1.0)
    got = out[0].item()
    print(f"norm {got!r} exact {exact!r} rel {abs(got - exact) / exact:.3e}")
    assert abs(got - exact) <= NORM_RTOL * exact
    s = torch.tensor([0.5], dtype=torch.float32, device="cuda")
    L.check(L.load().dgvit_scale_by_device_scalar(_p(x), n, _p(s), _stream()), "dgvit_scale_by_device_scalar")
    assert x[:4].tolist() == [2.0 ** -13] * 4
    assert x[-4:].tolist() == [1.5] * 4
    assert x[(1 << 31) + 5].item() == 2.0 ** -13 and x[(1 << 31) - 1].item() == 2.0 ** -13
    del x
    torch.cuda.empty_cache()
