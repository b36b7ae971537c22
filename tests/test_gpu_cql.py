"""GPU: conservative Q-learning.
  * the fused head with shared input pieces through the C ABI, bit for bit against the unshared entry points on materialised inputs, the
    shared pieces' gradient against the ordered fp32 sum of the unshared rows; every output and the scratch inside canary guard zones;
  * q_many of GoTQNetwork and QNetwork against _head on feat.repeat_interleave(M, 0), the encoder counted, the gradient that reaches the
    encoder output caught with a tensor hook; sample_many against _tanh_gaussian on the repeated head outputs;
  * cql_penalty against the fp64 restatement tests/cql_ref.py under the rule of tests/test_gpu_sac_losses.py::test_kernel_parity, its
    exact conditions, and a captured critic step."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cql_ref as R

pytestmark = pytest.mark.gpu

CANARY = 555.0
GUARD = 64            # floats on each side of a buffer (256 bytes: payloads stay 16-byte aligned)
NAN = float("nan")
N1, N2 = 128, 32      # the critics' hidden widths


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


@pytest.fixture(scope="module")
def lib(amd):
    from dgvit_amd import _lib
    return _lib.load()


def _ok(rc, what):
    from dgvit_amd import _lib
    _lib.check(rc, what)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tab(bufs):
    return (ctypes.c_void_p * len(bufs))(*[0 if b is None else b.ptr for b in bufs])


def _p(b):
    return ctypes.c_void_p(0 if b is None else b.ptr)


class Buf:
    """n floats that start `off` floats behind a 16-byte boundary, inside guard zones.  Everything but the payload holds ``fill`` (NaN for
    inputs: reading it poisons the result; the canary for outputs)."""

    def __init__(self, n=None, data=None, off=0, fill=CANARY):
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
            n = data.size
        self.n, self.off, self.fill = n, off, fill
        self.buf = torch.full((GUARD + off + n + GUARD,), fill, dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD + off:GUARD + off + n]
        self.ptr = self.t.data_ptr()
        if data is not None:
            self.t.copy_(torch.from_numpy(data))

    def numpy(self, *shape):
        return self.t.cpu().numpy().reshape(*shape)

    def check(self, what, written=True):
        rest = self.buf.clone()
        if written:
            rest[GUARD + self.off:GUARD + self.off + self.n] = self.fill
        assert bool((rest == self.fill).all()), f"{what}: wrote " + ("outside its extent" if written else "into a slot it must leave alone")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def ordered_sum(rows, B, M):
    """((r[bM] + r[bM+1]) + ...) + r[bM+M-1] in fp32, row by row"""
    rows = np.asarray(rows, np.float32).reshape(B, M, -1)
    acc = rows[:, 0].copy()
    for m in range(1, M):
        acc = (acc + rows[:, m]).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------------ the shared head through the C ABI
# name, B, M, pieces, shared pieces, towers, third layers, W1 offset in floats, NULL dy
HEAD_CASES = [
    ("direct_3x5", 3, 5, (64, 2), (0,), 2, 1, 0, ()),
    ("straddle_7x10", 7, 10, (64, 2), (0,), 2, 1, 0, ()),
    ("long_group_2x33", 2, 33, (64, 2), (0,), 2, 1, 0, ()),
    ("m1_5x1", 5, 1, (64, 2), (0,), 2, 1, 0, ()),
    ("cnn_4x9", 4, 9, (256, 32, 2), (0, 1), 2, 1, 0, ()),
    ("k64_6x6", 6, 6, (62, 2), (0,), 2, 1, 0, ()),
    ("w1_scalar_6x6", 6, 6, (64, 2), (0,), 2, 1, 1, ()),
    ("policy_null_dy_7x10", 7, 10, (64, 2), (0,), 1, 2, 0, (1,)),
]


def _head_data(name, B, M, ks, shared, towers, heads3):
    rs = np.random.RandomState(sum(map(ord, name)))
    K0, rows = sum(ks), B * M
    xs = [rs.randn(B if s in shared else rows, k).astype(np.float32) for s, k in enumerate(ks)]
    params = []
    for _ in range(towers):
        p = [rs.randn(N1, K0) / K0 ** 0.5, rs.randn(N1) * 0.1, rs.randn(N2, N1) / N1 ** 0.5, rs.randn(N2) * 0.1]
        for _ in range(heads3):
            p += [rs.randn(2, N2) / N2 ** 0.5, rs.randn(2) * 0.1]
        params += [q.astype(np.float32) for q in p]
    dys = [rs.randn(rows, 2).astype(np.float32) for _ in range(towers * heads3)]
    return xs, params, dys


def _run_head(lib, case, share_call, bad_share=None):
    """forward + backward of one case through the shared entry points (share_call) or the unshared ones on materialised inputs ->
    outputs by name, after the canary checks"""
    from dgvit_amd import _lib as L
    name, B, M, ks, shared, towers, heads3, w1_off, null_dy = case
    xs, params, dys = _head_data(name, B, M, ks, shared, towers, heads3)
    rows, per = B * M, 4 + 2 * heads3
    if not share_call:
        xs = [np.repeat(x, M, axis=0) if s in shared else x for s, x in enumerate(xs)]
    d = L.dgvit_mlp_desc()
    d.batch, d.nseg, d.n1, d.n2, d.n3, d.towers, d.heads3 = rows, len(ks), N1, N2, 2, towers, heads3
    for s, k in enumerate(ks):
        d.kx[s], d.ldx[s] = k, k
    share = (ctypes.c_int * len(ks))(*(bad_share or [M if s in shared else 1 for s in range(len(ks))]))
    xb = [Buf(data=x, fill=NAN) for x in xs]
    pb = [Buf(data=q, off=w1_off if i % per == 0 else 0, fill=NAN) for i, q in enumerate(params)]
    h1, h2, y = Buf(towers * rows * N1), Buf(towers * rows * N2), Buf(towers * heads3 * rows * 2)
    if share_call:
        rc = lib.dgvit_mlp_head_forward_shared(ctypes.byref(d), share, _tab(xb), _tab(pb), _p(h1), _p(h2), _p(y), _st())
    else:
        rc = lib.dgvit_mlp_head_forward(ctypes.byref(d), _tab(xb), _tab(pb), _p(h1), _p(h2), _p(y), _st())
    torch.cuda.synchronize()
    if bad_share is None:
        _ok(rc, f"forward {name}")
    else:
        assert rc == -1
    for b, what in ((h1, "h1"), (h2, "h2"), (y, "y")):
        b.check(f"{name} {what}", written=bad_share is None)
    out = {"h1": h1.numpy(towers, rows, N1), "h2": h2.numpy(towers, rows, N2), "y": y.numpy(towers, heads3, rows, 2)}
    base = lib.dgvit_mlp_head_backward_scratch_floats(ctypes.byref(d))
    if share_call and bad_share is None:
        nsc = lib.dgvit_mlp_head_backward_shared_scratch_floats(ctypes.byref(d), share)
        assert nsc == base + (sum(rows * ks[s] for s in shared) if M > 1 else 0)
    else:
        nsc = base
    sc = Buf(nsc)
    dyb = [None if i in null_dy else Buf(data=g, fill=NAN) for i, g in enumerate(dys)]
    dins = [Buf(x.shape[0] * x.shape[1]) for x in xs]
    dpar = [Buf(q.size) for q in params]
    if share_call:
        rc = lib.dgvit_mlp_head_backward_shared(ctypes.byref(d), share, _tab(xb), _tab(pb), _p(h1), _p(h2), _tab(dyb), _tab(dins), _tab(dpar),
                                                _p(sc), nsc, _st())
    else:
        rc = lib.dgvit_mlp_head_backward(ctypes.byref(d), _tab(xb), _tab(pb), _p(h1), _p(h2), _tab(dyb), _tab(dins), _tab(dpar), _p(sc), nsc, _st())
    torch.cuda.synchronize()
    if bad_share is None:
        _ok(rc, f"backward {name}")
    else:
        assert rc == -1
    sc.check(f"{name} scratch", written=bad_share is None)
    for s, b in enumerate(dins):
        b.check(f"{name} din.{s}", written=bad_share is None)
        out[f"din.{s}"] = b.numpy(xs[s].shape[0], ks[s])
    for i, b in enumerate(dpar):
        t, q = divmod(i, per)
        unused = q >= 4 and (t * heads3 + (q - 4) // 2) in null_dy          # the third layer of a NULL dy gets no gradient
        b.check(f"{name} dpar.{i}", written=bad_share is None and not unused)
        if not unused:
            out[f"dpar.{i}"] = b.numpy(*params[i].shape)
    return out


@pytest.mark.parametrize("case", HEAD_CASES, ids=[c[0] for c in HEAD_CASES])
def test_shared_head_equals_the_unshared_head_on_materialised_inputs(lib, case):
    name, B, M, ks, shared = case[:5]
    got, want = _run_head(lib, case, True), _run_head(lib, case, False)
    assert set(got) == set(want)
    assert not np.isnan(got["y"]).any()
    for k in got:
        s = int(k.split(".")[1]) if k.startswith("din.") else None
        if s in shared:
            assert got[k].shape == (B, ks[s]), k
            assert same_bits(got[k], ordered_sum(want[k], B, M)), f"{name} {k}: not the ordered fp32 sum of the unshared rows"
        else:
            assert same_bits(got[k], want[k]), f"{name} {k}: differs from the unshared call, max |diff| {np.abs(got[k] - want[k]).max():.3e}"
    again = _run_head(lib, case, True)
    for k in got:
        assert same_bits(got[k], again[k]), f"{name} {k}: two runs differ"


def test_shared_head_refusals_leave_every_buffer_alone(lib):
    for bad in ([4, 1], [5, 2], [0, 1], [257, 1]):
        _run_head(lib, HEAD_CASES[0], True, bad_share=bad)           # 15 rows: not a multiple of 4; 2 is not the common count; ...


# ------------------------------------------------------------------------------------------------ q_many
def _critic(amd, kind, K=1):
    torch.manual_seed(7)
    kw = {"frame_channels": K} if K != 1 else {}
    if kind == "got":           # the smallest encoder the GPU tests build, one block
        net = amd.GoTQNetwork(2, 2, 1, 2, 64, image_size=(12, 20), patch_size=(3, 5), **kw)
        shape = (12, 20, K) if K != 1 else (12, 20)
    else:
        net = amd.QNetwork(2, 2, **kw)
        shape = (40, 48, K) if K != 1 else (40, 48)
    return net.cuda().eval(), shape


def _towers(net):
    return [(net.fc1, net.fc2, [net.fc3]), (net.fc11, net.fc21, [net.fc31])]


def _q_many_case(amd, kind, B, M, K=1, frozen=False):
    from dgvit_amd.sac_networks import _head
    net, shape = _critic(amd, kind, K)
    if frozen:
        for p in net.parameters():
            p.requires_grad_(False)
    g = torch.Generator().manual_seed(B * 100 + M)
    frames, pstate = torch.rand(B, *shape, generator=g).cuda(), torch.randn(B, 2, generator=g).cuda()
    actions = torch.randn(B, M, 2, generator=g).cuda().requires_grad_(True)
    w1, w2 = torch.randn(B, M, 2, generator=g).cuda(), torch.randn(B, M, 2, generator=g).cuda()
    calls, feats, gfeat = [], [], []

    def seen(out, rows):
        calls.append(rows)
        feats.append(out)
        if out.requires_grad:
            out.register_hook(lambda gr: gfeat.append(gr.clone()))

    if kind == "got":
        handle = net.trans.register_forward_hook(lambda mod, inp, out: seen(out, inp[0].shape[0]))
    else:
        inner = net._features

        def counting(istate):
            out = inner(istate)
            seen(out, istate.shape[0])
            return out
        net._features = counting
    q1, q2 = net.q_many([frames, pstate], actions)
    assert q1.shape == q2.shape == (B, M, 2)
    assert calls == [B], f"the encoder ran {len(calls)} time(s) on {calls} rows, not once on {B}"
    ((q1 * w1).sum() + (q2 * w2).sum()).backward()
    torch.cuda.synchronize()
    got_a = actions.grad.clone()
    head = [p for tw in _towers(net) for p in (tw[0].weight, tw[0].bias, tw[1].weight, tw[1].bias, tw[2][0].weight, tw[2][0].bias)]
    got_p = [None if p.grad is None else p.grad.clone() for p in head]
    if kind == "got":
        handle.remove()
    else:
        del net._features
    # the materialised route on the features of that one encoder call
    for p in net.parameters():
        p.grad = None
    rows = []
    feat = feats[0].detach().view(B, -1).requires_grad_(not frozen)
    fm = feat.repeat_interleave(M, 0)
    if not frozen:
        fm.register_hook(lambda gr: rows.append(gr.clone()))
    pieces = [fm]
    if kind == "cnn":
        from dgvit_amd.sac_networks import _lin
        pieces.append(_lin(net.fc_embed, pstate, relu=True).detach().repeat_interleave(M, 0))
    a2 = actions.detach().clone().requires_grad_(True)
    (r1,), (r2,) = _head(pieces + [a2.view(B * M, 2)], _towers(net))
    assert torch.equal(q1.detach().view(B * M, 2), r1.detach()) and torch.equal(q2.detach().view(B * M, 2), r2.detach()), "q differs from the materialised head"
    ((r1 * w1.view(B * M, 2)).sum() + (r2 * w2.view(B * M, 2)).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(got_a, a2.grad.view(B, M, 2)), "actions.grad differs from the materialised route's"
    assert bool(got_a.abs().max() > 0)
    if frozen:
        assert all(gp is None for gp in got_p) and not gfeat
        return
    for gp, p in zip(got_p, head):
        assert gp is not None and torch.equal(gp, p.grad), "a head parameter gradient differs from the materialised route's"
    assert len(gfeat) == 1 and len(rows) == 1
    want = ordered_sum(rows[0].cpu().numpy(), B, M)
    assert same_bits(gfeat[0].view(B, -1).cpu().numpy(), want), "the gradient at the encoder output is not the ordered sum of the rows"


@pytest.mark.parametrize("kind", ["got", "cnn"])
@pytest.mark.parametrize("B, M", [(3, 5), (7, 10)])
def test_q_many_runs_the_encoder_once_and_equals_the_materialised_head(amd, kind, B, M):
    _q_many_case(amd, kind, B, M)


@pytest.mark.parametrize("kind", ["got", "cnn"])
def test_q_many_of_a_frozen_critic_still_differentiates_the_actions(amd, kind):
    _q_many_case(amd, kind, 7, 10, frozen=True)


@pytest.mark.parametrize("kind", ["got", "cnn"])
def test_q_many_on_frame_stacks(amd, kind):
    _q_many_case(amd, kind, 3, 5, K=2)


def test_q_many_equals_forward_on_repeated_frames_row_for_row(amd):
    """M = 1 is forward() itself; and best-of-N: the argmax over dim 1 picks among the M values of a state"""
    net, shape = _critic(amd, "cnn")
    g = torch.Generator().manual_seed(1)
    frames, pstate, a = torch.rand(4, *shape, generator=g).cuda(), torch.randn(4, 2, generator=g).cuda(), torch.randn(4, 1, 2, generator=g).cuda()
    with torch.no_grad():
        q1, q2 = net.q_many([frames, pstate], a)
        f1, f2 = net([frames, pstate, a[:, 0]])
    assert torch.equal(q1[:, 0], f1) and torch.equal(q2[:, 0], f2)


# ------------------------------------------------------------------------------------------------ sample_many
@pytest.mark.parametrize("kind", ["got", "cnn"])
def test_sample_many_is_sample_on_the_repeated_head_outputs(amd, kind, monkeypatch):
    from dgvit_amd import sac_networks as N
    torch.manual_seed(3)
    B, n = 5, 7
    if kind == "got":
        pol = amd.GoTPolicy(2, 2, 1, 2, 64, image_size=(12, 20), patch_size=(3, 5)).to("cuda").eval()
        frames = torch.rand(B, 12, 20).cuda()
        enc, count = pol.trans, []
        enc.register_forward_hook(lambda mod, inp, out: count.append(inp[0].shape[0]))
    else:
        pol = amd.GaussianPolicy(2, 2).to("cuda").eval()
        frames = torch.rand(B, 40, 48).cuda()
        inner, count = pol._features, []
        pol._features = lambda istate: (count.append(istate.shape[0]), inner(istate))[1]
    pstate = torch.randn(B, 2).cuda()
    eps = torch.randn(B * n, 2).cuda()
    monkeypatch.setattr(N, "_standard_normal", lambda like: eps[:like.shape[0]].clone())
    action, log_prob, tanh_mean = pol.sample_many([frames, pstate], n)
    assert count == [B], "one encoder pass on B frames"
    assert action.shape == (B, n, 2) and log_prob.shape == (B, n) and tanh_mean.shape == (B, 2)
    mean, lsr = pol._head_outputs([frames, pstate])
    a, lp, tm = N._tanh_gaussian(pol, mean.repeat_interleave(n, 0), lsr.repeat_interleave(n, 0))
    assert torch.equal(action.view(B * n, 2), a) and torch.equal(log_prob.reshape(B * n, 1), lp) and torch.equal(tanh_mean, tm[::n])
    s_a, s_lp, s_tm = pol.sample([frames, pstate])
    assert torch.equal(s_tm, tanh_mean), "tanh_mean is sample()'s"
    (action.sum() + log_prob.sum()).backward()
    assert pol.fc1.weight.grad is not None and bool(torch.isfinite(pol.fc1.weight.grad).all())


# ------------------------------------------------------------------------------------------------ cql_penalty: parity
def _rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


def _device(amd, x, T, mask, kw):
    q = {k: v.cuda().requires_grad_(True) for k, v in x.items() if k != "log_w"}
    lw = None if x["log_w"] is None else x["log_w"].cuda()
    kw = dict(kw)
    la = None
    if "log_weight" in kw:
        la = kw["log_weight"] = kw["log_weight"].cuda().requires_grad_(True)
    out = amd.sac_losses.cql_penalty(q["q1_cat"], q["q2_cat"], q["q1_data"], q["q2_data"], log_w=lw, temperature=T,
                                     mask=None if mask is None else mask.cuda(), **kw)
    assert out.loss.shape == () and out.gap.shape == (2,) and out.used.shape == () and not out.gap.requires_grad and not out.used.requires_grad
    out.loss.backward()
    assert la is None or la.grad is None, "nothing flows from the penalty into log_weight"
    got = dict(loss=out.loss, gap=out.gap, used=out.used, dq1_cat=q["q1_cat"].grad, dq2_cat=q["q2_cat"].grad, dq1_data=q["q1_data"].grad,
               dq2_data=q["q2_data"].grad)
    if "target_gap" in kw:
        for t in q.values():
            t.grad = None
        out.weight_loss.backward()
        assert all(t.grad is None for t in q.values()), "nothing flows from the weight loss into the critics"
        got.update(weight_loss=out.weight_loss, dlog_weight=la.grad)
    else:
        assert out.weight_loss is None
    return {k: v.detach().double().cpu() for k, v in got.items()}


@pytest.mark.parametrize("lagrange", [False, True], ids=["float_weight", "log_weight"])
def test_cql_penalty_parity(amd, lagrange):
    """the rule of tests/test_gpu_sac_losses.py::test_kernel_parity: per output, max |hip - ref64| / max |ref64| against the same quantity
    of the restatement's own fp32 evaluation on the CPU (margin 2; 4 where exp(log_weight) is taken on the device; 2^-23 where the
    fp32 evaluation is exact, as for `used`, a sum of ones).  The table it prints is recorded in DESIGN 3.47."""
    margin = 4.0 if lagrange else 2.0
    names = R.OUTPUTS + (R.LAGRANGE_OUTPUTS if lagrange else ())
    kw = dict(log_weight=torch.tensor([0.3]), target_gap=0.25) if lagrange else dict(weight=0.7)
    hip, yard, exact = {k: 0.0 for k in names}, {k: 0.0 for k in names}, []
    for shape, T, scale in R.CASES:
        for with_log_w in (False, True):
            x = R.inputs(shape, scale, 11, with_log_w)
            x64 = {k: None if v is None else v.double() for k, v in x.items()}
            for mask in (None, R.mixed_mask(shape[0]), torch.zeros(shape[0], dtype=torch.bool)):
                dev = _device(amd, x, T, mask, kw)
                assert set(dev) == set(names)
                for k in names:
                    assert bool(torch.isfinite(dev[k]).all()), (k, shape, T)
                if mask is not None and not bool(mask.any()):
                    for k in names:
                        assert bool((dev[k] == 0).all()), f"{k}: not an exact zero when no row is used"
                    continue
                r64, r32 = R.penalty(**x64, temperature=T, mask=mask, **kw), R.penalty(**x, temperature=T, mask=mask, **kw)
                for k in names:
                    assert dev[k].shape == r64[k].shape, (k, dev[k].shape, r64[k].shape)
                    assert bool(torch.isfinite(r32[k]).all()) and float(r32[k].abs().max()) > 0, (k, shape, T)
                    h, y = _rel(dev[k], r64[k]), _rel(r32[k].double(), r64[k])
                    hip[k], yard[k] = max(hip[k], h), max(yard[k], y)
                    if y == 0.0:
                        exact.append((k, shape, h))
    print(f"\ncql_penalty, {'log_weight' if lagrange else 'float weight'} (margin {margin}): output  hip  yardstick  hip/yardstick")
    for k in names:
        print(f"  {k:12s} {hip[k]:.3e}  {yard[k]:.3e}  {hip[k] / yard[k] if yard[k] > 0 else math.inf:.2f}")
    print("  outputs whose fp32 evaluation is exact:", sorted(set((k, s) for k, s, _ in exact)), max((h for *_, h in exact), default=0.0))
    for k, shape, h in exact:
        assert h <= 2.0 ** -23, (k, shape, h)
    for k in names:
        if yard[k] == 0.0:                    # exact in fp32 in every case
            assert hip[k] <= 2.0 ** -23, (k, hip[k])
        else:
            assert hip[k] <= margin * yard[k], (k, hip[k], yard[k])


# ------------------------------------------------------------------------------------------------ cql_penalty: exact conditions
def _pen(amd, shape=(7, 30, 2), T=1.0, scale=1.0, grad=True, **kw):
    x = {k: None if v is None else v.cuda() for k, v in R.inputs(shape, scale, 5, True).items()}
    q = [x[k].requires_grad_(grad) for k in ("q1_cat", "q2_cat", "q1_data", "q2_data")]
    return x, q, amd.sac_losses.cql_penalty(*q, log_w=x["log_w"], temperature=T, **kw)


def test_cql_an_all_false_mask_gives_exact_zeros(amd):
    for mask in (torch.zeros(7, dtype=torch.bool), torch.zeros(7, 1)):
        la = torch.tensor([0.3], device="cuda", requires_grad=True)
        x, q, out = _pen(amd, T=0.1, scale=50.0, mask=mask.cuda(), log_weight=la, target_gap=0.25)
        (out.loss + out.weight_loss).backward()
        for t in (out.loss, out.weight_loss, out.gap, out.used, la.grad, *[t.grad for t in q]):
            assert bool((t == 0).all()) and not bool(torch.isnan(t).any())


def test_cql_one_proposal_is_the_identity(amd):
    """M = 1: lse = z, within 1 fp32 ulp (T (z / T) in double, rounded once in the gap)"""
    for T in (1.0, 0.1, 3.0):
        x, q, out = _pen(amd, shape=(1, 1, 1), T=T, scale=3.0, weight=1.0)
        d = {k: float(v.detach().double()) for k, v in x.items()}
        z1, z2 = d["q1_cat"] - d["log_w"] - d["q1_data"], d["q2_cat"] - d["log_w"] - d["q2_data"]
        for got, want in zip(out.gap.tolist(), (z1, z2)):
            assert abs(got - want) <= 2.0 ** -23 * abs(want), (T, got, want)


def test_cql_gradients(amd):
    B, M, C = 33, 5, 3
    mask = R.mixed_mask(B).cuda()
    x, q, out = _pen(amd, shape=(B, M, C), T=2.0, scale=10.0, weight=0.7, mask=mask)
    assert float(out.used) == float(mask.sum())
    out.loss.backward()
    g1 = [t.grad.clone() for t in q]
    for g in g1:
        assert bool((g[~mask] == 0).all()), "rows outside the mask get exactly zero gradient"
        assert bool((g[mask] != 0).all())
    want = float(np.float32(0.7)) / (float(mask.sum()) * C)          # the weight crosses the ABI as a float
    for gc, gd in ((g1[0], g1[2]), (g1[1], g1[3])):
        s = gc[mask].double().sum(1)
        assert float((s - want).abs().max()) <= M * 2.0 ** -24 * want, "the softmax sums to w / (used C) within fp32 rounding of M terms"
        assert float((gd[mask].double() + want).abs().max()) <= 2.0 ** -24 * want
    # a non-unit upstream gradient scales the gradients
    for t in q:
        t.grad = None
    _, q2, out2 = _pen(amd, shape=(B, M, C), T=2.0, scale=10.0, weight=0.7, mask=mask)
    (out2.loss * 3.0).backward()
    for a, b in zip(g1, (t.grad for t in q2)):
        assert torch.equal(3.0 * a, b)
    # inputs that ask for no gradient get None
    x, q3, _ = _pen(amd, shape=(B, M, C), grad=False, weight=0.7)
    q3[1].requires_grad_(True)
    out3 = amd.sac_losses.cql_penalty(*q3, log_w=x["log_w"].requires_grad_(True), weight=0.7)
    out3.loss.backward()
    assert q3[0].grad is None and q3[2].grad is None and q3[3].grad is None and x["log_w"].grad is None and q3[1].grad is not None
    with torch.no_grad():
        _, _, out4 = _pen(amd, shape=(B, M, C), weight=0.7)
    assert not out4.loss.requires_grad
    # two calls give the same bits
    _, q5, out5 = _pen(amd, shape=(B, M, C), T=2.0, scale=10.0, weight=0.7, mask=mask)
    out5.loss.backward()
    assert torch.equal(out5.loss, out.loss) and all(torch.equal(a, t.grad) for a, t in zip(g1, q5))


def test_cql_weight_loss_reaches_only_log_weight(amd):
    from dgvit_amd.optim import FlatAdam
    la = torch.tensor([0.3], device="cuda", requires_grad=True)
    opt = FlatAdam([la], lr=1e-2)
    x, q, out = _pen(amd, log_weight=la, target_gap=0.25)
    opt.zero_grad()
    out.weight_loss.backward()
    assert all(t.grad is None for t in q) and la.grad is not None and la.grad.shape == (1,)
    excess = float(out.gap.double().sum()) - 0.5
    assert float(la.grad) == pytest.approx(-math.exp(float(np.float32(0.3))) * excess, rel=1e-6)
    assert float(out.weight_loss) == float(la.grad) and float(out.loss) == pytest.approx(-float(out.weight_loss), rel=1e-7)
    g = float(la.grad)
    opt.step()
    assert g != 0 and float(la.detach()) == pytest.approx(float(np.float32(0.3)) - 1e-2 * math.copysign(1.0, g), rel=1e-6)


# ------------------------------------------------------------------------------------------------ capture
def test_a_captured_cql_critic_step_equals_the_eager_steps(amd):
    from dgvit_amd.optim import FlatAdam
    S = amd.sac_losses
    B, M = 8, 6
    g = torch.Generator().manual_seed(2)
    frames, pstate = torch.rand(B, 40, 48, generator=g).cuda(), torch.randn(B, 2, generator=g).cuda()
    act, actions = torch.randn(B, 2, generator=g).cuda(), torch.randn(B, M, 2, generator=g).cuda()
    log_w = torch.randn(B, M, generator=g).cuda()
    rew, nlp = torch.randn(B, 1, generator=g).cuda(), torch.randn(B, 1, generator=g).cuda()
    q1n, q2n = torch.randn(B, 2, generator=g).cuda(), torch.randn(B, 2, generator=g).cuda()
    values = (0.3, 1.2, -0.7)

    def make():
        net, _ = _critic(amd, "cnn")
        la = torch.tensor([values[0]], device="cuda")
        opt = FlatAdam([net], lr=1e-3, capturable=True)

        def step():
            q1, q2 = net([frames, pstate, act])
            c1, c2 = net.q_many([frames, pstate], actions)
            c = S.critic_loss(q1, q2, rew, q1n, q2n, nlp, alpha=0.2)
            p = S.cql_penalty(c1, c2, q1, q2, log_w=log_w, log_weight=la, target_gap=0.1)
            opt.zero_grad(set_to_none=True)
            (c.loss + p.loss).backward()
            opt.step()
            return c.loss, p.loss, p.gap, p.weight_loss
        return net, la, step

    net_e, la_e, step_e = make()
    net_g, la_g, step_g = make()
    graph = amd.GraphedStep(step_g, warmup=1)
    step_e()                                    # the warm-up step of the graphed twin
    seen = []
    for v in values:
        la_e.fill_(v)
        la_g.fill_(v)
        want = [t.clone() for t in step_e()]
        got = [t.clone() for t in graph()]
        for a, b in zip(got, want):
            assert torch.equal(a, b), "a replay gives the bits of the eager step"
        seen.append(got)
    for a, b in zip(net_g.parameters(), net_e.parameters()):
        assert torch.equal(a, b), "after three replays the parameters are those of the eager steps"
    assert not torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[1][3], seen[2][3]), "the penalty follows log_weight"
