"""GPU: parameter groups and device-side learning-rate schedules in one launch -- dgvit_adam_step_groups at the C level
(bit-equal to the existing Adam kernels where they overlap, to itself segment by segment, and within ADAM_TOL of an fp64 per-element
reference), FlatAdamW / FlatAdam with groups and an LRSchedule against torch.optim.AdamW + LambdaLR, under GraphedStep, set_lr,
state_dict, and a run past 2 GiB.

ADAM_TOL is the project's bound for an fp32 Adam step against a reference (test_flat_adam_matches_torch_adam): an emulation of the
kernel's fp32 formulas against fp64 over 8 scheduled steps on N(0, 1) data stays below 0.06 of it."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import GIB, O, need_device_memory  # noqa: E402

ADAM_TOL = dict(rtol=2e-5, atol=2e-6)
HYPER = dict(lr=3e-3, eps=1e-3)            # test_gpu_grad_clip.py's, with the decay set per test
BETA1, BETA2, EPS = 0.9, 0.999, 1e-3
GRID_PASS4 = 2048 * 256                    # float4s one pass of the (capped) grid covers


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available()
    return dgvit_amd


def _p(t, offset_bytes=0):
    return ctypes.c_void_p(t.data_ptr() + offset_bytes)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _randn(n, seed):
    return torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


def _groups_call(bufs, g, n, end4, group, nseg, hyper, ngroups, decoupled, step, sched=(0, 0, 0, 0.0), step_dev=None, scale=None,
                 lr_out=None, first4=0, seg0=0, sched_step=None):
    """dgvit_adam_step_groups on the float4s [first4, first4 + n / 4) of the buffers, with the tables read from entry seg0 on"""
    from dgvit_amd import _lib as L
    off = 16 * first4
    rc = L.load().dgvit_adam_step_groups(
        _p(bufs[0], off), _p(g, off), _p(bufs[1], off), _p(bufs[2], off), n, _p(end4, 8 * seg0), _p(group, seg0), nseg, _p(hyper), ngroups,
        _p(lr_out) if lr_out is not None else None, BETA1, BETA2, EPS, decoupled, step, step if sched_step is None else sched_step,
        _p(step_dev) if step_dev is not None else None, *sched, _p(scale) if scale is not None else None, _stream())
    L.check(rc, "dgvit_adam_step_groups")


# ------------------------------------------------------------------------------------------------ 1. anchor: the existing kernels
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
def test_one_group_is_the_existing_kernel_bit_for_bit(amd, scaled):
    """one group, L2 decay, constant schedule == dgvit_adam_step[_scaled] with a device step counter; the grid-stride loop iterates (more
    than one pass of the capped grid) and ends in a ragged tail; a host step gives the same bits as a device step"""
    from dgvit_amd import _lib as L
    lib = L.load()
    n4 = GRID_PASS4 + 257
    n = 4 * n4
    lr, wd = 3e-3, 0.01
    init = [_randn(n, 1), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    new, host, old = ([t.clone() for t in init] for _ in range(3))
    end4 = torch.tensor([n4], dtype=torch.int64, device="cuda")
    group = torch.zeros(1, dtype=torch.uint8, device="cuda")
    hyper = torch.tensor([[lr, wd]], dtype=torch.float32, device="cuda")
    s = torch.tensor([0.37], dtype=torch.float32, device="cuda") if scaled else None
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    lr_out = torch.full((1,), float("nan"), device="cuda")
    for t in (1, 2, 3):
        g = _randn(n, 10 + t)
        step_dev.fill_(t)
        _groups_call(new, g, n, end4, group, 1, hyper, 1, 0, 0, step_dev=step_dev, scale=s, lr_out=lr_out)     # (step = 0: not read)
        _groups_call(host, g, n, end4, group, 1, hyper, 1, 0, t, scale=s)
        args = (_p(old[0]), _p(g), _p(old[1]), _p(old[2]), n, lr, BETA1, BETA2, EPS, wd, t, _p(step_dev))
        if scaled:
            L.check(lib.dgvit_adam_step_scaled(*args, _p(s), _stream()), "dgvit_adam_step_scaled")
        else:
            L.check(lib.dgvit_adam_step(*args, _stream()), "dgvit_adam_step")
        for x, y, z, name in zip(new, old, host, "pmv"):
            assert torch.equal(x, y), f"{name} differs from the existing kernel at step {t}"
            assert torch.equal(x, z), f"{name}: host step and device step differ at step {t}"
        assert torch.equal(lr_out, hyper[:, 0])
    assert not torch.equal(new[0], init[0])


# ------------------------------------------------------------------------------------------------ 2. the segment lookup
def _boundaries(nseg, n4, seed):
    """ascending segment ends (the last is n4): random, but with one-float4 segments, two of them side by side, ends at 255, 256 and
    257, and a last segment of one float4 -- as many of these as nseg has room for"""
    forced = [n4 - 1, 256, 1, 2, 255, 257][:nseg - 1]
    rng = np.random.RandomState(seed)
    ends = set(forced)
    while len(ends) < nseg - 1:
        ends.add(int(rng.randint(1, n4)))
    return sorted(ends) + [n4]


SCHED = (1, 2, 6, 0.1)      # cosine, warm-up 2, 6 steps in all, down to a tenth


def _factor(s):
    from dgvit_amd.optim import LRSchedule
    return LRSchedule("cosine", warmup_steps=2, total_steps=6, final_ratio=0.1).factor(s)


@pytest.fixture(scope="module")
def lookup_data():
    n4 = 3 * GRID_PASS4 + 257          # every lane walks three or four grid passes: its cursor has to move
    n = 4 * n4
    init = [_randn(n, 2), _randn(n, 3) * 0.1, _randn(n, 4).abs() * 0.01]
    grads = {t: _randn(n, 20 + t) for t in (3, 4)}
    return n4, init, grads


@pytest.mark.parametrize("decoupled", [0, 1], ids=["l2", "decoupled"])
@pytest.mark.parametrize("nseg", [1, 2, 257, 2048])
def test_segment_lookup(amd, lookup_data, nseg, decoupled):
    """three groups over nseg segments: bit-equal to the same entry point run once per segment, and within ADAM_TOL of fp64 with
    per-element lr and weight decay, every element counted.  Steps 3 and 4 of the cosine schedule (factor 1 and 0.868)."""
    n4, init, grads = lookup_data
    n = 4 * n4
    hyper_host = [(3e-3, 0.05), (1e-3, 0.0), (2e-2, 0.3)]
    hyper = torch.tensor(hyper_host, dtype=torch.float32, device="cuda")
    ends = _boundaries(nseg, n4, 1000 + nseg)
    assert len(ends) == nseg and all(a < b for a, b in zip(ends, ends[1:])) and ends[-1] == n4
    rng = np.random.RandomState(nseg)
    groups = [int(x) for x in rng.randint(0, 3, size=nseg)]
    starts = [0] + ends[:-1]
    if nseg >= 257:
        assert {255, 256, 257, n4 - 1, 1, 2} <= set(ends)
    end4 = torch.tensor(ends, dtype=torch.int64).cuda()
    group = torch.tensor(groups, dtype=torch.uint8).cuda()
    lens = torch.tensor([e - s for s, e in zip(starts, ends)], dtype=torch.int64).cuda()
    one, seg = [t.clone() for t in init], [t.clone() for t in init]
    ref = [t.double() for t in init]
    seg_of = torch.repeat_interleave(group.long(), lens * 4)                    # the group of every element
    assert seg_of.numel() == n
    lr_e, wd_e = hyper.double()[seg_of, 0], hyper.double()[seg_of, 1]
    b1, b2, eps = float(np.float32(BETA1)), float(np.float32(BETA2)), float(np.float32(EPS))
    lr_out = torch.full((3,), float("nan"), device="cuda")
    for t in (3, 4):
        g = grads[t]
        _groups_call(one, g, n, end4, group, nseg, hyper, 3, decoupled, t, sched=SCHED, lr_out=lr_out)
        for k in range(nseg):
            _groups_call(seg, g, 4 * (ends[k] - starts[k]), lens, group, 1, hyper, 3, decoupled, t, sched=SCHED, first4=starts[k], seg0=k)
        for x, y, name in zip(one, seg, "pmv"):
            assert torch.equal(x, y), f"{name} differs from the per-segment runs at step {t}"
        f = _factor(t - 1)
        want_lr = torch.tensor([lr * f for lr, _ in hyper_host], dtype=torch.float64)
        np.testing.assert_allclose(lr_out.cpu().double().numpy(), want_lr.numpy(), rtol=1e-6)
        g64 = g.double()
        lr_t = lr_e * f
        if decoupled:
            ref[0] = ref[0] * (1.0 - lr_t * wd_e)
            gg = g64
        else:
            gg = g64 + wd_e * ref[0]
        ref[1] = b1 * ref[1] + (1.0 - b1) * gg
        ref[2] = b2 * ref[2] + (1.0 - b2) * gg * gg
        ref[0] = ref[0] - (lr_t / (1.0 - b1 ** t)) * ref[1] / (ref[2].sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    for x, r, name in zip(one, ref, "pmv"):
        err = (x.double() - r).abs()
        bound = ADAM_TOL["atol"] + ADAM_TOL["rtol"] * r.abs()
        worst = float((err / bound).max())
        print(f"nseg={nseg} decoupled={decoupled} {name}: worst error / bound {worst:.4f} over {err.numel()} elements")
        assert worst <= 1.0, name
    assert not torch.equal(one[0], init[0])


def test_one_float4_boundaries_with_two_segments(amd):
    """nseg = 2 has one boundary: behind the first float4, at 256, and before the last float4, each against the per-segment runs"""
    n4 = GRID_PASS4 + 257
    n = 4 * n4
    hyper = torch.tensor([(3e-3, 0.05), (2e-2, 0.3)], dtype=torch.float32, device="cuda")
    group = torch.tensor([1, 0], dtype=torch.uint8).cuda()
    g = _randn(n, 31)
    init = [_randn(n, 30), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    for cut in (1, 256, n4 - 1):
        end4 = torch.tensor([cut, n4], dtype=torch.int64).cuda()
        lens = torch.tensor([cut, n4 - cut], dtype=torch.int64).cuda()
        one, seg = [t.clone() for t in init], [t.clone() for t in init]
        _groups_call(one, g, n, end4, group, 2, hyper, 2, 1, 1)
        _groups_call(seg, g, 4 * cut, lens, group, 1, hyper, 2, 1, 1, first4=0, seg0=0)
        _groups_call(seg, g, 4 * (n4 - cut), lens, group, 1, hyper, 2, 1, 1, first4=cut, seg0=1)
        for x, y, name in zip(one, seg, "pmv"):
            assert torch.equal(x, y), f"{name} differs with the boundary at {cut}"
        # and the two sides did take different hyper-parameters: with the groups swapped the parameters differ on both sides
        swapped = [t.clone() for t in init]
        _groups_call(swapped, g, n, end4, torch.tensor([0, 1], dtype=torch.uint8).cuda(), 2, hyper, 2, 1, 1)
        assert not torch.equal(swapped[0][:4 * cut], one[0][:4 * cut]) and not torch.equal(swapped[0][4 * cut:], one[0][4 * cut:])


# ------------------------------------------------------------------------------------------------ 3. FlatAdamW against torch.optim.AdamW
def _policy(amd, seed=51, batch=16):
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=64, depth=2, heads=2)
    m = amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    m.load_state_dict(O.make_params(O.policy_param_spec(cfg), seed), strict=True)
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(cfg, batch, seed))
    return m.cuda().eval(), img, pstate


def _loss(m, img, pstate, it):
    mean, log_std = m([img, pstate])
    return (mean ** 2).mean() + (log_std ** 2).mean() * (it + 1)


HEAD_LR = 1e-3


def _our_groups(m, weight_decay=0.05):
    from dgvit_amd.optim import no_decay_groups
    heads = [p for k, p in m.named_parameters() if not k.startswith("trans.")]
    return no_decay_groups(m.trans, weight_decay) + [{"params": heads, "lr": HEAD_LR, "weight_decay": 0.01}]


def _torch_groups(m, weight_decay=0.05):
    """the same three groups, by name, for torch.optim.AdamW"""
    decay, rest, heads = [], [], []
    for k, p in m.named_parameters():
        if not k.startswith("trans."):
            heads.append(p)
        elif p.ndim >= 2 and not k.endswith(("pos_embedding", "cls_token")):
            decay.append(p)
        else:
            rest.append(p)
    return [{"params": decay, "weight_decay": weight_decay}, {"params": rest, "weight_decay": 0.0},
            {"params": heads, "lr": HEAD_LR, "weight_decay": 0.01}]


def _count_runs_and_segments(opt):
    """what step() should launch, from the homes alone: maximal stretches of adjacent slots with a gradient inside one section of one
    home (all step counts are equal here); and how often the group changes inside them"""
    from dgvit_amd import optim
    by_home = {}
    for p in opt.params:
        if p.grad is not None:
            home, i = optim._HOME_OF[p]
            by_home.setdefault(id(home), (home, []))[1].append((i, opt._group_of[id(p)]))
    runs = segments = 0
    for home, slots in by_home.values():
        slots.sort()
        runs += 1
        segments += 1
        for (a, ga), (b, gb) in zip(slots, slots[1:]):
            if b != a + 1 or home.sections[a] != home.sections[b]:
                runs += 1
                segments += 1
            elif ga != gb:
                segments += 1
    return runs, segments


def test_flat_adamw_with_groups_matches_torch_adamw(amd):
    from dgvit_amd.optim import FlatAdam, FlatAdamW, home_of
    base, img, pstate = _policy(amd)
    a, b, c = (copy.deepcopy(base) for _ in range(3))
    home_of(a)
    home_of(c)                                                   # one home per policy, the layout FlatAdam([policy]) uses
    oa = FlatAdamW(_our_groups(a), **HYPER)
    ob = torch.optim.AdamW(_torch_groups(b), **HYPER)
    oc = FlatAdam(_our_groups(c), **HYPER)                       # the same numbers as L2 decay: must end up somewhere else
    assert oa.last_lr is None and len(oa.param_groups) == 3
    assert [g["lr"] for g in oa.param_groups] == [3e-3, 3e-3, HEAD_LR] and [g["weight_decay"] for g in oa.param_groups] == [0.05, 0.0, 0.01]
    for it in range(3):
        for m, o in ((a, oa), (b, ob), (c, oc)):
            o.zero_grad(set_to_none=True)
            _loss(m, img, pstate, it).backward()
        if it == 1:                                              # one parameter without a gradient: its run is split in two
            for m in (a, b, c):
                assert m.fc1.bias.grad is not None
                m.fc1.bias.grad = None
        runs, segments = _count_runs_and_segments(oa)
        for o in (oa, ob, oc):
            o.step()
        if it == 0:
            print(f"step 0: {oa.last_step_launches} launches for {runs} runs holding {segments} segments of {len(oa.param_groups)} groups")
            assert oa.last_step_launches == runs == oc.last_step_launches
            assert segments >= runs + 8, "decay and no-decay parameters should alternate along the encoder's run"
        if it == 1:
            print(f"step 1 (fc1.bias skipped): {oa.last_step_launches} launches, {runs} runs")
            assert oa.last_step_launches == runs
        np.testing.assert_allclose(oa.last_lr.cpu().numpy(), np.array([3e-3, 3e-3, HEAD_LR], dtype=np.float32), rtol=1e-6)
    enc = sum((p.numel() + 3) & ~3 for p in a.trans.param_table())
    # (a run of a single parameter, as the split leaves behind, is a view of its own gradient as well: hence not ==)
    assert 3 * enc <= home_of(a).zero_copy_elems < 3 * enc + 1024, "encoder gradients should have been consumed in place, once per step"
    far = total = 0
    for (k, pa), (_, pb), (_, pc) in zip(a.named_parameters(), b.named_parameters(), c.named_parameters()):
        xa, xb, xc = (t.detach().cpu().numpy() for t in (pa, pb, pc))
        np.testing.assert_allclose(xa, xb, err_msg=k, **ADAM_TOL)
        far += int((np.abs(xc - xb) > 100 * (ADAM_TOL["atol"] + ADAM_TOL["rtol"] * np.abs(xb))).sum())
        total += xb.size
    print(f"L2 FlatAdam with the same numbers differs from torch.optim.AdamW beyond 100 x tolerance in {far} of {total} entries")
    assert far > 0, "decoupled and L2 decay agree: the comparison above shows nothing"


# ------------------------------------------------------------------------------------------------ 4. schedule
@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_schedule_matches_lambda_lr(amd, kind):
    from dgvit_amd.optim import FlatAdamW, LRSchedule, home_of
    sched = LRSchedule(kind, warmup_steps=2, total_steps=6, final_ratio=0.1)
    base, img, pstate = _policy(amd, 52)
    a, b = copy.deepcopy(base), copy.deepcopy(base)
    home_of(a)
    oa = FlatAdamW(_our_groups(a), schedule=sched, **HYPER)
    ob = torch.optim.AdamW(_torch_groups(b), **HYPER)
    lam = torch.optim.lr_scheduler.LambdaLR(ob, lambda s: sched.factor(s))
    for it in range(8):
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad(set_to_none=True)
            _loss(m, img, pstate, it).backward()
        oa.step()
        ob.step()
        want = np.array([lr * sched.factor(it) for lr in (3e-3, 3e-3, HEAD_LR)])
        np.testing.assert_allclose([g["lr"] for g in ob.param_groups], want, rtol=1e-12)       # torch used the same rates
        lam.step()
        got = oa.last_lr.cpu().double().numpy()
        print(f"{kind} step {it}: last_lr {got.tolist()} want {want.tolist()}")
        np.testing.assert_allclose(got, want, rtol=1e-6)
    assert oa.step_count == 8 and [g["lr"] for g in oa.param_groups] == [3e-3, 3e-3, HEAD_LR]      # the base rates stay what they were
    for (k, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), err_msg=k, **ADAM_TOL)


# ------------------------------------------------------------------------------------------------ 5. + 6. capture, set_lr
def _state_of(opt):
    """(parameters, exp_avg, exp_avg_sq) of every parameter that has taken a step, cloned"""
    sd = opt.state_dict()
    ps = [p.detach().clone() for p in opt.params]
    return ps, [s["exp_avg"] for s in sd["state"] if s is not None], [s["exp_avg_sq"] for s in sd["state"] if s is not None]


def test_graphed_adamw_follows_the_schedule_and_set_lr(amd):
    """FlatAdamW(capturable, groups, schedule, max_grad_norm) inside GraphedStep: K replays == K eager steps of a twin that passes the
    step from the host, bit for bit; last_lr follows the schedule across replays; set_lr reaches the next replay"""
    from dgvit_amd.optim import FlatAdamW, LRSchedule, home_of
    sched = LRSchedule("cosine", warmup_steps=2, total_steps=12, final_ratio=0.1)
    base, img, pstate = _policy(amd, 61, batch=8)
    probe = copy.deepcopy(base)
    _loss(probe, img, pstate, 0).backward()
    max_norm = 0.25 * math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in probe.parameters() if p.grad is not None))

    def make(model, capturable):
        home_of(model)
        opt = FlatAdamW(_our_groups(model), capturable=capturable, schedule=sched, max_grad_norm=max_norm, **HYPER)

        def step():
            opt.zero_grad(set_to_none=True)
            loss = _loss(model, img, pstate, 0)
            loss.backward()
            opt.step()
            return loss.detach()
        return step, opt

    ma, mb = copy.deepcopy(base), copy.deepcopy(base)
    step_a, opt_a = make(ma, False)
    step_b, opt_b = make(mb, True)
    graph = amd.GraphedStep(step_b, warmup=3)          # 3 warm-up steps inside; the capture pass itself executes nothing
    for _ in range(3):
        step_a()
    base_lr = [3e-3, 3e-3, HEAD_LR]
    for k in range(4):
        step_a()
        graph()
        want = np.array([lr * sched.factor(3 + k) for lr in base_lr])
        got = opt_b.last_lr.cpu().double().numpy()
        print(f"replay {k}: last_lr {got.tolist()} want {want.tolist()} grad norm {opt_b.last_grad_norm.item()!r}")
        np.testing.assert_allclose(got, want, rtol=1e-6)
        assert torch.equal(opt_a.last_lr, opt_b.last_lr)
    torch.cuda.synchronize()
    sa, sb = _state_of(opt_a), _state_of(opt_b)
    for xs, ys, what in zip(sa, sb, ("parameter", "exp_avg", "exp_avg_sq")):
        assert len(xs) == len(ys) > 20
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert torch.equal(x, y), f"{what} {i}: replayed and eager steps differ"
    assert opt_b.state_dict()["step"] == 7
    # ---- set_lr: 0 freezes the parameters of the next replay (and of the next eager step), the moments go on; the old rates move them again
    for run, opt in ((graph, opt_b), (step_a, opt_a)):
        opt.set_lr(0.0)
        assert [g["lr"] for g in opt.param_groups] == [0.0] * 3
        before = _state_of(opt)
        run()
        after = _state_of(opt)
        assert all(torch.equal(x, y) for x, y in zip(before[0], after[0])), "a parameter moved at lr = 0"
        assert not any(torch.equal(x, y) for x, y in zip(before[1], after[1])), "exp_avg stood still"
        assert torch.equal(opt.last_lr, torch.zeros(3, device="cuda"))
        for gidx, lr in enumerate(base_lr):
            opt.set_lr(lr, group=gidx)
        run()
        moved = _state_of(opt)
        n_moved = sum(not torch.equal(x, y) for x, y, p in zip(after[0], moved[0], opt.params) if p.grad is not None)
        assert n_moved == sum(p.grad is not None for p in opt.params), "parameters did not move again after set_lr(old)"
        np.testing.assert_allclose(opt.last_lr.cpu().double().numpy(), np.array([lr * sched.factor(8) for lr in base_lr]), rtol=1e-6)
    for x, y in zip(_state_of(opt_a)[0], _state_of(opt_b)[0]):
        assert torch.equal(x, y), "replayed and eager steps differ after set_lr"
    for bad in (-1.0, math.nan, math.inf, "1e-3", True, None):
        with pytest.raises(ValueError, match="set_lr"):
            opt_a.set_lr(bad)
    for bad in (3, -1, 1.0, True):
        with pytest.raises(ValueError, match="group"):
            opt_a.set_lr(1e-3, group=bad)


# ------------------------------------------------------------------------------------------------ 7. state_dict
def _toy(seed):
    """a Linear and two loose tensors with seeded parameters; gradients are assigned by hand, so every step is deterministic"""
    gen = torch.Generator().manual_seed(seed)
    lin = torch.nn.Linear(37, 19)
    with torch.no_grad():
        for p in lin.parameters():
            p.copy_(torch.randn(p.shape, generator=gen))
    lin = lin.cuda()
    loose = [torch.randn(5, 3, generator=gen).cuda().requires_grad_(), torch.randn(1, generator=gen).cuda().requires_grad_()]
    return lin, loose


def _toy_step(opt, lin, loose, it):
    for k, p in enumerate([*lin.parameters(), *loose]):
        p.grad = _randn(p.numel(), 7000 + 10 * it + k).view_as(p)
    opt.step()


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_state_dict_round_trip(amd, capturable):
    from dgvit_amd.optim import FlatAdamW, LRSchedule

    def make(lin, loose, schedule, lrs=(3e-3, 1e-2)):
        return FlatAdamW([{"params": lin, "lr": lrs[0], "weight_decay": 0.05}, {"params": loose, "lr": lrs[1], "weight_decay": 0.0}],
                         eps=1e-3, capturable=capturable, schedule=schedule)

    sched = LRSchedule("linear", warmup_steps=2, total_steps=7, final_ratio=0.2)
    lin_a, loose_a = _toy(1)
    oa = make(lin_a, loose_a, sched)
    for it in range(5):
        _toy_step(oa, lin_a, loose_a, it)
    lin_b, loose_b = _toy(1)
    ob = make(lin_b, loose_b, sched)
    for it in range(3):
        _toy_step(ob, lin_b, loose_b, it)
    ob.set_lr(4e-3, group=0)          # (an lr changed on the way is part of the state; the straight run sees it from step 3 on as well)
    sd = ob.state_dict()
    assert {"step", "lr", "betas", "eps", "weight_decay", "state", "decoupled", "schedule", "groups"} == set(sd)
    assert sd["step"] == 3 and sd["decoupled"] is True and sd["groups"] == [{"lr": 4e-3, "weight_decay": 0.05}, {"lr": 1e-2, "weight_decay": 0.0}]
    assert sd["schedule"] == {"kind": "linear", "warmup_steps": 2, "total_steps": 7, "final_ratio": 0.2}
    # the straight run: the same change at the same place
    lin_s, loose_s = _toy(1)
    os_ = make(lin_s, loose_s, sched)
    for it in range(3):
        _toy_step(os_, lin_s, loose_s, it)
    os_.set_lr(4e-3, group=0)
    for it in range(3, 5):
        _toy_step(os_, lin_s, loose_s, it)
    # a fresh optimiser on a twin of the parameters, built with OTHER rates and no schedule: everything comes from the state
    lin_c, loose_c = _toy(2)
    with torch.no_grad():
        for dst, src in zip([*lin_c.parameters(), *loose_c], [*lin_b.parameters(), *loose_b]):
            dst.copy_(src)
    oc = make(lin_c, loose_c, None, lrs=(1.0, 1.0))
    oc.load_state_dict(sd)
    assert oc.step_count == 3 and [g["lr"] for g in oc.param_groups] == [4e-3, 1e-2] and oc.schedule.state_dict() == sd["schedule"]
    for it in range(3, 5):
        _toy_step(oc, lin_c, loose_c, it)
    want = 1e-2 * sched.factor(4)
    assert abs(oc.last_lr[1].item() - want) <= 1e-6 * want, "the schedule position was not restored"
    for x, y in zip([*lin_c.parameters(), *loose_c], [*lin_s.parameters(), *loose_s]):
        assert torch.equal(x, y), "five steps with a save / load after three differ from five straight steps"
    sc, ss = oc.state_dict(), os_.state_dict()
    assert sc["step"] == ss["step"] == 5
    for x, y in zip(sc["state"], ss["state"]):
        assert x["step"] == y["step"] == 5 and torch.equal(x["exp_avg"], y["exp_avg"]) and torch.equal(x["exp_avg_sq"], y["exp_avg_sq"])
    assert not torch.equal(lin_a.weight, lin_s.weight), "set_lr(4e-3) changed nothing: the comparison above shows less than it should"
    # a dict from before there were groups is accepted and leaves groups and schedule alone
    old = {k: v for k, v in sd.items() if k not in ("decoupled", "schedule", "groups")}
    oc.load_state_dict(old)
    assert [g["lr"] for g in oc.param_groups] == [4e-3, 1e-2] and oc.schedule is not None and oc.step_count == 3


# ------------------------------------------------------------------------------------------------ 8. past 2 GiB
def test_segment_boundary_past_2_gib(amd):
    """n = 2^29 + 4 * 257 floats per buffer (2 GiB + 4 KiB): two segments with the same hyper-parameters whose boundary lies beyond byte
    2^31 must give dgvit_adam_step's bits.  Needs p, m, v twice and g once, 14 GiB, plus 3 GiB for torch's comparisons."""
    from dgvit_amd import _lib as L
    n = (1 << 29) + 4 * 257
    need_device_memory(17 * GIB)
    n4 = n // 4
    cut = (1 << 27) + 100                                     # float4 index: byte 2^31 + 1600
    assert 16 * cut > 1 << 31 and cut < n4
    g = _randn(n, 81)
    new = [_randn(n, 80), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")]
    old = [t.clone() for t in new]
    lr, wd = 3e-3, 0.01
    end4 = torch.tensor([cut, n4], dtype=torch.int64).cuda()
    group = torch.tensor([0, 1], dtype=torch.uint8).cuda()
    hyper = torch.tensor([[lr, wd], [lr, wd]], dtype=torch.float32, device="cuda")
    step_dev = torch.ones(1, dtype=torch.int64, device="cuda")
    _groups_call(new, g, n, end4, group, 2, hyper, 2, 0, 1)
    L.check(L.load().dgvit_adam_step(_p(old[0]), _p(g), _p(old[1]), _p(old[2]), n, lr, BETA1, BETA2, EPS, wd, 1, _p(step_dev), _stream()),
            "dgvit_adam_step")
    for x, y, name in zip(new, old, "pmv"):
        assert torch.equal(x, y), f"{name} differs from dgvit_adam_step"
    assert new[1][-1].item() != 0.0 and new[1][4 * cut].item() != 0.0 and new[1][4 * cut - 1].item() != 0.0
    del g, new, old
    torch.cuda.empty_cache()
