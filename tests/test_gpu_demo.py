"""GPU: learning from demonstrations -- replay.sample_mixed / update_priorities_mixed against each ring's own sample(),
bit for bit; functional.tanh_gaussian_log_prob and the policies' log_prob, sac_losses.bc_loss and nll_loss against the float64
restatement tests/demo_ref.py.

The rule of the parity tests is test_gpu_sac_losses.test_kernel_parity's: per output, max |hip - ref64| / max |ref64|, the largest over
the cases, against 2 x the same quantity of the restatement's own fp32 evaluation on the CPU -- the yardstick, nothing of it comes from
the HIP side -- and 2^-23 relative wherever that fp32 evaluation is exact.  The tests print the tables; DESIGN 3.46 holds the figures
measured on an MI355X."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import demo_ref as D  # noqa: E402

MARGIN = 2.0
_CACHE = {}


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


def _rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


def _table(title, names, hip, yard):
    print(f"\n{title}: output  hip  yardstick  hip/yardstick")
    for k in names:
        print(f"  {k:12s} {hip[k]:.3e}  {yard[k]:.3e}  {hip[k] / yard[k] if yard[k] > 0 else math.inf:.2f}")


# ================================================================================================ sample_mixed
KINDS = {     # name -> (class is prioritized, constructor keywords, slots)
    "f32": (False, dict(), 32),
    "u8": (False, dict(frame_dtype=torch.uint8), 16),
    "shared": (False, dict(shared_next_obs=True), 32),
    "env2": (False, dict(num_envs=2), 24),
    "per": (True, dict(), 64),
    "per_u8": (True, dict(frame_dtype=torch.uint8), 16),
}


def _build(amd, kind, shape, copy):
    """a ring of the kind, filled past its end (1.5 x its slots, so it has wrapped) with k / 255 frames, episodes of 5 steps and a few
    ``done``; the same (kind, shape) gives the same ring whatever ``copy``, and a ring is built once per module"""
    key = ("ring", kind, shape, copy)
    if key in _CACHE:
        return _CACHE[key]
    from dgvit_amd import replay
    per, kw, size = KINDS[kind]
    cls = replay.PrioritizedDeviceReplayBuffer if per else replay.DeviceReplayBuffer
    ring = cls(size, obs_shape=shape, pstate_dim=2, act_dim=2, seed=11, **kw)
    ring.track_episodes()
    E = ring.num_envs
    g = torch.Generator().manual_seed(sum(map(ord, kind)) + shape[0])
    steps = size * 3 // 2 // E
    frames = torch.randint(0, 256, (steps + 1, E, *shape), generator=g).float() / 255
    for t in range(steps):
        ring.add_vec(obs=frames[t], next_obs=frames[t + 1], pobs=torch.randn(E, 2, generator=g), next_pobs=torch.randn(E, 2, generator=g),
                     act=torch.randn(E, 2, generator=g), rew=torch.randn(E, generator=g), done=(torch.rand(E, generator=g) < 0.1).float(),
                     episode_end=torch.full((E,), t % 5 == 4))
    if per:
        ring.update_priorities(torch.arange(ring.stored), (torch.rand(ring.stored, generator=g) * 3).cuda())
    _CACHE[key] = ring
    return ring


def _both(amd, kinds, shape):
    """two identical sets of rings with their generators at the same state"""
    sets = [[_build(amd, k, shape, (c, i)) for i, k in enumerate(kinds)] for c in (0, 1)]
    for rings in sets:
        for i, r in enumerate(rings):
            r.gen.manual_seed(100 + i)
    return sets


def _is_per(ring):
    from dgvit_amd import replay
    return isinstance(ring, replay.PrioritizedDeviceReplayBuffer)


def _own(ring, n, kw, beta=0.4):
    return ring.sample(n, beta=beta, **kw) if _is_per(ring) else ring.sample(n, **kw)


def _check_contract(amd, kinds, counts, shape, kw, seed=5):
    """sample_mixed on one set of rings against each ring's own sample on the other: bit for bit, key for key"""
    from dgvit_amd import replay
    mixed_rings, own_rings = _both(amd, kinds, shape)
    states = [r.gen.get_state() for r in mixed_rings]
    torch.manual_seed(seed)
    batch = replay.sample_mixed(list(zip(mixed_rings, counts)), **kw)
    torch.manual_seed(seed)
    own = [_own(r, n, kw) if n else None for r, n in zip(own_rings, counts)]
    total = sum(counts)
    assert isinstance(batch, dict) and batch["counts"] == tuple(counts) and batch.rings == tuple(mixed_rings)
    keys = set().union(*(set(o) for o in own if o is not None))
    if any(_is_per(r) for r in mixed_rings):
        keys.add("weights")
    assert set(batch) == keys | {"source", "counts"}, (sorted(batch), sorted(keys))
    want_source = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(counts)])
    assert batch["source"].dtype == torch.int32 and torch.equal(batch["source"].cpu(), want_source)
    r0 = 0
    for i, (o, n) in enumerate(zip(own, counts)):
        if o is None:
            assert torch.equal(mixed_rings[i].gen.get_state(), states[i]), "a ring with a share of 0 does not draw"
            continue
        assert not torch.equal(mixed_rings[i].gen.get_state(), states[i]) or "indices" in kw
        for k in keys:
            rows = batch[k][r0:r0 + n]
            if k == "weights" and k not in o:
                assert torch.equal(rows, torch.ones(n, 1, device="cuda")), "a uniform ring's rows weigh 1"
                continue
            assert rows.shape == o[k].shape and rows.dtype == o[k].dtype, (k, rows.shape, o[k].shape)
            assert torch.equal(rows, o[k]), (kinds, counts, kw, i, k)
        assert int(o["indexes"].max()) < mixed_rings[i].stored, "indexes are slots of the row's own ring"
        r0 += n
    probe = _own(own_rings[0], total, kw)        # a plain sample of as many rows: the same layout
    for k in keys - {"weights"}:
        assert batch[k].shape == probe[k].shape and batch[k].stride() == probe[k].stride(), (k, batch[k].stride(), probe[k].stride())
    if kw.get("frame_stack"):
        assert batch["obs"].is_contiguous() and batch["next_obs"].is_contiguous() and batch["obs"].shape == (total, *shape, kw["frame_stack"])
    return batch, own, mixed_rings, own_rings


PLAIN = dict()
ALL3 = dict(random_shift=2, return_shifts=True, n_step=3, gamma=0.9, frame_stack=3)
KEYWORDS = {"plain": PLAIN, "shift": dict(random_shift=2, return_shifts=True), "nstep": dict(n_step=3, gamma=0.9), "stack": dict(frame_stack=3),
            "all3": ALL3, "shifts_without_shift": dict(return_shifts=True)}
SHAPES = [(6, 10), (5, 7)]      # rows of 60 floats, and of 35: no multiple of 4, so rows are padded and a stack's last copy is real


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("counts", [(5, 3), (1, 1), (7, 0), (0, 4)], ids=str)
@pytest.mark.parametrize("kw", ["plain", "all3"])
def test_mixed_rows_are_each_rings_own_sample(amd, shape, counts, kw):
    _check_contract(amd, ("f32", "u8"), counts, shape, KEYWORDS[kw])


@pytest.mark.parametrize("kw", list(KEYWORDS))
def test_every_keyword_of_sample(amd, kw):
    _check_contract(amd, ("u8", "f32"), (5, 3), (5, 7), KEYWORDS[kw])


@pytest.mark.parametrize("kinds", [("u8", "f32"), ("shared", "f32"), ("f32", "shared"), ("env2", "f32"), ("f32", "env2"), ("per", "f32"),
                                   ("u8", "per"), ("per", "per_u8")], ids="-".join)
@pytest.mark.parametrize("kw", ["plain", "all3"])
def test_every_kind_of_ring(amd, kinds, kw):
    batch, own, *_ = _check_contract(amd, kinds, (5, 3), (5, 7), KEYWORDS[kw])
    if "per" in kinds[0] or "per" in kinds[1]:
        w = batch["weights"]
        assert w.shape == (8, 1) and bool((w > 0).all()) and bool((w <= 1).all()) and bool((w < 1).any()), "the importance weights are the ring's own"


def test_three_rings(amd):
    for kw in (PLAIN, ALL3):
        _check_contract(amd, ("f32", "per", "u8"), (2, 3, 1), (6, 10), kw)
        _check_contract(amd, ("f32", "per", "u8"), (2, 0, 1), (6, 10), kw)


def test_given_indices_and_uniforms(amd):
    from dgvit_amd import replay
    (a, p, u), (a2, p2, u2) = _both(amd, ("f32", "per", "u8"), (5, 7))
    ia, iu = torch.tensor([3, 31, 0, 17, 17], device="cuda"), torch.tensor([15, 2], dtype=torch.int32)
    un = torch.tensor([0.0, 0.999, 0.5, 0.25], device="cuda")
    batch = replay.sample_mixed([(a, 5), (p, 4), (u, 2)], indices=[ia, None, iu], uniforms=[None, un, None], beta=0.7, stratified=True, n_step=2)
    own = [a2.sample(5, indices=ia, n_step=2), p2.sample(4, beta=0.7, stratified=True, uniforms=un, n_step=2), u2.sample(2, indices=iu, n_step=2)]
    assert torch.equal(batch["indexes"][:5], ia) and torch.equal(batch["indexes"][9:].cpu(), iu.long())
    for k in own[1]:
        want = torch.cat([o[k] if k in o else torch.ones(o["rew"].shape[0], 1, device="cuda") for o in own])
        assert torch.equal(batch[k], want), k


def test_update_priorities_mixed_routes_the_row_ranges(amd):
    from dgvit_amd import replay
    (p, a, q), (p2, a2, q2) = _both(amd, ("per", "f32", "per_u8"), (6, 10))
    before = [r.priorities() for r in (p, q)]
    batch = replay.sample_mixed([(p, 5), (a, 3), (q, 4)], beta=0.5)
    own = [p2.sample(5, beta=0.5), a2.sample(3), q2.sample(4, beta=0.5)]
    td = torch.rand(12, 1, generator=torch.Generator().manual_seed(3)).cuda() * 4
    replay.update_priorities_mixed(batch, td)
    p2.update_priorities(own[0]["indexes"], td[:5])
    q2.update_priorities(own[2]["indexes"], td[8:])
    try:
        for mine, theirs, old in ((p, p2, before[0]), (q, q2, before[1])):
            assert torch.equal(mine.tree, theirs.tree), "the whole tree, leaves and sums, is the ring's own update_priorities'"
            assert not torch.equal(mine.priorities(), old)
        replay.update_priorities_mixed(batch, td.reshape(-1))            # (B,) is the same argument
        assert torch.equal(p.tree, p2.tree)
        only_uniform = replay.sample_mixed([(a, 2)])
        assert "weights" not in only_uniform
        replay.update_priorities_mixed(only_uniform, td[:2])             # nothing to route
        zero_share = replay.sample_mixed([(a, 2), (p, 0)])
        assert torch.equal(zero_share["weights"], torch.ones(2, 1, device="cuda")), "the key is there whenever a ring of the list is prioritized"
    finally:
        for k in [k for k in _CACHE if k[0] == "ring" and k[1] in ("per", "per_u8")]:     # these rings' priorities have moved: rebuild them
            del _CACHE[k]


def test_a_captured_mixed_sample_follows_both_rings(amd):
    from dgvit_amd import replay
    from dgvit_amd.replay import DeviceReplayBuffer
    shape = (5, 7)
    rings = [DeviceReplayBuffer(16, obs_shape=shape, seed=1), DeviceReplayBuffer(16, obs_shape=shape, seed=2, frame_dtype=torch.uint8)]
    g = torch.Generator().manual_seed(0)

    def add(ring, n):
        for _ in range(n):
            f = torch.randint(0, 256, (2, *shape), generator=g).float() / 255
            ring.add(obs=f[0], next_obs=f[1], pobs=torch.randn(2, generator=g), next_pobs=torch.randn(2, generator=g), act=torch.randn(2, generator=g),
                     rew=float(torch.randn((), generator=g)), done=0.0)
    for r in rings:
        r.track_episodes()
        add(r, 16)
    fixed = [torch.tensor([0, 5, 15, 7, 7], device="cuda"), torch.tensor([3, 9, 12], device="cuda")]
    kw = dict(n_step=2, frame_stack=2, random_shift=1, return_shifts=True)

    def fn():
        return replay.sample_mixed([(rings[0], 5), (rings[1], 3)], indices=fixed, **kw)
    graph = amd.GraphedStep(fn, warmup=1)
    first = {k: v.clone() for k, v in graph().items() if torch.is_tensor(v)}
    for r in rings:
        add(r, 9)                       # slots 0 .. 8 of both rings are new, and the newest slot has moved
    out = graph()
    torch.cuda.synchronize()
    assert out["counts"] == (5, 3)
    r0 = 0
    for r, idx in zip(rings, fixed):
        n = idx.numel()
        # the shifts are the replay's own draw: the plain stacks at the same slots, shifted by the returned table, are the reference
        plain = r.sample(n, indices=idx, n_step=2, frame_stack=2)
        for k in ("pobs", "act", "rew", "next_pobs", "done", "discount", "steps", "indexes"):
            assert torch.equal(out[k][r0:r0 + n], plain[k]), k
        for k in ("obs", "next_obs"):
            sh = out[k + "_shift"][r0:r0 + n].cpu()
            src = torch.nn.functional.pad(plain[k].permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").cpu()
            want = torch.stack([src[j, :, 1 + int(sh[j, 0]):1 + int(sh[j, 0]) + shape[0], 1 + int(sh[j, 1]):1 + int(sh[j, 1]) + shape[1]] for j in range(n)])
            assert torch.equal(out[k][r0:r0 + n].cpu(), want.permute(0, 2, 3, 1)), k
        r0 += n
    assert not torch.equal(out["act"][:5], first["act"][:5]) and not torch.equal(out["act"][5:], first["act"][5:]), "both rings moved, and the replay followed"


def _launches(amd, run):
    """the library's own launch totals (per profile kind) of one run, as tests/test_gpu_profile_census.py reads them"""
    from dgvit_amd import _lib
    lib = amd.load_library()
    torch.cuda.synchronize()
    kinds = _lib.PROFILE_KINDS
    assert lib.dgvit_profile_sampling(1) == 0
    try:
        assert lib.dgvit_profile_start(8192) == 0
        run()
        torch.cuda.synchronize()
        ms, work, cnt = (ctypes.c_double * kinds)(), (ctypes.c_double * kinds)(), (ctypes.c_longlong * kinds)()
        assert lib.dgvit_profile_stop(ms, work, cnt) == 0, lib.dgvit_last_error()
        work_all, cnt_all = (ctypes.c_double * kinds)(), (ctypes.c_longlong * kinds)()
        assert lib.dgvit_profile_totals(work_all, cnt_all) == 0
    finally:
        lib.dgvit_profile_sampling(1)
    return list(cnt_all)


@pytest.mark.parametrize("kw", ["plain", "all3"])
def test_a_mixed_call_launches_what_its_rings_launch(amd, kw):
    from dgvit_amd import replay
    kw = KEYWORDS[kw]
    (a, p, u), (a2, p2, u2) = _both(amd, ("f32", "per", "u8"), (5, 7))
    run_own = lambda: (a2.sample(5, **kw), p2.sample(3, **kw), u2.sample(2, **kw))  # noqa: E731
    run_mixed = lambda: replay.sample_mixed([(a, 5), (p, 3), (u, 2)], **kw)  # noqa: E731
    run_own(), run_mixed()
    own, mixed = _launches(amd, run_own), _launches(amd, run_mixed)
    print(f"library launches per kind: three sample() calls {own}, one sample_mixed {mixed}")
    assert sum(own) > 0 and mixed == own
    assert _launches(amd, lambda: replay.sample_mixed([(a, 5), (p, 0), (u, 0)], **kw)) == _launches(amd, lambda: a2.sample(5, **kw))


class _CountingLib:
    """the object ``_lib.load()`` returns, every ``dgvit_*`` entry point counting its calls: the gathers, the walk, the row tables and
    dgvit_ring_next_rows do not pass the profile bracket, so ``_launches`` sees none of them"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dgvit_"):
            return fn

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


# the library entry points ONE sample(5, ...) calls, per ring kind and keyword set, each of them one launch: read once through
# _CountingLib on the commit before sample, the prioritized sample and sample_mixed became one path, and kept as literals.  7 gathers for
# a plain call; the walk in the place of three of them with n_step; dgvit_ring_next_rows more for an unstacked call on a shared ring; the
# row tables and two stacked gathers in the place of the two frame gathers with frame_stack; the draw more on a prioritized ring
SAMPLE_LAUNCHES = {
    "f32": dict(plain=7, shift=7, nstep=5, stack=8, all3=6),
    "u8": dict(plain=7, shift=7, nstep=5, stack=8, all3=6),
    "shared": dict(plain=8, shift=8, nstep=6, stack=8, all3=6),
    "env2": dict(plain=7, shift=7, nstep=5, stack=8, all3=6),
    "per": dict(plain=8, shift=8, nstep=6, stack=9, all3=7),
}


@pytest.mark.parametrize("kind", list(SAMPLE_LAUNCHES))
def test_a_plain_sample_launches_what_it_launched(amd, kind, monkeypatch):
    """test_a_mixed_call_launches_what_its_rings_launch compares one path with itself; these literals anchor the count.  Of them the
    profile counters (``_launches``) see the prioritized draw alone, on that commit as on this one."""
    from dgvit_amd import _lib
    ring = _build(amd, kind, (5, 7), ("launches", 0))
    for name, want in SAMPLE_LAUNCHES[kind].items():
        run = lambda: _own(ring, 5, KEYWORDS[name])  # noqa: E731
        run()
        assert sum(_launches(amd, run)) == int(kind == "per"), (kind, name)
        counting = _CountingLib(_lib.load())
        with monkeypatch.context() as mp:
            mp.setattr(_lib, "_lib", counting)
            run()
        torch.cuda.synchronize()
        print(f"entry points of one sample(5): {kind} {name} {sum(counting.calls.values())} {counting.calls}")
        assert sum(counting.calls.values()) == want, (kind, name, counting.calls, want)


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("kw", ["plain", "all3"])
def test_given_indices_are_adopted_not_copied(amd, kind, kw):
    """a contiguous int64 tensor on the ring's device IS the result's ``indexes``: no copy, which the library's counters would not see"""
    ring = _build(amd, kind, (5, 7), ("launches", 0))
    t = torch.tensor([3, 15, 0, 7, 7], device="cuda")
    out = ring.sample(5, indices=t, **KEYWORDS[kw])
    assert out["indexes"].data_ptr() == t.data_ptr() and torch.equal(out["indexes"], t)


# ================================================================================================ log_prob
LP_B, LP_A = (1, 37, 257, 300), (1, 2, 3, 16)     # 257 crosses the 256-thread block; A = 3 is no power of two, 16 the limit
LP_OUT = ("log_prob", "dmean", "dlog_std")


def _lp_inputs(Bn, A, per_action):
    """fp32 CPU tensors.  log_std_raw walks a fixed ladder -- below LOG_SIG_MIN, on it, inside, on LOG_SIG_MAX, above -- so every case has
    every kind; of the actions, tanh(N(0, 1.5)) scale + bias, every 5th element is set exactly to a bound and every 11th beyond it."""
    key = ("lp", Bn, A, per_action)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(7000 + 100 * Bn + 2 * A + per_action)
        n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
        scale = (0.5 + torch.rand(A, generator=g)) if per_action else torch.tensor(1.7)
        bias = n(A) if per_action else torch.tensor(-0.3)
        ladder = torch.tensor([-25.0, D.LOG_SIG_MIN, -3.0, -1.0, 0.0, 0.7, D.LOG_SIG_MAX, 3.5])
        flat = torch.arange(Bn * A)
        lsr = (ladder[flat % 8] + torch.where((flat % 8 == 1) | (flat % 8 == 6), 0.0, 1.0) * 0.3 * n(Bn * A)).reshape(Bn, A)
        lsr = torch.where((flat % 8 == 0).reshape(Bn, A), lsr.clamp(max=-20.5), torch.where((flat % 8 == 7).reshape(Bn, A), lsr.clamp(min=2.5), lsr))
        y = torch.tanh(1.5 * n(Bn, A))
        sign = torch.where(y >= 0, 1.0, -1.0)
        y = torch.where((flat % 5 == 2).reshape(Bn, A), sign, y)
        y = torch.where((flat % 11 == 7).reshape(Bn, A), sign * 1.25, y)
        _CACHE[key] = dict(mean=n(Bn, A), lsr=lsr, action=y * scale + bias, scale=scale, bias=bias, up=n(Bn, 1))
    return _CACHE[key]


def _lp_reference(Bn, A, per_action, dtype):
    key = ("lpref", Bn, A, per_action, dtype)
    if key not in _CACHE:
        x = {k: v.to(dtype).clone() for k, v in _lp_inputs(Bn, A, per_action).items()}      # (to() of an fp32 tensor is the cached tensor itself)
        mean, lsr = x["mean"].requires_grad_(True), x["lsr"].requires_grad_(True)
        lp = D.log_prob(mean, lsr, x["action"], x["scale"], x["bias"])
        (lp * x["up"]).sum().backward()
        _CACHE[key] = {k: v.detach().double() for k, v in dict(log_prob=lp, dmean=mean.grad, dlog_std=lsr.grad).items()}
    return _CACHE[key]


def _lp_device(amd, Bn, A, per_action):
    x = {k: v.cuda() for k, v in _lp_inputs(Bn, A, per_action).items()}
    mean, lsr, action = x["mean"].requires_grad_(True), x["lsr"].requires_grad_(True), x["action"].requires_grad_(True)
    lp = amd.functional.tanh_gaussian_log_prob(mean, lsr, action, x["scale"], x["bias"], D.LOG_SIG_MIN, D.LOG_SIG_MAX)
    assert lp.shape == (Bn, 1) and bool(torch.isfinite(lp).all()), "actions at and beyond the bounds stay finite"
    (lp * x["up"]).sum().backward()
    assert action.grad is None, "nothing flows to the action"
    outside = (x["lsr"] < D.LOG_SIG_MIN) | (x["lsr"] > D.LOG_SIG_MAX)
    if Bn * A >= 8:
        assert outside.any() and (x["lsr"] == D.LOG_SIG_MIN).any() and (x["lsr"] == D.LOG_SIG_MAX).any()
    assert torch.equal(lsr.grad == 0, outside), "exactly 0 outside the clamp; the bounds count as inside (and e^2 = 1 does not occur)"
    return {k: v.detach().double().cpu() for k, v in dict(log_prob=lp, dmean=mean.grad, dlog_std=lsr.grad).items()}


def test_log_prob_parity(amd):
    hip, yard, exact = {k: 0.0 for k in LP_OUT}, {k: 0.0 for k in LP_OUT}, []
    for Bn in LP_B:
        for A in LP_A:
            for per_action in (False, True):
                r64, r32 = (_lp_reference(Bn, A, per_action, dt) for dt in (torch.float64, torch.float32))
                dev = _lp_device(amd, Bn, A, per_action)
                for k in LP_OUT:
                    assert dev[k].shape == r64[k].shape
                    h, y = _rel(dev[k], r64[k]), _rel(r32[k], r64[k])
                    hip[k], yard[k] = max(hip[k], h), max(yard[k], y)
                    if y == 0.0:
                        exact.append((k, Bn, A, h))
    _table("log_prob (margin 2)", LP_OUT, hip, yard)
    print("  outputs whose fp32 evaluation is exact:", sorted(set((k, b, a) for k, b, a, _ in exact)))
    for k, Bn, A, h in exact:
        assert h <= 2.0 ** -23, (k, Bn, A, h)
    for k in LP_OUT:
        assert yard[k] > 0, k
        assert hip[k] <= MARGIN * yard[k], (k, hip[k], yard[k])


def test_log_prob_away_from_the_clip_is_within_fp32_rounding(amd):
    """the yardstick above is dominated by the rows at the clip, where fp32 cannot even represent 1 - 1e-6; on rows with |y| <= 0.9 and
    log_std in [-3, 2] every term is well-conditioned; the device computes in double and rounds the sum once, so it is within 2^-24 of
    its own value of the reference (the double arithmetic's 1e-15 is the 1.01)"""
    g = torch.Generator().manual_seed(2)
    Bn, A = 300, 3
    mean, lsr = torch.randn(Bn, A, generator=g), torch.rand(Bn, A, generator=g) * 5 - 3
    scale, bias = 0.5 + torch.rand(A, generator=g), torch.randn(A, generator=g)
    action = torch.tanh(torch.randn(Bn, A, generator=g)).clamp(-0.9, 0.9) * scale + bias
    up = 0.5 + torch.rand(Bn, 1, generator=g)
    m64, l64 = mean.double().requires_grad_(True), lsr.double().requires_grad_(True)
    ref = D.log_prob(m64, l64, action.double(), scale.double(), bias.double())
    (ref * up.double()).sum().backward()
    md, ld = mean.cuda().requires_grad_(True), lsr.cuda().requires_grad_(True)
    got = amd.functional.tanh_gaussian_log_prob(md, ld, action.cuda(), scale.cuda(), bias.cuda(), D.LOG_SIG_MIN, D.LOG_SIG_MAX)
    (got * up.cuda()).sum().backward()
    err = _rel(got.detach().double().cpu(), ref.detach())
    print(f"log_prob away from the clip: {err:.3e} relative to the largest value ({err / 2.0 ** -24:.2f} x 2^-24)")
    assert err <= 1.01 * 2.0 ** -24
    # the backward as well: each gradient element is one double expression rounded once, so it is within 2^-24 of ITS OWN fp64 value
    # (element by element, which a backward evaluated in fp32 -- several roundings, and e^2 - 1 cancelling -- does not meet); the
    # 1e-12 of the largest value is the double arithmetic's own error where e^2 - 1 cancels
    for name, dev, want in (("dmean", md.grad, m64.grad), ("dlog_std", ld.grad, l64.grad)):
        diff, bound = (dev.double().cpu() - want).abs(), 1.01 * 2.0 ** -24 * want.abs() + 1e-12 * want.abs().max()
        worst = float((diff / want.abs().clamp(min=1e-30)).max())
        print(f"{name} away from the clip: worst element {worst:.3e} relative ({worst / 2.0 ** -24:.2f} x 2^-24)")
        assert bool((want != 0).all()) and bool((diff <= bound).all()), (name, worst)


def test_log_prob_wiring(amd):
    x = {k: v.cuda() for k, v in _lp_inputs(37, 2, True).items()}
    F = amd.functional
    args = (x["action"], x["scale"], x["bias"], D.LOG_SIG_MIN, D.LOG_SIG_MAX)
    mean, lsr = x["mean"].requires_grad_(True), x["lsr"].requires_grad_(True)
    lp = F.tanh_gaussian_log_prob(mean, lsr, *args)
    lp.sum().backward(retain_graph=True)
    g1, g2 = mean.grad.clone(), lsr.grad.clone()
    mean.grad = lsr.grad = None
    (4 * lp).sum().backward()               # a power of two: the backward rounds g e exp(-ls) once, and 4 x commutes with that rounding
    assert torch.equal(mean.grad, 4 * g1) and torch.equal(lsr.grad, 4 * g2) and g1.abs().max() > 0
    assert torch.equal(F.tanh_gaussian_log_prob(mean, lsr, *args), lp.detach()), "two calls give the same bits"
    with torch.no_grad():
        assert not F.tanh_gaussian_log_prob(mean, lsr, *args).requires_grad
    # a scalar scale / bias is the per-action one with equal entries
    one = F.tanh_gaussian_log_prob(mean, lsr, x["action"], torch.tensor(1.7).cuda(), torch.tensor(-0.3).cuda(), -20, 2)
    two = F.tanh_gaussian_log_prob(mean, lsr, x["action"], torch.full((2,), 1.7).cuda(), torch.full((2,), -0.3).cuda(), -20, 2)
    assert torch.equal(one, two)
    # the empty batch takes torch ops
    e = torch.zeros(0, 2, device="cuda", requires_grad=True)
    out = F.tanh_gaussian_log_prob(e, e, torch.zeros(0, 2, device="cuda"), x["scale"], x["bias"], -20, 2)
    assert out.shape == (0, 1)
    out.sum().backward()


def test_log_prob_through_the_modules(amd):
    """GoTPolicy.log_prob and GaussianPolicy.log_prob are the functional applied to forward()'s head outputs"""
    from dgvit_amd import sac_networks as N
    g = torch.Generator().manual_seed(4)

    class Space:
        high, low = np.array([1.0, 0.5], dtype=np.float32), np.array([-1.0, -0.1], dtype=np.float32)
    Bn = 5
    act = (torch.tanh(torch.randn(Bn, 2, generator=g)) * torch.tensor([1.0, 0.3]) + torch.tensor([0.0, 0.2])).cuda()
    act[0, 0], act[1, 1] = 1.0, 0.9            # at a bound and beyond one
    pstate = torch.randn(Bn, 2, generator=g).cuda()
    torch.manual_seed(0)
    got = amd.GoTPolicy(2, 2, 2, 2, 64, action_space=Space(), image_size=(84, 84), patch_size=(12, 12)).to("cuda").eval()     # sac_trajectory_ref's shapes
    cnn = amd.GaussianPolicy(2, 2, action_space=Space()).to("cuda").eval()       # (eval: a train-mode encoder draws new dropout masks per call)
    img = torch.rand(Bn, 84, 84, generator=g).cuda()
    for pol in (got, cnn):
        lp = pol.log_prob([img, pstate], act)
        mean, _ = pol.forward([img, pstate])
        _, lsr = pol._head_outputs([img, pstate])
        want = amd.functional.tanh_gaussian_log_prob(mean, lsr, act, pol.action_scale, pol.action_bias, N.LOG_SIG_MIN, N.LOG_SIG_MAX)
        assert lp.shape == (Bn, 1) and torch.equal(lp, want) and bool(torch.isfinite(lp).all())
        ref = D.log_prob(mean.detach().double().cpu(), lsr.detach().double().cpu(), act.double().cpu(), pol.action_scale.double().cpu(),
                         pol.action_bias.double().cpu())
        np.testing.assert_allclose(lp.detach().double().cpu().numpy(), ref.numpy(), rtol=1e-5)
        pol.zero_grad()
        lp.mean().backward()
        assert pol.mean_linear.weight.grad.abs().max() > 0 and pol.fc1.weight.grad.abs().max() > 0, "the likelihood trains the policy"


# ================================================================================================ bc_loss / nll_loss
BC_SHAPES = [(1, 1), (37, 2), (300, 3), (33, 7), (5, 16)]
MASKS = ("none", "bool", "float01", "weights")
BC_OUT = ("loss", "used", "grad")


def _bc_inputs(Bn, A):
    key = ("bc", Bn, A)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(500 * Bn + A)
        n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
        keep = torch.rand(Bn, generator=g) < 0.6
        keep[0] = True
        grid = lambda: torch.randint(-2048, 2048, (Bn, A), generator=g).float() / 1024      # multiples of 2^-10: sums of <= 16 are exact  # noqa: E731
        q = dict(q1d=grid(), q2d=grid(), q1p=grid(), q2p=grid())
        tie = torch.arange(Bn) % 3 == 1            # exact ties of the two row means: both sides the same numbers
        q["q1p"][tie], q["q2p"][tie] = q["q1d"][tie], q["q2d"][tie]
        if Bn >= 3:                                # ... and a tie of different numbers with the same mean
            q["q1d"][2], q["q2d"][2], q["q1p"][2], q["q2p"][2] = 0.5, 0.75, 0.5, 2.0
        _CACHE[key] = dict(pred=n(Bn, A), action=n(Bn, A), logp=3 * n(Bn, 1) - 2, up=torch.tensor(1.0) + torch.rand((), generator=g),
                           bool=keep, float01=keep.float().reshape(Bn, 1), weights=torch.where(keep, 0.25 + torch.rand(Bn, generator=g), 0.0), **q)
    return _CACHE[key]


def _bc_reference(Bn, A, kind, mask, filt, dtype):
    key = ("bcref", Bn, A, kind, mask, filt, dtype)
    if key not in _CACHE:
        x = _bc_inputs(Bn, A)
        m = None if mask == "none" else (x[mask] if mask == "bool" else x[mask].to(dtype))
        if kind == "bc":
            p = x["pred"].to(dtype).clone().requires_grad_(True)
            qd, qp = ((x["q1d"].to(dtype), x["q2d"].to(dtype)), (x["q1p"].to(dtype), x["q2p"].to(dtype))) if filt else (None, None)
            loss, used = D.bc_loss(p, x["action"].to(dtype), m, qd, qp)
        else:
            p = x["logp"].to(dtype).clone().requires_grad_(True)
            loss, used = D.nll_loss(p, m)
        (loss * x["up"].to(dtype)).backward()
        _CACHE[key] = {k: v.detach().double() for k, v in dict(loss=loss, used=used, grad=p.grad).items()}
    return _CACHE[key]


def _bc_device(amd, Bn, A, kind, mask, filt):
    S = amd.sac_losses
    x = {k: v.cuda() for k, v in _bc_inputs(Bn, A).items()}
    m = None if mask == "none" else x[mask]
    if kind == "bc":
        p = x["pred"].requires_grad_(True)
        kw = dict(q_demo=(x["q1d"], x["q2d"]), q_pi=(x["q1p"], x["q2p"])) if filt else {}
        out = S.bc_loss(p, x["action"], mask=m, **kw)
    else:
        p = x["logp"].requires_grad_(True)
        out = S.nll_loss(p, mask=m)
    assert out.loss.shape == () and out.used.shape == () and not out.used.requires_grad and out.loss.requires_grad
    (out.loss * x["up"]).backward()             # a non-unit upstream gradient
    assert x["action"].grad is None
    return {k: v.detach().double().cpu() for k, v in dict(loss=out.loss, used=out.used, grad=p.grad).items()}


@pytest.mark.parametrize("kind", ["bc", "bc_filtered", "nll"])
def test_demonstration_loss_parity(amd, kind):
    filt, base = kind == "bc_filtered", "nll" if kind == "nll" else "bc"
    hip, yard, exact = {k: 0.0 for k in BC_OUT}, {k: 0.0 for k in BC_OUT}, []
    for Bn, A in BC_SHAPES:
        for mask in MASKS:
            r64, r32 = (_bc_reference(Bn, A, base, mask, filt, dt) for dt in (torch.float64, torch.float32))
            dev = _bc_device(amd, Bn, A, base, mask, filt)
            if filt:                           # the grid makes every decision exact: the count of rows is the reference's, to the bit
                x = _bc_inputs(Bn, A)
                f = torch.minimum(x["q1d"], x["q2d"]).double().mean(1) > torch.minimum(x["q1p"], x["q2p"]).double().mean(1)
                ties = torch.minimum(x["q1d"], x["q2d"]).double().mean(1) == torch.minimum(x["q1p"], x["q2p"]).double().mean(1)
                assert (Bn < 3 or ties.sum() >= 2) and not bool((f & ties).any()), "there are exact ties, and a tie does not apply"
                if mask in ("none", "bool", "float01"):
                    assert float(dev["used"]) == float(r64["used"]) == float((f & (x["bool"] if mask != "none" else True)).sum())
            if float(r64["used"]) == 0:        # nothing applies in this case (a filter that rejects the only row): exact zeros
                assert float(dev["loss"]) == 0 and float(dev["used"]) == 0 and not dev["grad"].any()
                continue
            for k in BC_OUT:
                assert dev[k].shape == r64[k].shape, (k, dev[k].shape, r64[k].shape)
                h, y = _rel(dev[k], r64[k]), _rel(r32[k], r64[k])
                hip[k], yard[k] = max(hip[k], h), max(yard[k], y)
                if y == 0.0:
                    exact.append((k, Bn, A, mask, h))
    _table(f"{kind} (margin 2)", BC_OUT, hip, yard)
    print("  outputs whose fp32 evaluation is exact:", sorted(set(e[:4] for e in exact)), max((e[-1] for e in exact), default=0.0))
    for *where, h in exact:
        assert h <= 2.0 ** -23, (where, h)
    for k in BC_OUT:
        assert yard[k] > 0, k
        assert hip[k] <= MARGIN * yard[k], (k, hip[k], yard[k])


@pytest.mark.parametrize("Bn, A", BC_SHAPES)
def test_nothing_applies_gives_exact_zeros(amd, Bn, A):
    S = amd.sac_losses
    x = {k: v.cuda() for k, v in _bc_inputs(Bn, A).items()}
    zeros = (torch.zeros(Bn, device="cuda"), torch.zeros(Bn, 1, dtype=torch.bool, device="cuda"))
    for m in zeros:
        p, lp = x["pred"].clone().requires_grad_(True), x["logp"].clone().requires_grad_(True)
        lp.data[0] = float("-inf")              # a row that does not count cannot poison the sum
        for out, leaf in ((S.bc_loss(p, x["action"], mask=m), p), (S.nll_loss(lp, mask=m), lp)):
            (2 * out.loss).backward()
            assert float(out.loss) == 0 and float(out.used) == 0 and torch.equal(leaf.grad, torch.zeros_like(leaf)), "zeros, never NaN"
    # a filter that rejects every row: q_pi above q_demo everywhere
    p = x["pred"].clone().requires_grad_(True)
    out = S.bc_loss(p, x["action"], q_demo=(x["q1d"], x["q2d"]), q_pi=(x["q1d"] + 1, x["q2d"] + 1))
    out.loss.backward()
    assert float(out.loss) == 0 and float(out.used) == 0 and not p.grad.any()
    # ... and one that is a tie everywhere
    out = S.bc_loss(p, x["action"], q_demo=(x["q1d"], x["q2d"]), q_pi=(x["q2d"], x["q1d"]))
    assert float(out.used) == 0


def test_masks_that_say_the_same_give_the_same_bits(amd):
    S = amd.sac_losses
    x = {k: v.cuda() for k, v in _bc_inputs(300, 3).items()}
    a = S.bc_loss(x["pred"], x["action"], mask=x["bool"])
    for m in (x["float01"], x["float01"].reshape(-1), x["bool"].reshape(-1, 1)):
        b = S.bc_loss(x["pred"], x["action"], mask=m)
        assert torch.equal(a.loss, b.loss) and torch.equal(a.used, b.used)
    ones = S.bc_loss(x["pred"], x["action"], mask=torch.ones(300, device="cuda"))
    none = S.bc_loss(x["pred"], x["action"])
    assert torch.equal(ones.loss, none.loss) and float(none.used) == 300
    assert float(a.used) == float(x["bool"].sum()) and not a.loss.requires_grad
    # the selected rows' plain mean, in fp32 on the device
    want = ((x["pred"] - x["action"])[x["bool"]] ** 2).mean()
    np.testing.assert_allclose(float(a.loss), float(want), rtol=1e-6)


def test_the_sum_of_policy_loss_and_demonstration_term_backpropagates_once(amd):
    """policy_loss + lambda bc.loss, one backward: log_pi, q and pred gradients against the fp64 restatement (pred feeds both terms' graphs
    in a real step; here the leaves are separate so that each gradient is checked on its own)"""
    import sac_losses_ref as R
    S = amd.sac_losses
    Bn, A, lam, alpha = 37, 2, 0.5, 0.2
    x = _bc_inputs(Bn, A)
    g = torch.Generator().manual_seed(9)
    extra = dict(lp=torch.randn(Bn, 1, generator=g), q1=torch.randn(Bn, A, generator=g), q2=torch.randn(Bn, A, generator=g))

    def run(dtype, dev):
        t = {k: v.to(dtype).clone().to(dev) for k, v in {**x, **extra}.items() if v.is_floating_point()}
        leaves = [t[k].requires_grad_(True) for k in ("lp", "q1", "q2", "pred")]
        if dev == "cuda":
            pl = S.actor_loss(t["lp"], t["q1"], t["q2"], alpha=alpha).policy_loss
            bc = S.bc_loss(t["pred"], t["action"], mask=x["bool"].cuda()).loss
        else:
            pl, bc = R.actor_loss(alpha, t["lp"], t["q1"], t["q2"]), D.bc_loss(t["pred"], t["action"], x["bool"])[0]
        total = pl + lam * bc
        total.backward()
        return [total.detach().double().cpu()] + [l.grad.double().cpu() for l in leaves]
    r64, r32, dev = run(torch.float64, "cpu"), run(torch.float32, "cpu"), run(torch.float32, "cuda")
    for name, d, a, b in zip(("total", "dlog_pi", "dq1", "dq2", "dpred"), dev, r64, r32):
        h, y = _rel(d, a), _rel(b, a)
        print(f"  {name:8s} {h:.3e}  {y:.3e}")
        assert h <= max(MARGIN * y, 2.0 ** -23), (name, h, y)


def test_a_captured_loss_follows_a_mask_refilled_between_replays(amd):
    S = amd.sac_losses
    Bn, A = 37, 2
    x = {k: v.cuda() for k, v in _bc_inputs(Bn, A).items()}
    mask = torch.ones(Bn, dtype=torch.bool, device="cuda")
    weights = torch.ones(Bn, device="cuda")
    pred, lp = x["pred"].requires_grad_(True), x["logp"].requires_grad_(True)

    def fn():
        pred.grad = lp.grad = None
        a, b = S.bc_loss(pred, x["action"], mask=mask, q_demo=(x["q1d"], x["q2d"]), q_pi=(x["q1p"], x["q2p"])), S.nll_loss(lp, mask=weights)
        (a.loss + 2 * b.loss).backward()
        return a.loss.detach(), a.used, b.loss.detach(), b.used, pred.grad, lp.grad
    graph = amd.GraphedStep(fn, warmup=1)
    seen = []
    for fill in (x["bool"], ~x["bool"], torch.zeros_like(x["bool"]), torch.ones_like(x["bool"])):
        mask.copy_(fill)
        weights.copy_(fill.float() * 0.5)
        out = [t.clone() for t in graph()]
        for a, b in zip(out, fn()):
            assert torch.equal(a, b), "a replay computes what an eager call computes with the mask of that time"
        seen.append(out)
    assert float(seen[2][1]) == 0 and float(seen[2][0]) == 0 and not seen[2][4].any() and not seen[2][5].any()
    assert float(seen[0][3]) == 0.5 * float(x["bool"].sum()) and float(seen[3][3]) == 0.5 * Bn
    assert float(seen[0][1]) + float(seen[1][1]) == float(seen[3][1]) > 0, "the two halves' rows are the whole's"


# ================================================================================================ trajectory
def _demo_case():
    import sac_trajectory_ref as T
    if "demo" not in _CACHE:
        case, stores, idx = D.make_demo_case()
        r64, r32 = (D.run_demo(case, stores, idx, dt, **T.BASE_KW) for dt in (torch.float64, torch.float32))
        _CACHE["demo"] = (case, stores, idx, r64, r32, T.distance(r32, r64, T.BASE_LR))
    case, stores, idx, r64, r32, Y = _CACHE["demo"]
    assert T.cap_violations(Y, D.DEMO_STEPS, T.BASE_LR) == [], "the reference's own fp32 run breaks the cap: the case is ill-conditioned"
    return _CACHE["demo"]


def _demo_hip_run(amd, case, stores, idx, captured, eager_steps=2):
    """The steps on the device: every batch from sample_mixed([(agent, 6), (demo, 2)]) at injected slots, the fused losses, the actor loss
    actor_loss(...).policy_loss + LAMBDA bc_loss(pi, act, mask=source == 1).loss, FlatAdam.  Captured: steps 0 .. eager_steps - 1 eager,
    the next GraphedStep's warm-up call, the rest replays -- test_gpu_sac_losses._hip_run's scheme."""
    import contextlib
    import copy
    import sac_trajectory_ref as T
    import dgvit_amd.sac_networks as N
    from dgvit_amd import replay
    from dgvit_amd.optim import FlatAdam, soft_update
    S = amd.sac_losses
    cfg, nsteps, batch = case["cfg"], len(case["steps"]), case["batch"]
    alpha, gamma, tau, lr = (T.BASE_KW[k] for k in ("alpha", "gamma", "tau", "lr"))
    pol = amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, image_size=cfg.image, patch_size=cfg.patch)
    pol.load_state_dict(dict(case["actor"]), strict=True)
    crt = amd.QNetwork(2, 2)
    crt.load_state_dict(dict(case["critic_params"]), strict=True)
    pol, crt = pol.cuda().eval(), crt.cuda().eval()
    tgt = copy.deepcopy(crt)
    op, oc = FlatAdam([pol], lr=lr, capturable=captured), FlatAdam([crt], lr=lr, capturable=captured)
    rings = [replay.DeviceReplayBuffer(2 * slots, obs_shape=cfg.image, seed=i) for i, slots in enumerate(D.DEMO_SLOTS)]
    for ring, store in zip(rings, stores):
        ring.add_batch(**store)
    slots = [torch.zeros(n, dtype=torch.int64, device="cuda") for n in D.DEMO_COUNTS]
    bufs = [torch.zeros(batch, 2, device="cuda") for _ in range(2)]
    calls = [0]

    def draw(like):
        calls[0] += 1
        return bufs[(calls[0] - 1) % 2]
    out = dict(qf=[], pl=[], used=[], source=[])

    def fill(k):
        for dst, src in zip(slots, idx[k]):
            dst.copy_(src)
        bufs[0].copy_(case["steps"][k]["e1"])
        bufs[1].copy_(case["steps"][k]["e2"])

    def learn():
        b = replay.sample_mixed(list(zip(rings, D.DEMO_COUNTS)), indices=slots)
        with torch.no_grad():
            na, nlogp, _ = pol.sample([b["next_obs"], b["next_pobs"]])
            q1n, q2n = tgt([b["next_obs"], b["next_pobs"], na])
        q1, q2 = crt([b["obs"], b["pobs"], b["act"]])
        c = S.critic_loss(q1, q2, b["rew"], q1n, q2n, nlogp, alpha=alpha, gamma=gamma)
        oc.zero_grad(); c.loss.backward(); oc.step()
        pi, logp, _ = pol.sample([b["obs"], b["pobs"]])
        q1p, q2p = crt([b["obs"], b["pobs"], pi])
        bc = S.bc_loss(pi, b["act"], mask=b["source"] == 1)
        pl = S.actor_loss(logp, q1p, q2p, alpha=alpha).policy_loss + D.LAMBDA * bc.loss
        op.zero_grad(); oc.zero_grad(); pl.backward(); op.step()
        soft_update(tgt, crt, tau)
        return dict(qf=c.loss.detach(), pl=pl.detach(), used=bc.used, source=b["source"])

    def record(o):
        torch.cuda.synchronize()
        out["qf"].append(float(o["qf"].double())), out["pl"].append(float(o["pl"].double())), out["used"].append(float(o["used"]))
        out["source"].append(o["source"].cpu().tolist())

    with contextlib.ExitStack() as stack:
        mp = stack.enter_context(pytest.MonkeyPatch.context())
        mp.setattr(N, "_standard_normal", draw)
        first_replay = nsteps
        if captured:
            for k in range(eager_steps):
                fill(k)
                record(learn())
            seen = []
            fill(eager_steps)
            graph = amd.GraphedStep(lambda: seen.append(learn()) or seen[-1], warmup=1)
            assert len(seen) == 2, "one warm-up call, which ran the step, and the capture, which ran nothing"
            record(seen[0])
            first_replay = eager_steps + 1
        for k in range(0 if not captured else first_replay, nsteps):
            fill(k)
            record(graph() if captured else learn())
    assert calls[0] > 0 and calls[0] % 2 == 0
    for net, m in (("actor", pol), ("critic", crt), ("target", tgt)):
        out[net] = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return out


@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_demonstration_regularised_trajectory(amd, mode):
    """GoTPolicy + CNN QNetwork at sac_trajectory_ref's base configuration, B = 6 agent + 2 demonstration rows from sample_mixed, four
    steps with the behaviour-cloning term in the actor loss, eager or captured from step 2, under sac_trajectory_ref.check (MARGIN 4)
    against the float64 host run of the same steps (demo_ref.run_demo)."""
    import sac_trajectory_ref as T
    case, stores, idx, r64, r32, Y = _demo_case()
    hip = _demo_hip_run(amd, case, stores, idx, captured=mode == "captured")
    d = T.distance(hip, r64, T.BASE_LR)
    r, bad = T.check(d, Y, D.DEMO_STEPS, T.BASE_LR)
    print(T.report(f"demonstration-regularised, {mode}", d, Y, r))
    print("  pl per step:", hip["pl"], "fp64:", r64["pl"], "used:", hip["used"])
    assert hip["used"] == r64["used"] == [2.0] * D.DEMO_STEPS and all(s == [0] * 6 + [1] * 2 for s in hip["source"])
    assert not bad, "\n".join(bad)
