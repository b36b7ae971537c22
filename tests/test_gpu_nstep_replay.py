"""GPU: n-step replay sampling -- dgvit_ring_mark, dgvit_nstep_walk, sample(..., n_step=, gamma=) of both buffers, and
critic_loss(discount=) through dgvit_sac_critic_loss_v2.

Everything is compared with the numpy restatement tests/nstep_ref.py (itself checked against the transition stream alone in
tests/test_nstep_replay_host.py), never with the code under test.  The ring has 37 slots of 6 x 10 frames; 52 transitions go through add
and add_batch mixed, so it wraps and 15 slots are overwritten; the frame of stream position t is replay_u8_ref.pattern(t) / 255, exact in
both ring formats.  ``rew`` must be within nstep_ref's derived tolerance of the float64 sum, ``discount`` within 2^-23 relative of
gamma^m, and both bit-equal where the arithmetic is exact (nstep_ref.exact); steps, next_obs, next_pobs, done and the indexes are exact.

Measured on an MI355X (the tests print the figures): largest |rew - ref64| / tolerance 0.417 over every n, gamma and index set;
critic_loss(discount=) hip / yardstick (margin 2): target 0.86, loss 0.88, td 0.83, dq1 1.00, dq2 0.43; the n-step target through the loss
head 4.37e-08 against a yardstick of 3.80e-08."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nstep_ref as N  # noqa: E402
import replay_shift_ref as RS  # noqa: E402
import replay_u8_ref as R  # noqa: E402
import sac_losses_ref as SR  # noqa: E402

H, W = N.FRAME
P = 64                      # stream positions that have data: the scenario's 52 and what the capture test adds


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


@pytest.fixture(scope="module")
def data():
    """per stream position: the two frames (codes and k / 255 floats) and the small fields that the stream itself does not hold"""
    g = np.random.default_rng(37)
    codes = {"obs": R.pattern(np.arange(P), H, W).reshape(P, H, W), "next_obs": R.pattern(1000 + np.arange(P), H, W).reshape(P, H, W)}
    d = {k: R.dequantize(v) for k, v in codes.items()}
    d.update({k: g.standard_normal((P, 2)).astype(np.float32) for k in ("pobs", "next_pobs", "act")})
    d["codes"] = codes
    return d


@pytest.fixture(scope="module")
def world():
    """the scenario and the reference ring after it, computed once and left unchanged"""
    stream, ops = N.scenario()
    return stream, ops, N.offer(N.Ring(N.SIZE), stream, ops)


def _fields(stream, data, ts):
    ts = np.asarray(ts)
    return dict(obs=data["obs"][ts], next_obs=data["next_obs"][ts], pobs=data["pobs"][ts], next_pobs=data["next_pobs"][ts], act=data["act"][ts],
                rew=np.array([[stream[t][0]] for t in ts], np.float32), done=np.array([[stream[t][1]] for t in ts], np.float32))


def _offer(buf, stream, data, ops, ring=None):
    """the ops on a device buffer; with ``ring`` (a reference ring fed alongside) the flags are compared after every call"""
    for op in ops:
        if op[0] == "episode_end":
            buf.on_episode_end()
        elif op[0] == "add":
            buf.add(**{k: v[0] for k, v in _fields(stream, data, [op[1]]).items()})
        else:
            buf.add_batch(**_fields(stream, data, op[1]))
        if ring is not None:
            N.offer(ring, stream, [op])
            assert buf.episode_flags.dtype == torch.uint8 and tuple(buf.episode_flags.shape) == (buf.size,)
            assert np.array_equal(buf.episode_flags.cpu().numpy(), ring.flags), op
            assert (buf.next_index, buf.stored) == (ring.next_index, ring.stored)


def _buffer(amd, world, data, cls=None, track=True, **kw):
    from dgvit_amd.replay import DeviceReplayBuffer
    stream, ops, _ = world
    buf = (cls or DeviceReplayBuffer)(N.SIZE, obs_shape=(H, W), pstate_dim=N.PSTATE, act_dim=N.ACT, seed=0, **kw)
    if track:
        buf.track_episodes()
    _offer(buf, stream, data, ops if track else [op for op in ops if op[0] != "episode_end"])     # (on_episode_end() would start tracking)
    return buf


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _check(batch, ring, idx, n, gamma, data, frames=True):
    """one n-step batch against the restatement on ``ring`` -> the largest |rew - ref| / tolerance"""
    idx = np.asarray(idx, np.int64)
    B = idx.size
    w = ring.walk(idx, n, gamma)
    start = np.clip(idx, 0, ring.size - 1)
    at, tail = ring.pos[start], ring.pos[w["tail"]]
    assert (tail >= 0).all()
    for k, shape, dtype in (("rew", (B, 1), torch.float32), ("discount", (B, 1), torch.float32), ("done", (B, 1), torch.float32),
                            ("steps", (B,), torch.int32), ("indexes", (B,), torch.int64), ("next_pobs", (B, N.PSTATE), torch.float32),
                            ("obs", (B, H, W), torch.float32), ("next_obs", (B, H, W), torch.float32)):
        assert tuple(batch[k].shape) == shape and batch[k].dtype == dtype, (k, tuple(batch[k].shape), batch[k].dtype)
    got = {k: v.cpu().numpy() for k, v in batch.items()}
    assert np.array_equal(got["steps"], w["steps"]), (n, gamma)
    assert np.array_equal(got["indexes"], idx), "indexes stay the start slots"
    assert np.array_equal(got["done"][:, 0], w["done"])
    for k, where in (("pobs", at), ("act", at), ("next_pobs", tail)) + ((("obs", at), ("next_obs", tail)) if frames else ()):
        assert np.array_equal(got[k], data[k][where]), (k, n, gamma)
    err = np.abs(got["rew"][:, 0].astype(np.float64) - w["ret64"])
    assert (err <= w["tol"]).all(), (n, gamma, float((err / np.maximum(w["tol"], 1e-300)).max()))
    assert (np.abs(got["discount"][:, 0].astype(np.float64) - w["disc64"]) <= 2.0 ** -23 * w["disc64"]).all(), (n, gamma)
    if N.exact(n, gamma):
        assert np.array_equal(got["rew"][:, 0].view(np.uint32), w["rew"].view(np.uint32)), (n, gamma)
        assert np.array_equal(got["discount"][:, 0].view(np.uint32), w["discount"].view(np.uint32)), (n, gamma)
    ok = w["tol"] > 0
    return float((err[ok] / w["tol"][ok]).max()) if ok.any() else 0.0


# ------------------------------------------------------------------------------------------------ 1. the walk
@pytest.fixture(scope="module")
def plain(amd, world, data):
    return _buffer(amd, world, data)


def _index_sets():
    g = np.random.default_rng(67)
    many = g.integers(0, N.SIZE, 67)
    many[[0, 5, 66]] = 14                     # the newest slot at three batch positions, one of them in the workgroup's partial last wave
    many[[1, 64]] = 36
    many[[2, 3, 4]] = [-1, N.SIZE, 1 << 40]   # clamped, as the gathers clamp
    return {"arange": np.arange(N.SIZE), "one": np.array([23]), "many": many}


@pytest.mark.parametrize("which", ["arange", "one", "many"])
def test_walk_equals_the_restatement(amd, world, data, plain, which):
    _, _, ring = world
    idx = _index_sets()[which]
    idx_d = torch.from_numpy(idx).cuda()
    worst = 0.0
    for n in N.NS:
        for gamma in N.GAMMAS:
            a = plain.sample(0, indices=idx_d, n_step=n, gamma=gamma)
            b = plain.sample(0, indices=idx_d, n_step=n, gamma=gamma)
            worst = max(worst, _check(a, ring, idx, n, gamma, data))
            assert list(a) == list(b)
            for k in a:
                assert np.array_equal(_bits(a[k]) if a[k].dtype == torch.float32 else a[k].cpu().numpy(),
                                      _bits(b[k]) if b[k].dtype == torch.float32 else b[k].cpu().numpy()), ("two calls", k, n, gamma)
            start = np.clip(idx, 0, N.SIZE - 1)
            for s in np.unique(start):            # the same start slot anywhere in the batch: the same bits
                rows = np.flatnonzero(start == s)
                for k in ("rew", "discount", "done", "next_pobs", "next_obs"):
                    x = _bits(a[k]).reshape(idx.size, -1)[rows]
                    assert (x == x[0]).all(), (k, s, n, gamma)
    print(f"\n{which}: largest |rew - ref64| / tolerance = {worst:.3f}")


def test_n_step_1_is_the_plain_sample(amd, plain):
    idx = torch.arange(N.SIZE, device="cuda")
    one, ref = plain.sample(0, indices=idx, n_step=1, gamma=0.99), plain.sample(0, indices=idx)
    assert list(ref) == ["obs", "pobs", "act", "rew", "next_obs", "next_pobs", "done", "indexes"], "the plain dict is what it was"
    assert set(one) == set(ref) | {"discount", "steps"}
    for k in ref:
        assert one[k].shape == ref[k].shape and np.array_equal(_bits(one[k]) if k != "indexes" else one[k].cpu().numpy(),
                                                               _bits(ref[k]) if k != "indexes" else ref[k].cpu().numpy()), k
    assert (one["steps"] == 1).all()
    assert np.array_equal(_bits(one["discount"]), np.full((N.SIZE, 1), np.float32(0.99)).view(np.int32))


def test_partially_filled_ring_and_the_newest_slot(amd, data):
    from dgvit_amd.replay import DeviceReplayBuffer
    stream, ops = N.scenario(total=20)
    buf = DeviceReplayBuffer(N.SIZE, obs_shape=(H, W), seed=0)
    ring = N.Ring(N.SIZE)
    buf.track_episodes()
    assert not buf.episode_flags.any()
    _offer(buf, stream, data, ops, ring)
    assert buf.stored == 20 and buf.next_index == 20
    idx = np.arange(20)
    for n in N.NS:
        for gamma in (0.99, 0.5):
            _check(buf.sample(0, indices=torch.from_numpy(idx).cuda(), n_step=n, gamma=gamma), ring, idx, n, gamma, data)
    newest = buf.sample(0, indices=torch.tensor([19], device="cuda"), n_step=64, gamma=0.5)
    assert int(newest["steps"]) == 1 and float(newest["discount"]) == 0.5 and float(newest["rew"]) == float(stream[19][0])
    assert np.array_equal(newest["next_obs"].cpu().numpy()[0], data["next_obs"][19])


# ------------------------------------------------------------------------------------------------ 4., 5. the flags
def test_flags_follow_every_store(amd, world, data):
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    stream, ops, final = world
    for cls in (DeviceReplayBuffer, PrioritizedDeviceReplayBuffer):      # the prioritized store hook does not call the base's
        buf, ring = cls(N.SIZE, obs_shape=(H, W), seed=0), N.Ring(N.SIZE)
        buf.track_episodes()
        buf.track_episodes()
        _offer(buf, stream, data, ops, ring)
        assert np.array_equal(ring.flags, final.flags)
    small = [(r, np.float32(0), False) for r in np.linspace(-1, 1, 40, dtype=np.float32)]
    buf, ring = DeviceReplayBuffer(8, obs_shape=(H, W), seed=0), N.Ring(8, tracked=False)
    with pytest.raises(RuntimeError, match="empty"):
        buf.on_episode_end()
    first = [("add_batch", [0, 1, 2, 3, 4])]
    _offer(buf, small, data, first)                                     # before tracking: nothing is allocated
    N.offer(ring, small, first)
    assert buf.episode_flags is None
    buf.on_episode_end()                                                # starts tracking: HEAD on the newest slot, then END
    ring.episode_end()
    assert buf.episode_flags.cpu().tolist() == ring.flags.tolist() == [0, 0, 0, 0, N.HEAD | N.END, 0, 0, 0]
    _offer(buf, small, data, [("add_batch", [5, 6, 7]),                 # ends exactly at the ring's last slot
                              ("add_batch", list(range(8, 19))),        # more than `size` transitions: the last 8 stay
                              ("episode_end",), ("add", 19), ("add_batch", list(range(20, 28))),    # exactly `size`, from slot 1
                              ("add", 28), ("episode_end",), ("add_batch", [29, 30, 31, 32, 33, 34, 35])], ring)
    assert np.array_equal(buf.store["rew"][:, 0].cpu().numpy(), ring.rew)


def test_a_buffer_that_never_tracked_has_no_flags(amd, world, data):
    buf = _buffer(amd, world, data, track=False)
    assert buf.episode_flags is None
    b = buf.sample(16)
    buf.sample(0, indices=torch.arange(4, device="cuda"), random_shift=2, return_shifts=True)
    assert buf.episode_flags is None and "discount" not in b and "steps" not in b
    late = buf.sample(0, indices=torch.arange(N.SIZE, device="cuda"), n_step=2, gamma=0.5)     # tracking starts here: only the head is known
    want = np.zeros(N.SIZE, np.uint8)
    want[14] = N.HEAD
    assert np.array_equal(buf.episode_flags.cpu().numpy(), want)
    assert int(late["steps"][14]) == 1


# ------------------------------------------------------------------------------------------------ 6. compositions
def test_uint8_ring(amd, world, data):
    _, _, ring = world
    buf = _buffer(amd, world, data, frame_dtype=torch.uint8)
    idx = _index_sets()["many"]
    b = buf.sample(0, indices=torch.from_numpy(idx).cuda(), n_step=3, gamma=0.99)
    _check(b, ring, idx, 3, 0.99, data)
    tail = ring.pos[ring.walk(idx, 3, 0.99)["tail"]]
    want = torch.from_numpy(data["codes"]["next_obs"][tail]).float() / 255
    assert torch.equal(b["next_obs"].cpu(), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["fp32", "uint8"])
def test_random_shift(amd, world, data, dtype):
    _, _, ring = world
    buf = _buffer(amd, world, data, frame_dtype=dtype)
    idx = _index_sets()["many"]
    B, pad = idx.size, 2
    b = buf.sample(0, indices=torch.from_numpy(idx).cuda(), n_step=5, gamma=0.5, random_shift=pad, return_shifts=True)
    _check(b, ring, idx, 5, 0.5, data, frames=False)
    w = ring.walk(idx, 5, 0.5)
    for k, where, stream_id in (("obs", ring.pos[np.clip(idx, 0, N.SIZE - 1)], 0), ("next_obs", ring.pos[w["tail"]], 1)):
        np.testing.assert_array_equal(b[k + "_shift"].cpu().numpy(), RS.draw_shifts(B, pad, buf.shift_seed, stream_id))
        assert torch.equal(b[k].cpu(), RS.ref_shift(torch.from_numpy(data[k][where]), b[k + "_shift"].cpu(), pad)), k
    assert int(b["next_obs_shift"].abs().max()) > 0


def test_prioritized_buffer(amd, world, data):
    from dgvit_amd.replay import PrioritizedDeviceReplayBuffer
    _, _, ring = world
    buf = _buffer(amd, world, data, cls=PrioritizedDeviceReplayBuffer, alpha=1.0, eps=0.0)
    every = torch.arange(N.SIZE, device="cuda")
    prio = torch.from_numpy(1.0 + np.arange(N.SIZE, dtype=np.float32) % 5).cuda()
    buf.update_priorities(every, prio)
    B = 67
    u = torch.rand(B, device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    one, many = buf.sample(B, beta=0.7, uniforms=u), buf.sample(B, beta=0.7, uniforms=u, n_step=3, gamma=0.99)
    assert torch.equal(one["indexes"], many["indexes"]) and torch.equal(one["weights"], many["weights"])
    assert one["weights"].min() < 1, "the weights are not trivial"
    idx = many["indexes"].cpu().numpy()
    assert len(np.unique(idx)) > 20
    _check(many, ring, idx, 3, 0.99, data)
    buf.update_priorities(many["indexes"], torch.full((B,), 9.0, device="cuda"))
    want = prio.cpu().numpy().copy()
    want[idx] = 9.0                               # the start slots, not the tails
    np.testing.assert_array_equal(buf.priorities().cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 7. capture
def test_a_captured_sample_follows_the_ring(amd, world, data):
    from dgvit_amd.replay import DeviceReplayBuffer
    stream, ops, final = world
    buf = _buffer(amd, world, data)
    ring = N.offer(N.Ring(N.SIZE), stream, ops)
    assert np.array_equal(ring.flags, final.flags)
    untracked = DeviceReplayBuffer(N.SIZE, obs_shape=(H, W), seed=0)
    idx = np.array([13, 14, 15, 16, 17, 18, 19, 0, 36, 30, 12])        # the head is slot 14; five adds take it to 19
    idx_d = torch.from_numpy(idx).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            buf.sample(0, indices=idx_d, n_step=3, gamma=0.99)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = buf.sample(0, indices=idx_d, n_step=3, gamma=0.99)
        with pytest.raises(amd.DgvitError, match="capture"):
            untracked.track_episodes()
        with pytest.raises(amd.DgvitError, match="capture"):
            untracked.sample(0, indices=idx_d, n_step=3)
    assert untracked.episode_flags is None
    graph.replay()
    torch.cuda.synchronize()
    eager = buf.sample(0, indices=idx_d, n_step=3, gamma=0.99)
    for k in eager:
        assert torch.equal(static[k], eager[k]), k
    _check(static, ring, idx, 3, 0.99, data)
    more = list(stream) + [(np.float32(0.25), np.float32(0), False), (np.float32(-0.5), np.float32(0), True), (np.float32(1), np.float32(0), False),
                           (np.float32(-1), np.float32(1), False), (np.float32(0.125), np.float32(0), False)]
    late = [("add", 52), ("add", 53), ("episode_end",), ("add_batch", [54, 55, 56])]
    _offer(buf, more, data, late, ring)
    assert buf.next_index == 20
    now = ring.walk(idx, 3, 0.99)
    graph.replay()
    torch.cuda.synchronize()
    _check(static, ring, idx, 3, 0.99, data)
    assert not np.array_equal(now["steps"], final.walk(idx, 3, 0.99)["steps"]), "the ring has moved on, and the walks with it"


# ------------------------------------------------------------------------------------------------ 8. a big ring
def test_walks_that_wrap_a_big_ring(amd):
    """100 003 slots filled by one add_batch that starts at slot 70, so the head is slot 69 and a 64-step walk from any of the last 63
    slots wraps past slot 0: the slot arithmetic next to nrows, with rewards that tell the slots apart"""
    from dgvit_amd.replay import DeviceReplayBuffer
    S = 100003
    g = np.random.default_rng(100003)
    rew = (g.integers(-256, 257, S) / 256.0).astype(np.float32)
    done = np.zeros(S, np.float32)
    done[[10, 40000]] = 1
    npobs = g.standard_normal((S, 2)).astype(np.float32)
    codes = g.integers(0, 256, (S, 2, 2), dtype=np.uint8)
    buf = DeviceReplayBuffer(S, obs_shape=(2, 2), seed=0)
    ring = N.Ring(S)
    buf.track_episodes()
    buf.next_index = ring.next_index = 70
    frames = R.dequantize(codes)
    buf.add_batch(obs=frames, next_obs=frames, pobs=npobs, next_pobs=npobs, act=npobs, rew=rew[:, None], done=done[:, None])
    ring.store(rew, done, np.arange(S))
    assert np.array_equal(buf.episode_flags.cpu().numpy(), ring.flags) and ring.flags[69] == N.HEAD and ring.flags.sum() == N.HEAD
    idx = np.concatenate([S - 64 + np.arange(64), [69, 68, 7, 75, 40065]])      # stream positions 10 and 40000 sit in slots 80 and 40070
    for n, gamma in ((64, 0.99), (64, 1.0), (5, 0.5)):
        b = buf.sample(0, indices=torch.from_numpy(idx).cuda(), n_step=n, gamma=gamma)
        w = ring.walk(idx, n, gamma)
        got = {k: v.cpu().numpy() for k, v in b.items()}
        assert np.array_equal(got["steps"], w["steps"])
        if n == 64:
            assert (w["steps"][:64] == 64).all() and w["steps"][64:].tolist() == [1, 2, 63, 6, 6], "full walks; head, head, head, done, done"
            assert (w["tail"][1:64] < 64).all()
        err = np.abs(got["rew"][:, 0].astype(np.float64) - w["ret64"])
        assert (err <= w["tol"]).all(), (n, gamma, float((err / np.maximum(w["tol"], 1e-300)).max()))
        assert (np.abs(got["discount"][:, 0].astype(np.float64) - w["disc64"]) <= 2.0 ** -23 * w["disc64"]).all()
        if N.exact(n, gamma):
            assert np.array_equal(got["rew"][:, 0].view(np.uint32), w["rew"].view(np.uint32))
        tail = ring.pos[w["tail"]]
        assert np.array_equal(got["done"][:, 0], w["done"]) and np.array_equal(got["next_pobs"], npobs[tail])
        assert np.array_equal(got["next_obs"], frames[tail]) and np.array_equal(got["obs"], frames[ring.pos[idx]])


# ------------------------------------------------------------------------------------------------ 9. critic_loss(discount=)
ALPHA, GAMMA = 0.2, 0.99
CRITIC_SHAPES = [(1, 1), (5, 2), (67, 2)]
CRITIC_OUT = ("target", "loss", "td", "dq1", "dq2")


def _critic_inputs(Bn, A):
    g = torch.Generator().manual_seed(977 * Bn + A)
    n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
    m = torch.randint(1, 6, (Bn, 1), generator=g)
    return dict(q1=n(Bn, A), q2=n(Bn, A), reward=n(Bn, 1), q1n=n(Bn, A), q2n=n(Bn, A), nlp=n(Bn, 1), done=(torch.rand(Bn, 1, generator=g) < 0.25).float(),
                w=1 - torch.rand(Bn, 1, generator=g), discount=(torch.tensor(GAMMA, dtype=torch.float64) ** m).float())


def _critic_ref(x, dtype, use_done, use_w):
    x = {k: v.to(dtype) for k, v in x.items()}
    q1, q2 = x["q1"].clone().requires_grad_(True), x["q2"].clone().requires_grad_(True)
    y = SR.target(x["reward"], x["q1n"], x["q2n"], x["nlp"], ALPHA, x["discount"], x["done"] if use_done else None)
    loss = SR.critic_loss(q1, q2, y, x["w"] if use_w else None)
    loss.backward()
    return {k: v.detach().double() for k, v in dict(target=y, loss=loss, td=SR.td(q1.detach(), y), dq1=q1.grad, dq2=q2.grad).items()}


def _critic_dev(amd, x, use_done, use_w, **kw):
    x = {k: v.cuda() for k, v in x.items()}
    q1, q2 = x["q1"].requires_grad_(True), x["q2"].requires_grad_(True)
    c = amd.sac_losses.critic_loss(q1, q2, x["reward"], x["q1n"], x["q2n"], x["nlp"], alpha=ALPHA, done=x["done"] if use_done else None,
                                   weights=x["w"] if use_w else None, **kw)
    c.loss.backward()
    return dict(target=c.target, loss=c.loss, td=c.td, dq1=q1.grad, dq2=q2.grad)


def _rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


def test_critic_loss_with_a_per_sample_discount(amd):
    """test_gpu_sac_losses.py's rule for gamma=: per output, max |hip - ref64| / max |ref64|, the largest over the cases, against 2 x the same
    quantity of the restatement's own fp32 evaluation; where that evaluation is exact, within 2^-23"""
    hip, yard, exact = {k: 0.0 for k in CRITIC_OUT}, {k: 0.0 for k in CRITIC_OUT}, []
    for Bn, A in CRITIC_SHAPES:
        x = _critic_inputs(Bn, A)
        for use_done in (False, True):
            for use_w in (False, True):
                r64, r32 = (_critic_ref(x, dt, use_done, use_w) for dt in (torch.float64, torch.float32))
                for disc in (x["discount"], x["discount"].reshape(-1)):            # (B, 1) and (B,)
                    dev = {k: v.detach().double().cpu() for k, v in _critic_dev(amd, x, use_done, use_w, discount=disc.cuda(), gamma=None).items()}
                    for k in CRITIC_OUT:
                        assert dev[k].shape == r64[k].shape, k
                        h, y = _rel(dev[k], r64[k]), _rel(r32[k], r64[k])
                        hip[k], yard[k] = max(hip[k], h), max(yard[k], y)
                        if y == 0.0:
                            exact.append((k, Bn, A, h))
    print("\ncritic_loss(discount=): output  hip  yardstick  hip/yardstick")
    for k in CRITIC_OUT:
        print(f"  {k:8s} {hip[k]:.3e}  {yard[k]:.3e}  {hip[k] / yard[k] if yard[k] > 0 else float('inf'):.2f}")
    for k, Bn, A, h in exact:
        assert h <= 2.0 ** -23, (k, Bn, A, h)
    for k in CRITIC_OUT:
        assert yard[k] > 0, k
        assert hip[k] <= 2.0 * yard[k], (k, hip[k], yard[k])


@pytest.mark.parametrize("Bn, A", CRITIC_SHAPES)
def test_a_constant_discount_is_the_gamma_call_bit_for_bit(amd, Bn, A):
    x = _critic_inputs(Bn, A)
    for use_done in (False, True):
        for use_w in (False, True):
            a = _critic_dev(amd, x, use_done, use_w, gamma=GAMMA)
            b = _critic_dev(amd, x, use_done, use_w, discount=torch.full((Bn,), GAMMA, device="cuda"))
            for k in CRITIC_OUT:
                assert np.array_equal(_bits(a[k]), _bits(b[k])), (k, use_done, use_w)


def test_n_step_batch_through_the_critic_loss(amd, world, data, plain):
    """ring -> sample(n_step=3) -> critic_loss(discount=): the target against the float64 n-step target built from the restatement's
    unrounded return and gamma^m, under the same rule with the fp32 evaluation of the fp32 batch as the yardstick"""
    _, _, ring = world
    idx = np.arange(N.SIZE)
    batch = plain.sample(0, indices=torch.from_numpy(idx).cuda(), n_step=3, gamma=GAMMA)
    w = ring.walk(idx, 3, GAMMA)
    x = _critic_inputs(N.SIZE, 2)
    c = amd.sac_losses.critic_loss(x["q1"].cuda(), x["q2"].cuda(), batch["rew"], x["q1n"].cuda(), x["q2n"].cuda(), x["nlp"].cuda(), alpha=ALPHA,
                                   done=batch["done"], discount=batch["discount"])
    col = lambda a, dt: torch.from_numpy(np.asarray(a)).to(dt).reshape(-1, 1)  # noqa: E731
    y64 = SR.target(col(w["ret64"], torch.float64), x["q1n"].double(), x["q2n"].double(), x["nlp"].double(), ALPHA, col(w["disc64"], torch.float64),
                    col(w["done"], torch.float64))
    y32 = SR.target(col(w["rew"], torch.float32), x["q1n"], x["q2n"], x["nlp"], ALPHA, col(w["discount"], torch.float32), col(w["done"], torch.float32))
    h, y = _rel(c.target.double().cpu(), y64), _rel(y32.double(), y64)
    print(f"\nn-step target: hip {h:.3e}  yardstick {y:.3e}")
    assert y > 0 and h <= 2.0 * y, (h, y)
    assert (w["steps"] < 3).any() and (w["done"] == 1).any(), "walks of every kind are in the batch"
