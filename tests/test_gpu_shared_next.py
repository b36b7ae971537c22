"""GPU: the replay ring that stores each frame once -- DeviceReplayBuffer(shared_next_obs=True) through
dgvit_ring_plan_next, dgvit_ring_store_frames_shared and dgvit_ring_next_rows.

The two-matrix ring is the reference: twin buffers get the same seed and the same calls, one of them ``shared_next_obs=True``, and every
``sample`` of all written slots must be bit-equal in every field -- plain, with n_step in {1, 3, 64}, and with random_shift=2 after the
same torch.manual_seed, shift tables included.  The stream honours the contract (tests/shared_next_ref.py: inside an episode the obs of
step t + 1 is the next_obs of step t, a new episode starts with a new frame); frames are 6 x 10 and 5 x 7 (35 pixels: the row padding of
both formats).  The twins' pool is the default one, every other slot of every lane, which these streams never fill.  The overflow
itself is compared with the numpy restatement: ``lost_terminal_frames()``, the ``next_row`` table, and lost slots returning their own obs."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nstep_ref as N  # noqa: E402
import shared_next_ref as S  # noqa: E402
import vec_replay_ref as V  # noqa: E402

FIELDS = ("obs", "pobs", "act", "rew", "next_obs", "next_pobs", "done")
FRAMES = ("obs", "next_obs")
SCENARIOS = [(3, 36, 20), (1, 37, 52), (4, 8, 7), (4, 4, 6)]
SHAPES = [(6, 10), (5, 7)]
DTYPES = [torch.float32, torch.uint8]


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


def _classes():
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    return {"base": DeviceReplayBuffer, "per": PrioritizedDeviceReplayBuffer}


def _data(strs, frs, shape):
    """data[k][t, e]: field k of environment e's transition t; frames from their ids, as codes and as the exact floats code / 255"""
    T, E = len(strs[0]), len(strs)
    g = np.random.default_rng(100 * E + T)
    d = {"codes": {}}
    for j, k in enumerate(FRAMES):
        d["codes"][k] = np.stack([np.stack([S.pixels(frs[e][t][j], shape, codes=True) for e in range(E)]) for t in range(T)])
        d[k] = d["codes"][k].astype(np.float32) / np.float32(255.0)
    d.update({k: g.standard_normal((T, E, 2)).astype(np.float32) for k in ("pobs", "next_pobs", "act")})
    d["rew"] = np.array([[[s[t][0]] for s in strs] for t in range(T)], np.float32)
    d["done"] = np.array([[[s[t][1]] for s in strs] for t in range(T)], np.float32)
    d["end"] = np.array([[s[t][2] for s in strs] for t in range(T)], bool)
    return d


@functools.lru_cache(maxsize=None)
def _world(E, T, shape):
    """(streams, frame ids, data), computed once per shape and left unchanged"""
    strs = V.streams(E, T)
    frs = S.all_frames(strs)
    return strs, frs, _data(strs, frs, shape)


@functools.lru_cache(maxsize=None)
def _ops_world(shape):
    """nstep_ref.scenario(): one environment, add / add_batch / on_episode_end"""
    stream, ops = N.scenario()
    frs = S.frames(stream)
    return stream, ops, frs, _data([stream], [frs], shape)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _twins(cls, E, size, shape, dtype, P=None):
    kw = dict(obs_shape=shape, pstate_dim=V.PSTATE, act_dim=V.ACT, seed=3, frame_dtype=dtype, num_envs=E)
    return cls(size, **kw), cls(size, shared_next_obs=True, terminal_frames=P, **kw)


def _fields(d, ts, mode, u8, squeeze):
    """the keywords of one call for the stream positions ts (a step: ts = t and the first axis is E; add: squeeze)"""
    f = {k: (d[k][ts, 0] if squeeze else d[k][ts]) for k in FIELDS}
    c = {k: (d["codes"][k][ts, 0] if squeeze else d["codes"][k][ts]) for k in FRAMES}
    if mode == "device":
        return {k: _dev(v) for k, v in f.items()}
    if mode == "codes" and u8:            # the ring's own codes: obs on the device, next_obs from the host
        return {**f, "obs": _dev(c["obs"]), "next_obs": c["next_obs"]}
    if mode == "mixed":
        return {**f, "next_obs": _dev(f["next_obs"]), "done": _dev(f["done"])}
    return dict(f)


MODES = ("host", "device", "codes", "mixed")


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (k, what)
        if x.dtype == torch.float32:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), (k, what)


def _compare(two, shared, what):
    """sample(indices=all written slots) of the twins, bit-equal in every field: plain, n-step, shifted"""
    assert (two.next_index, two.stored) == (shared.next_index, shared.stored)
    idx = torch.arange(two.stored, device="cuda")
    calls = [dict(), dict(n_step=1), dict(n_step=3, gamma=0.5), dict(n_step=64), dict(random_shift=2, return_shifts=True),
             dict(random_shift=2, return_shifts=True, n_step=3)]
    for kw in calls:
        out = []
        for buf in (two, shared):            # a prioritized sample draws its own indices: the base class's gathers at idx for both classes
            torch.manual_seed(11)
            out.append(_classes()["base"].sample(buf, idx.numel(), indices=idx, **kw))
        _same(out[0], out[1], (what, kw))
        if "random_shift" in kw and idx.numel() >= 16:
            assert out[1]["next_obs_shift"].abs().max() > 0 and not torch.equal(out[1]["obs_shift"], out[1]["next_obs_shift"])
    assert torch.equal(two.episode_flags, shared.episode_flags)


# ------------------------------------------------------------------------------------------------ 1. the twins
@pytest.mark.parametrize("cls", ["base", "per"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("E, size, steps", SCENARIOS)
def test_add_vec_twins_sample_the_same_bits(amd, E, size, steps, shape, dtype, cls):
    """through the wrap, with ends on the newest step, ends given with the step (even t) and by on_episode_end afterwards (odd t)"""
    strs, frs, d = _world(E, steps, shape)
    two, shared = _twins(_classes()[cls], E, size, shape, dtype)
    two.track_episodes()
    u8 = dtype is torch.uint8
    assert shared.episode_flags is not None, "the constructor starts track_episodes()"
    for t in range(steps):
        for buf in (two, shared):
            kw = _fields(d, t, MODES[t % 4], u8, False)
            if t % 2 == 0:
                buf.add_vec(**kw, episode_end=_dev(d["end"][t]) if t % 4 == 0 else d["end"][t])
            else:
                buf.add_vec(**kw)
                if E > 1:
                    buf.on_episode_end(envs=_dev(d["end"][t]))
                elif d["end"][t][0]:
                    buf.on_episode_end()
        if t % 3 == 2 or t == steps - 1 or d["end"][t].any() or (d["done"][t] != 0).any():
            _compare(two, shared, (t, MODES[t % 4]))
    assert shared.lost_terminal_frames() == 0 and two.lost_terminal_frames() == 0


@pytest.mark.parametrize("cls", ["base", "per"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_add_and_add_batch_twins_sample_the_same_bits(amd, shape, dtype, cls):
    """nstep_ref.scenario(): add, add_batch runs (with a done inside a run where an episode ends by done) and on_episode_end() after
    the store, through the wrap of a 37-slot ring"""
    stream, ops, frs, d = _ops_world(shape)
    two, shared = _twins(_classes()[cls], 1, N.SIZE, shape, dtype)
    two.track_episodes()
    u8 = dtype is torch.uint8
    for j, op in enumerate(ops):
        for buf in (two, shared):
            if op[0] == "episode_end":
                buf.on_episode_end()
            elif op[0] == "add":
                buf.add(**_fields(d, op[1], MODES[j % 4], u8, True))
            else:
                buf.add_batch(**_fields(d, op[1], MODES[j % 4], u8, True))
        if op[0] == "episode_end" or j % 4 == 3 or j == len(ops) - 1:
            _compare(two, shared, (j, op))
    assert shared.lost_terminal_frames() == 0
    ref = S.SharedRing(1, N.SIZE)
    for op in ops:
        ref.episode_end(np.array([True])) if op[0] == "episode_end" else ref.store(stream, frs, [op[1]] if op[0] == "add" else op[1])
    assert np.array_equal(shared.next_row.cpu().numpy(), ref.next_row) and shared._pool_state.tolist() == ref.state()


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
def test_an_add_batch_of_thousands_of_rows_equals_the_restatement(amd, dtype):
    """4100 rows (65 rounds of the bookkeeping's wave, the last one partial) with ends by done, into a ring of 5000 and again across its
    end; then a run that covers the whole ring"""
    size, shape, P = 5000, (5, 7), 300
    g = np.random.default_rng(7)
    T = 4100 + 4100 + size
    stream = [(np.float32(0), np.float32(g.random() < 0.05), False) for _ in range(T)]
    frs = S.frames(stream)
    d = _data([stream], [frs], shape)
    from dgvit_amd.replay import DeviceReplayBuffer
    two, shared = _twins(DeviceReplayBuffer, 1, size, shape, dtype, P=P)
    ref = S.SharedRing(1, size, P)
    for lo, hi in ((0, 4100), (4100, 8200), (8200, T)):
        for buf in (two, shared):
            buf.add_batch(**_fields(d, np.arange(lo, hi), "device", False, True))
        ref.store(stream, frs, range(lo, hi))
        assert np.array_equal(shared.next_row.cpu().numpy(), ref.next_row), (lo, hi)
        assert shared._pool_state.tolist() == ref.state() and ref.lost == 0 and ref.tail > 0
        idx = torch.arange(two.stored, device="cuda")
        _same(two.sample(idx.numel(), indices=idx), shared.sample(idx.numel(), indices=idx), (lo, hi))


# ------------------------------------------------------------------------------------------------ 2. prioritized draws
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
def test_prioritized_twins_draw_equal_batches_and_keep_equal_trees(amd, dtype):
    E, size, steps = SCENARIOS[0]
    strs, frs, d = _world(E, steps, (5, 7))
    two, shared = _twins(_classes()["per"], E, size, (5, 7), dtype)
    B = 64
    g = torch.Generator(device="cuda").manual_seed(5)
    for t in range(steps):
        for buf in (two, shared):
            buf.add_vec(**_fields(d, t, "device", False, False), episode_end=_dev(d["end"][t]))
        if t % 4 == 3:
            u = torch.rand(B, device="cuda", generator=g)
            a, b = (buf.sample(B, 0.7, uniforms=u, n_step=3 if t % 8 == 7 else None) for buf in (two, shared))
            _same(a, b, t)
            prio = torch.rand(B, device="cuda", generator=g)
            for buf, batch in ((two, a), (shared, b)):
                buf.update_priorities(batch["indexes"], prio)
            assert torch.equal(two.tree, shared.tree), t
    assert torch.equal(two.tree, shared.tree)


# ------------------------------------------------------------------------------------------------ 3. the overflow
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
@pytest.mark.parametrize("E, size, steps, P", [(3, 36, 20, 2), (1, 37, 52, 2)])
def test_a_full_pool_loses_what_the_restatement_loses(amd, E, size, steps, P, dtype):
    strs, frs, d = _world(E, steps, (6, 10))
    from dgvit_amd.replay import DeviceReplayBuffer
    two, shared = _twins(DeviceReplayBuffer, E, size, (6, 10), dtype, P=P)
    ref = S.SharedRing(E, size, P)
    for t in range(steps):
        for buf in (two, shared):
            buf.add_vec(**_fields(d, t, MODES[t % 4], dtype is torch.uint8, False), episode_end=d["end"][t])
        ref.add_vec_frames(strs, frs, t)
        assert np.array_equal(shared.next_row.cpu().numpy(), ref.next_row), t
    assert ref.lost > 0 and ref.tail > 0
    assert shared.lost_terminal_frames() == ref.lost and shared._pool_state.tolist() == ref.state()
    idx = torch.arange(size, device="cuda")
    a, b = two.sample(size, indices=idx), shared.sample(size, indices=idx)
    lost = torch.from_numpy(ref.next_row == np.arange(size)).cuda()
    assert 0 < int(lost.sum()) <= ref.lost
    assert torch.equal(b["next_obs"][lost], b["obs"][lost]), "a lost slot returns its own obs"
    assert not torch.equal(a["next_obs"][lost], b["next_obs"][lost])
    assert torch.equal(a["next_obs"][~lost], b["next_obs"][~lost]), "every other slot is still right"
    for k in FIELDS:
        if k != "next_obs":
            assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ 4. what is allocated
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
def test_the_arena_is_the_only_frame_storage(amd, dtype):
    from dgvit_amd.replay import DeviceReplayBuffer
    for E, size, P in ((3, 36, None), (1, 37, None), (4, 8, 5), (16, 1600, None)):
        buf = DeviceReplayBuffer(size, obs_shape=(5, 7), num_envs=E, frame_dtype=dtype, shared_next_obs=True, terminal_frames=P)
        want = S.default_pool(size, E) if P is None else P
        row = 48 if dtype is torch.uint8 else 36
        assert buf.terminal_frames == want and buf.arena_rows == size + E + want
        assert tuple(buf.arena.shape) == (size + E + want, row) and buf.arena.dtype == dtype
        assert "next_obs" not in buf.store and set(buf.store) == set(FIELDS) - {"next_obs"}
        assert buf.store["obs"].data_ptr() == buf.arena.data_ptr() and tuple(buf.store["obs"].shape) == (size, row)
        assert set(buf.fields) == set(buf.shapes) == set(buf.rows) == set(FIELDS)
        assert buf.next_row.dtype == torch.int32 and (buf.next_row == -1).all() and buf._pool_state.tolist() == [0, 0, 0]
        assert buf.episode_flags is not None and buf.lost_terminal_frames() == 0
    assert DeviceReplayBuffer(1600, obs_shape=(5, 7), num_envs=16, shared_next_obs=True).terminal_frames == 800


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
def test_a_buffer_without_the_keyword_is_what_it_was(amd, dtype):
    strs, frs, d = _world(3, 20, (5, 7))
    for cls in _classes().values():
        buf = cls(36, obs_shape=(5, 7), num_envs=3, frame_dtype=dtype, seed=3)
        row = 48 if dtype is torch.uint8 else 36
        assert list(buf.store) == list(FIELDS) and buf.arena is None and buf.arena_rows is None and buf.terminal_frames is None
        assert not buf.shared_next_obs and buf.episode_flags is None and not hasattr(buf, "next_row")
        for k in FRAMES:
            assert tuple(buf.store[k].shape) == (36, row) and buf.store[k].dtype == dtype
        assert buf.store["obs"].data_ptr() != buf.store["next_obs"].data_ptr()
        for t in range(5):
            buf.add_vec(**_fields(d, t, "device", False, False))
        out = _classes()["base"].sample(buf, 15, indices=torch.arange(15, device="cuda"))
        for k in FIELDS:
            assert np.array_equal(out[k].cpu().numpy().reshape(5, 3, -1), d[k][:5].reshape(5, 3, -1)), k
        assert buf.episode_flags is None, "nothing started tracking"


class Synchronised(RuntimeError):
    pass


def _raiser(name):
    def fn(*a, **k):
        raise Synchronised(name)
    return fn


def test_an_all_device_store_on_a_shared_ring_never_synchronises_or_pins(amd, monkeypatch):
    """add_vec, add and add_batch with every field and the ends on the device: no host read, no synchronize, no pinned staging matrix
    -- under a guard on the tensor methods and, where this build's detector works (it raises on .item()), under torch's own"""
    strs, frs, d = _world(3, 20, (5, 7))
    vec = [_twins(cls, 3, 36, (5, 7), dtype)[1] for cls in _classes().values() for dtype in DTYPES]
    one = [_twins(cls, 1, 36, (5, 7), dtype)[1] for cls in _classes().values() for dtype in DTYPES]
    steps = [(_fields(d, t, "device", False, False), _dev(d["end"][t] | (t == 1))) for t in range(3)]
    single = {k: v[0] for k, v in steps[0][0].items()}
    torch.cuda.synchronize()

    def run():
        for buf in vec:
            for kw, mask in steps:
                buf.add_vec(**kw, episode_end=mask)
                buf.on_episode_end(envs=mask)
        for buf in one:
            buf.add(**single)
            buf.on_episode_end()
            buf.add_batch(**steps[1][0])

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy", "pin_memory"):
            m.setattr(torch.Tensor, name, _raiser(name))
        m.setattr(torch.cuda, "synchronize", _raiser("torch.cuda.synchronize"))
        m.setattr(torch.cuda.Stream, "synchronize", _raiser("Stream.synchronize"))
        with pytest.raises(Synchronised):
            torch.ones(1, device="cuda").item()           # the guard does raise
        run()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device="cuda").item()
            detects = False
        except RuntimeError:
            detects = True
        if detects:
            run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for buf in vec:
        assert buf.stored == (18 if detects else 9) and not hasattr(buf, "_last_stage"), "nothing was staged"
        assert (buf.next_row[:buf.stored] >= 0).all()
    for buf in one:
        assert buf.stored == (8 if detects else 4) and not hasattr(buf, "_last_stage")


# ------------------------------------------------------------------------------------------------ 5. a captured sample follows the ring
def test_a_captured_nstep_sample_follows_the_shared_ring(amd):
    E, size, steps = SCENARIOS[0]
    strs, frs, d = _world(E, steps, (5, 7))
    from dgvit_amd.replay import DeviceReplayBuffer
    two, shared = _twins(DeviceReplayBuffer, E, size, (5, 7), torch.uint8)
    two.track_episodes()
    first = 14                                   # 42 slots offered: the ring has wrapped
    for t in range(first):
        for buf in (two, shared):
            buf.add_vec(**_fields(d, t, "device", False, False), episode_end=_dev(d["end"][t]))
    idx = torch.arange(size, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            shared.sample(size, n_step=3, gamma=0.99, indices=idx)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = shared.sample(size, n_step=3, gamma=0.99, indices=idx)
    graph.replay()
    torch.cuda.synchronize()
    _same(static, shared.sample(size, n_step=3, gamma=0.99, indices=idx), "replayed at once")
    before = {k: v.clone() for k, v in static.items()}
    for t in range(first, steps):
        for buf in (two, shared):
            buf.add_vec(**_fields(d, t, "device", False, False), episode_end=_dev(d["end"][t]))
    graph.replay()
    torch.cuda.synchronize()
    _same(static, shared.sample(size, n_step=3, gamma=0.99, indices=idx), "replayed after six more steps")
    _same(static, two.sample(size, n_step=3, gamma=0.99, indices=idx), "and equal to the two-matrix ring")
    assert not torch.equal(before["next_obs"], static["next_obs"]), "the ring has moved on"
