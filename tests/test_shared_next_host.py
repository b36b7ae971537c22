"""CPU (no GPU): the replay ring that stores each frame once -- the ``shared_next_obs`` / ``terminal_frames`` checks, the
entry points dgvit_ring_plan_next, dgvit_ring_store_frames_shared and dgvit_ring_next_rows with their argument checks, and the numpy
restatement tests/shared_next_ref.py against the truth computed from each environment's stream alone.  Every library call here fails its
argument check before any launch: the pointers are never dereferenced."""
import ctypes
import os

import numpy as np
import pytest

import nstep_ref as N
import shared_next_ref as S
import vec_replay_ref as V

FAKE = ctypes.c_void_p(0x1000)   # non-null, 16-byte aligned, never read: only argument checks run
OFF8 = ctypes.c_void_p(0x1008)
OFF4 = ctypes.c_void_p(0x1004)
OFF2 = ctypes.c_void_p(0x1002)

NAMES = ("dgvit_ring_plan_next", "dgvit_ring_store_frames_shared", "dgvit_ring_next_rows")
SCENARIOS = [(3, 36, 20), (1, 37, 52), (4, 8, 7), (4, 4, 6)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


# ------------------------------------------------------------------------------------------------ the Python checks
@pytest.mark.parametrize("kw", [dict(shared_next_obs=1), dict(shared_next_obs="yes"), dict(shared_next_obs=None),
                                dict(shared_next_obs=True, terminal_frames=0), dict(shared_next_obs=True, terminal_frames=-1),
                                dict(shared_next_obs=True, terminal_frames=37), dict(shared_next_obs=True, terminal_frames=True),
                                dict(shared_next_obs=True, terminal_frames=2.0), dict(terminal_frames=4),
                                dict(shared_next_obs=False, terminal_frames=4)], ids=str)
def test_bad_keywords_raise_before_any_device_is_touched(kw):
    """size = 36.  No GPU is needed to get here (without the keywords this is a TypeError)"""
    from dgvit_amd import replay
    word = "terminal_frames" if "terminal_frames" in kw else "shared_next_obs"
    for cls in (replay.DeviceReplayBuffer, replay.PrioritizedDeviceReplayBuffer):
        with pytest.raises(ValueError, match=word):
            cls(36, obs_shape=(6, 10), num_envs=3, **kw)


def test_good_keywords_pass_the_helper_and_the_default_pool():
    from dgvit_amd import replay
    assert replay._shared_next(False, None, 36, 3) == (False, None)
    assert replay._shared_next(True, None, 36, 3) == (True, 18) and replay._shared_next(True, None, 100000, 16) == (True, 50000)
    assert replay._shared_next(True, None, 4, 4) == (True, 4) and replay._shared_next(True, None, 37, 1) == (True, 19)
    assert replay._shared_next(True, np.int64(36), 36, 3) == (True, 36) and replay._shared_next(np.bool_(True), 1, 36, 3) == (True, 1)
    for size, E in ((36, 3), (37, 1), (8, 4), (4, 4), (100000, 16)):
        assert S.default_pool(size, E) == replay._shared_next(True, None, size, E)[1]


def test_num_envs_is_still_checked_before_anything_a_bare_object_lacks():
    import dgvit_amd
    from dgvit_amd import replay
    buf = object.__new__(replay.DeviceReplayBuffer)
    buf.num_envs = 3
    z = np.zeros((3, 2), np.float32)
    with pytest.raises(dgvit_amd.DgvitError, match="add_vec"):
        buf.add(obs=z, pobs=z, act=z, rew=z, next_obs=z, next_pobs=z, done=z)


# ------------------------------------------------------------------------------------------------ the entry points
def test_symbols_are_exported_bound_and_declared(lib):
    from dgvit_amd import _lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    with open(os.path.join(os.path.dirname(L.LIB_PATH), os.pardir, "include", "dgvit_hip.h")) as f:
        header = f.read()
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    for name in NAMES:
        assert hasattr(raw, name)
        assert "int " + name + "(" in header
    assert L.SIGNATURES["dgvit_ring_plan_next"] == (I, [P, P, P, P, LL, P, LL, LL, LL, LL, LL, P])
    assert L.SIGNATURES["dgvit_ring_store_frames_shared"] == (I, [P, I, LL, P, I, LL, P, P, I, LL, LL, LL, LL, LL, LL, LL, P])
    assert L.SIGNATURES["dgvit_ring_next_rows"] == (I, [P, P, P, LL, LL, P])
    assert L.SIGNATURES["dgvit_ring_store_frames"] == (I, [P, I, LL, P, I, LL, P, P, I, LL, LL, LL, LL, LL, P]), "no existing signature changes"
    from dgvit_amd import replay
    assert replay.FRAME_FIELDS == ("obs", "next_obs") and len(replay.SMALL_FIELDS) == 5


def test_abi_version_is_unchanged(lib):
    from dgvit_amd import _lib as L
    assert lib.dgvit_abi_version() == 7 and L.ABI_VERSION == 7


def _ids(v):
    return None if isinstance(v, bytes) else "-".join(f"{k}={x if not isinstance(x, ctypes.c_void_p) else x.value}" for k, x in v.items())


def _msg(lib, rc, name, word):
    assert rc == -1, "DGVIT_ERR_ARG"
    msg = lib.dgvit_last_error()
    assert name in msg and word in msg, msg


SHARED = [                                        # check_shared: the slots, the lanes and the pool, asked by both store entry points
    (dict(n=0), b"n=0"),
    (dict(n=-3), b"n=-3"),
    (dict(n=39), b"n=39"),
    (dict(nrows=0), b"nrows=0"),
    (dict(start=36), b"start=36"),
    (dict(start=-3), b"start=-3"),
    (dict(envs=0), b"envs=0"),
    (dict(envs=72), b"envs=72"),
    (dict(envs=5, n=5, start=0), b"envs=5"),      # does not divide nrows = 36
    (dict(n=4), b"n=4"),                          # not a multiple of envs = 3
    (dict(start=4), b"start=4"),
    (dict(pool=0), b"pool=0"),
    (dict(pool=37), b"pool=37"),
    (dict(nrows=3 << 30, pool=1), b"2^31"),       # next_row is int32
]


def _plan(lib, next_row=FAKE, state=FAKE, moves=FAKE, done=FAKE, done_ld=4, flags=FAKE, n=3, nrows=36, start=0, envs=3, pool=5):
    return lib.dgvit_ring_plan_next(next_row, state, moves, done, done_ld, flags, n, nrows, start, envs, pool, None)


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in ("next_row", "state", "moves", "done", "flags")] + SHARED + [
    (dict(done_ld=0), b"done_ld=0"),
    (dict(done_ld=-4), b"done_ld=-4"),
    (dict(next_row=OFF2), b"aligned"),
    (dict(moves=OFF2), b"aligned"),
    (dict(done=OFF2), b"aligned"),
    (dict(state=OFF4), b"aligned"),
], ids=_ids)
def test_ring_plan_next_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _plan(lib, **kw), b"ring_plan_next", word)


def _frames(lib, src0=FAKE, src0_u8=0, src0_ld=60, src1=FAKE, src1_u8=0, src1_ld=60, arena=FAKE, moves=FAKE, ring_u8=0, ring_ld=60, n=3,
            cols=60, nrows=36, start=0, envs=3, pool=5):
    return lib.dgvit_ring_store_frames_shared(src0, src0_u8, src0_ld, src1, src1_u8, src1_ld, arena, moves, ring_u8, ring_ld, n, cols, nrows,
                                              start, envs, pool, None)


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in ("src0", "src1", "arena", "moves")] + SHARED + [
    (dict(cols=0), b"cols=0"),
    (dict(cols=61), b"ring_ld=60"),               # an arena row shorter than a frame
    (dict(ring_ld=62, cols=35), b"ring_ld=62"),   # not a multiple of 4 floats
    (dict(ring_u8=1, ring_ld=60), b"ring_ld=60"),  # a byte arena's rows are multiples of 16
    (dict(src0_ld=59), b"src0_ld=59"),
    (dict(src1_ld=0), b"src1_ld=0"),
    (dict(src0_u8=1), b"uint8 ring"),             # codes into an fp32 arena
    (dict(src1_u8=1), b"uint8 ring"),
    (dict(src0_u8=2, ring_u8=1, ring_ld=64), b"src0_u8=2"),
    (dict(ring_u8=-1), b"ring_u8=-1"),
    (dict(arena=OFF8), b"aligned"),
    (dict(moves=OFF2), b"aligned"),
    (dict(src0=OFF2), b"aligned"),
    (dict(src1=OFF2), b"aligned"),
    (dict(n=1 << 20, nrows=1 << 20, envs=1, pool=1, ring_ld=1 << 26, cols=60), b"more than one launch"),
], ids=_ids)
def test_ring_store_frames_shared_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _frames(lib, **kw), b"ring_store_frames_shared", word)


def _next(lib, next_row=FAKE, idx=FAKE, out=FAKE, nsel=8, nrows=36):
    return lib.dgvit_ring_next_rows(next_row, idx, out, nsel, nrows, None)


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in ("next_row", "idx", "out")] + [
    (dict(nsel=0), b"nsel=0"),
    (dict(nsel=1 << 31), b"nsel=2147483648"),
    (dict(nrows=0), b"nrows=0"),
    (dict(next_row=OFF2), b"aligned"),
    (dict(idx=OFF4), b"aligned"),
    (dict(out=OFF4), b"aligned"),
], ids=_ids)
def test_ring_next_rows_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _next(lib, **kw), b"ring_next_rows", word)


# ------------------------------------------------------------------------------------------------ the restatement against the streams
def _check(ring, frs, lost=()):
    """every written slot: its obs row and what it resolves to as next_obs against its own stream; `lost`: the (e, t) that must return
    their own frame instead -> the number of slots that did"""
    own = 0
    for s in np.flatnonzero(ring.pos >= 0):
        e, t = int(s) % ring.E, int(ring.pos[s])
        assert ring.arena[s] == frs[e][t][0], (s, e, t)
        assert 0 <= ring.next_row[s] < ring.arena_rows
        if (e, t) in lost:
            assert ring.next_row[s] == s and ring.next_frame(s) == frs[e][t][0], ("lost slots return their own obs", s, e, t)
            own += 1
        else:
            assert ring.next_frame(s) == frs[e][t][1], (s, e, t)
    assert 0 <= ring.tail - ring.head <= ring.P and ring.max_live <= ring.P, "live <= P always"
    return own


def _run_vec(E, size, steps, P):
    strs = V.streams(E, steps)
    frs = S.all_frames(strs)
    ring = S.SharedRing(E, size, P)
    for t in range(steps):
        ring.add_vec_frames(strs, frs, t)
        lost, live = S.fifo_truth(strs, E, size, ring.P, t + 1)
        _check(ring, frs, lost)
        assert ring.tail - ring.head == len(live)
    return ring, strs, frs


def _run_ops(P, size=N.SIZE):
    """nstep_ref.scenario(): add, add_batch and on_episode_end() AFTER the store of an episode's last transition"""
    stream, ops = N.scenario()
    frs = S.frames(stream)
    ring = S.SharedRing(1, size, P)
    offered = 0
    for op in ops:
        if op[0] == "episode_end":
            ring.episode_end(np.array([True]))
            continue
        ts = [op[1]] if op[0] == "add" else op[1]
        ring.store(stream, frs, ts)
        offered = ts[-1] + 1
        _check(ring, [frs], S.fifo_truth([stream], 1, size, ring.P, offered)[0])
    return ring, stream, frs


@pytest.mark.parametrize("E, size, steps", SCENARIOS)
def test_every_slot_resolves_to_its_streams_next_frame_with_the_default_pool(E, size, steps):
    """After every step every written slot resolves to its true next frame, lost == 0 with the default P, live <= P always.  These
    streams' episodes are 1, 2, 3, 7 or 11 steps long (mean 4.8): at most 11 of the 36 and 9 of the 37 slots own a pool entry at once,
    the default pool has 18 and 19"""
    ring, strs, frs = _run_vec(E, size, steps, None)
    assert ring.P == S.default_pool(size, E)
    assert ring.lost == 0


def test_nsteps_own_scenario_with_the_default_pool():
    """As above on nstep_ref.scenario() (size 37, one environment, END by on_episode_end() after the store)"""
    ring, stream, frs = _run_ops(None)
    assert ring.P == 19 and ring.lost == 0


@pytest.mark.parametrize("E, size, steps", SCENARIOS)
def test_every_slot_resolves_to_its_streams_next_frame_with_a_pool_that_cannot_overflow(E, size, steps):
    """terminal_frames = size: at most size ended transitions are in the ring"""
    ring, strs, frs = _run_vec(E, size, steps, size)
    assert ring.lost == 0
    if (E, size, steps) == (3, 36, 20):
        assert ring.tail > 0 and ring.head > 0 and ring.max_live == 11, "entries were taken and, behind the wrap, freed"
    if size == E:
        assert ring.tail == 0 and (ring.next_row == size + np.arange(size)).all(), "a step that covers the ring: pending rows only"


def test_nsteps_own_scenario_with_a_pool_that_cannot_overflow():
    ring, stream, frs = _run_ops(N.SIZE)
    assert ring.lost == 0 and ring.tail > 0 and ring.head > 0
    assert any(tr[2] and not tr[1] for tr in stream), "an END that only on_episode_end() tells, set after the store"


@pytest.mark.parametrize("E, size, steps, P", [(3, 36, 20, 2), (1, 37, 52, 2), (3, 36, 20, 1)])
def test_a_pool_that_is_too_small_loses_exactly_what_the_fifo_rule_names(E, size, steps, P):
    """P chosen so that the reference overflows: lost > 0, the slots the stream-level FIFO rule names return their own frame, every other
    slot is still right (``_check`` after every step), and some ends were stored all the same"""
    ring, strs, frs = _run_vec(E, size, steps, P)
    lost, live = S.fifo_truth(strs, E, size, P, steps)
    assert ring.lost > 0 and len(lost) > 0 and _check(ring, frs, lost) == len(lost)
    assert ring.tail > 0 and len(live) > 0, "at least one end is stored"
    assert ring.lost >= len(lost), "the counter also counts lost slots that have left the ring since"


def test_lost_scenario_on_nsteps_own_ops():
    ring, stream, frs = _run_ops(2)
    assert ring.lost > 0 and ring.tail > 0


def test_a_step_that_covers_the_whole_ring():
    """size == E: no slot has a lane predecessor in the ring, every next_obs is a pending row, whatever ends"""
    strs = V.streams(4, 6)
    frs = S.all_frames(strs)
    ring = S.SharedRing(4, 4)
    for t in range(6):
        ring.add_vec_frames(strs, frs, t)
        assert ring.next_row.tolist() == [4, 5, 6, 7] and ring.state() == [0, 0, 0]
        assert [ring.next_frame(s) for s in range(4)] == [f[t][1] for f in frs]


def test_add_batch_with_an_interior_done():
    """one add_batch of 7 rows whose third has done = 1: its next_obs goes from the call's own rows into the pool, the fourth row starts
    a new episode, and the run's last next_obs is the pending row"""
    stream = [(np.float32(0), np.float32(1.0 if t == 2 else 0.0), False) for t in range(7)]
    frs = S.frames(stream)
    assert frs[3][0] != frs[2][1] and frs[2][0] == frs[1][1]
    ring = S.SharedRing(1, 10, 2)
    ring.store(stream, frs, range(7))
    assert ring.next_row[:7].tolist() == [1, 2, 11, 4, 5, 6, 10] and ring.state() == [0, 1, 0]
    _check(ring, [frs])
    more = stream + [(np.float32(0), np.float32(0), False)] * 6        # through the wrap: slot 2 is overwritten, its entry freed
    frs = S.frames(more)
    ring.store(more, frs, range(7, 13))
    assert ring.state() == [1, 1, 0]
    _check(ring, [frs])


def test_add_batch_over_the_whole_ring():
    """n == size: the first row's predecessor is the slot the call's own last row overwrites, so it does not count -- its done in the ring
    is already the new row's"""
    stream = [(np.float32(0), np.float32(1.0 if t in (4, 8) else 0.0), False) for t in range(15)]
    frs = S.frames(stream)
    ring = S.SharedRing(1, 5, 1)
    ring.store(stream, frs, range(5))          # slot 4 is terminal and the newest: pending
    assert ring.next_row.tolist() == [1, 2, 3, 4, 5]
    _check(ring, [frs])
    ring.store(stream, frs, range(5, 10))      # slot 4 (t = 4) is overwritten with the rest; slot 3 (t = 8) takes the pool's one entry
    assert ring.next_row.tolist() == [1, 2, 3, 6, 5] and ring.state() == [0, 1, 0]
    _check(ring, [frs])
    ring.store(stream, frs, range(10, 15))     # and frees it
    assert ring.state() == [1, 1, 0]
    _check(ring, [frs])


def test_an_end_set_by_on_episode_end_after_the_store():
    stream = [(np.float32(0), np.float32(0), t == 1) for t in range(4)]
    frs = S.frames(stream)
    ring = S.SharedRing(1, 8, 1)
    ring.store(stream, frs, [0])
    ring.store(stream, frs, [1])
    assert ring.next_row[:2].tolist() == [1, 8]
    ring.episode_end(np.array([True]))         # after the store: only the next store can see it
    ring.store(stream, frs, [2])
    assert ring.next_row[:3].tolist() == [1, 9, 8] and ring.state() == [0, 1, 0]
    ring.store(stream, frs, [3])
    _check(ring, [frs])
