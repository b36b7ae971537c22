"""CPU (no GPU): the replay ring of E parallel environments -- the ``num_envs`` check, the entry points
dgvit_ring_store_frames, dgvit_ring_store_small and dgvit_nstep_walk_strided with their argument checks, and the numpy restatement
tests/vec_replay_ref.py against the truth computed from each environment's stream alone.  Every library call here fails its argument check
before any launch: the pointers are never dereferenced."""
import ctypes
import os

import numpy as np
import pytest

import nstep_ref as N
import vec_replay_ref as V

FAKE = ctypes.c_void_p(0x1000)   # non-null, 16-byte aligned, never read: only argument checks run
OFF8 = ctypes.c_void_p(0x1008)
OFF2 = ctypes.c_void_p(0x1002)

NAMES = ("dgvit_ring_store_frames", "dgvit_ring_store_small", "dgvit_nstep_walk_strided")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


# ------------------------------------------------------------------------------------------------ the Python checks
@pytest.mark.parametrize("bad", [0, -1, True, 2.0, 5, 37, 72], ids=str)
def test_bad_num_envs_raises_before_any_device_is_touched(bad):
    """size = 36: 5 does not divide it, 37 and 72 are above it.  No GPU is needed to get here (without the keyword this is a TypeError)"""
    from dgvit_amd import replay
    for cls in (replay.DeviceReplayBuffer, replay.PrioritizedDeviceReplayBuffer):
        with pytest.raises(ValueError, match="num_envs"):
            cls(36, obs_shape=(6, 10), num_envs=bad)
    with pytest.raises(ValueError, match="num_envs"):
        replay._num_envs(bad, 36)


def test_good_num_envs_pass_the_helper():
    from dgvit_amd import replay
    assert [replay._num_envs(v, 36) for v in (1, 2, 3, 36, np.int64(12))] == [1, 2, 3, 36, 12]


# ------------------------------------------------------------------------------------------------ the entry points
def test_symbols_are_exported_bound_and_declared(lib):
    from dgvit_amd import _lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    with open(os.path.join(os.path.dirname(L.LIB_PATH), os.pardir, "include", "dgvit_hip.h")) as f:
        header = f.read()
    P, I, LL, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double
    for name in NAMES:
        assert hasattr(raw, name)
        assert "int " + name + "(" in header
    assert L.SIGNATURES["dgvit_ring_store_frames"] == (I, [P, I, LL, P, I, LL, P, P, I, LL, LL, LL, LL, LL, P])
    assert L.SIGNATURES["dgvit_ring_store_small"] == (I, [L.dgvit_small_fields, P, P, I, LL, LL, LL, P])
    assert L.SIGNATURES["dgvit_nstep_walk_strided"] == (I, [P, LL, P, LL, P, P, LL, P, LL, LL, LL, I, D] + [P] * 7)
    assert L.SIGNATURES["dgvit_nstep_walk"] == (I, [P, LL, P, LL, P, P, LL, P, LL, LL, I, D] + [P] * 7), "the first walk keeps its signature"
    assert L.SIGNATURES["dgvit_ring_mark"] == (I, [P, LL, LL, LL, P])
    assert "#define DGVIT_SMALL_FIELDS 5" in header and L.SMALL_FIELDS == 5
    assert ctypes.sizeof(L.dgvit_small_fields) == 5 * (8 + 8 + 8 + 4 + 4), "two pointer arrays, one of long long, two of int: no padding"
    from dgvit_amd import replay
    assert len(replay.SMALL_FIELDS) == 5 and set(replay.SMALL_FIELDS) | set(replay.FRAME_FIELDS) == {"obs", "pobs", "act", "rew", "next_obs",
                                                                                                    "next_pobs", "done"}


def test_abi_version_is_unchanged(lib):
    assert lib.dgvit_abi_version() == 7


def _ids(v):
    return None if isinstance(v, bytes) else "-".join(f"{k}={x if not isinstance(x, ctypes.c_void_p) else x.value}" for k, x in v.items())


def _msg(lib, rc, name, word):
    assert rc == -1, "DGVIT_ERR_ARG"
    msg = lib.dgvit_last_error()
    assert name in msg and word in msg, msg


def _frames(lib, src0=FAKE, src0_u8=0, src0_ld=60, src1=FAKE, src1_u8=0, src1_ld=60, ring0=FAKE, ring1=FAKE, ring_u8=0, ring_ld=60, n=3,
            cols=60, nrows=36, start=0):
    return lib.dgvit_ring_store_frames(src0, src0_u8, src0_ld, src1, src1_u8, src1_ld, ring0, ring1, ring_u8, ring_ld, n, cols, nrows, start,
                                       None)


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in ("src0", "src1", "ring0", "ring1")] + [
    (dict(n=0), b"n=0"),
    (dict(n=-3), b"n=-3"),
    (dict(n=37), b"n=37"),
    (dict(nrows=0), b"nrows=0"),
    (dict(start=36), b"start=36"),
    (dict(start=-1), b"start=-1"),
    (dict(start=1 << 40), b"start=1099511627776"),
    (dict(cols=0), b"cols=0"),
    (dict(cols=61), b"ring_ld=60"),               # a ring row shorter than a frame
    (dict(ring_ld=62, cols=35), b"ring_ld=62"),   # not a multiple of 4 floats
    (dict(ring_u8=1, ring_ld=60), b"ring_ld=60"),  # a byte ring's rows are multiples of 16
    (dict(src0_ld=59), b"src0_ld=59"),
    (dict(src1_ld=0), b"src1_ld=0"),
    (dict(src0_u8=1), b"uint8 ring"),             # codes into an fp32 ring
    (dict(src1_u8=1), b"uint8 ring"),
    (dict(src0_u8=2, ring_u8=1, ring_ld=64), b"src0_u8=2"),
    (dict(ring_u8=-1), b"ring_u8=-1"),
    (dict(ring0=OFF8), b"aligned"),
    (dict(ring1=OFF8), b"aligned"),
    (dict(src0=OFF2), b"aligned"),
    (dict(src1=OFF2), b"aligned"),
], ids=_ids)
def test_ring_store_frames_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _frames(lib, **kw), b"ring_store_frames", word)


def _small(lib, flags=FAKE, episode_end=FAKE, end_f32=0, n=3, nrows=36, start=0, **field):
    from dgvit_amd import _lib as L
    s = L.dgvit_small_fields()
    for j in range(5):
        s.src[j], s.ring[j], s.src_ld[j], s.cols[j], s.ring_ld[j] = 0x1000, 0x1000, 2, 2, 4
    for k, v in field.items():                      # e.g. src2=None, cols4=5: member and field index
        getattr(s, k[:-1])[int(k[-1])] = v.value if isinstance(v, ctypes.c_void_p) else v
    return lib.dgvit_ring_store_small(s, flags, episode_end, end_f32, n, nrows, start, None)


@pytest.mark.parametrize("kw, word", [({f"src{j}": None}, b"null") for j in range(5)] + [({f"ring{j}": None}, b"null") for j in range(5)] + [
    (dict(flags=None), b"null"),                  # ends without flags to write them to
    (dict(n=0), b"n=0"),
    (dict(n=-1), b"n=-1"),
    (dict(n=37), b"n=37"),
    (dict(n=5), b"n=5"),                          # does not divide nrows = 36
    (dict(nrows=0), b"nrows=0"),
    (dict(start=36), b"start=36"),
    (dict(start=-3), b"start=-3"),
    (dict(end_f32=2), b"end_f32=2"),
    (dict(end_f32=1, episode_end=OFF2), b"aligned"),
    (dict(cols0=0), b"cols[0]=0"),
    (dict(cols3=5), b"cols[3]=5"),                # more than the ring row holds
    (dict(ring_ld1=6, cols1=2), b"ring_ld[1]=6"),
    (dict(src_ld4=1), b"src_ld[4]=1"),
    (dict(src2=OFF2), b"aligned"),
    (dict(ring2=OFF8), b"aligned"),
], ids=_ids)
def test_ring_store_small_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _small(lib, **kw), b"ring_store_small", word)


def _walk(lib, rew=FAKE, rew_ld=4, done=FAKE, done_ld=4, flags=FAKE, next_small=FAKE, small_ld=4, idx=FAKE, nsel=8, nrows=36, stride=3, n=3,
          gamma=0.99, ret_out=FAKE, done_out=FAKE, discount_out=FAKE, next_small_out=FAKE, steps_out=FAKE, tail_out=FAKE):
    return lib.dgvit_nstep_walk_strided(rew, rew_ld, done, done_ld, flags, next_small, small_ld, idx, nsel, nrows, stride, n, gamma, ret_out,
                                        done_out, discount_out, next_small_out, steps_out, tail_out, None)


WALK_POINTERS = ("rew", "done", "flags", "next_small", "idx", "ret_out", "done_out", "discount_out", "next_small_out", "steps_out", "tail_out")


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in WALK_POINTERS] + [
    (dict(stride=0), b"stride=0"),
    (dict(stride=-3), b"stride=-3"),
    (dict(stride=37), b"stride=37"),
    (dict(nsel=0), b"nsel=0"),
    (dict(nsel=1 << 31), b"nsel=2147483648"),
    (dict(nrows=0), b"nrows=0"),
    (dict(n=0), b"n=0"),
    (dict(n=65), b"n=65"),
    (dict(gamma=float("nan")), b"gamma="),
    (dict(gamma=1.5), b"gamma=1.5"),
    (dict(rew_ld=0), b"rew_ld=0"),
    (dict(done_ld=-4), b"done_ld=-4"),
    (dict(small_ld=6), b"small_ld=6"),
    (dict(next_small=OFF8), b"16-byte aligned"),
    (dict(next_small_out=OFF8), b"16-byte aligned"),
    (dict(rew=OFF2), b"aligned"),
    (dict(idx=ctypes.c_void_p(0x1004)), b"aligned"),
    (dict(tail_out=ctypes.c_void_p(0x1004)), b"aligned"),
], ids=_ids)
def test_nstep_walk_strided_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _walk(lib, **kw), b"nstep_walk_strided", word)


# ------------------------------------------------------------------------------------------------ the restatement against the streams
def _compare(ring, strs, newest, n, gamma):
    """every written slot of ``ring``: the strided walk against the truth of the slot's own environment -> the stop reasons seen"""
    slots = np.flatnonzero(ring.pos >= 0)
    w = ring.walk(slots, n, gamma)
    for j, s in enumerate(slots):
        e, t = int(s) % ring.E, int(ring.pos[s])
        ret, disc, m, tail, done, why = V.truth(strs, e, t, newest, n, gamma)
        assert w["ret64"][j] == ret and w["disc64"][j] == disc, (s, n, gamma)
        assert w["steps"][j] == m and w["done"][j] == done and w["why"][j] == why, (s, n, gamma)
        assert w["tail"][j] % ring.E == e and ring.pos[w["tail"][j]] == tail, "the tail is the same environment's"
        assert w["tol"][j] == V.tolerance(strs[e], t, m, gamma, ret)
    return set(w["why"])


@pytest.mark.parametrize("E, size, steps", [(3, 36, 20), (1, 37, 52), (4, 4, 6), (4, 8, 7)])
def test_vector_ring_walk_equals_each_environments_stream(E, size, steps):
    strs = V.streams(E, steps)
    ring, seen, on_newest = V.VecRing(E, size), set(), 0
    for t in range(steps):
        ring.offer(strs, t)
        base = (t * E) % size
        assert ring.next_index == (base + E) % size and ring.stored == min((t + 1) * E, size)
        assert np.array_equal(np.flatnonzero(ring.flags & N.HEAD), base + np.arange(E)), "exactly the newest step carries HEAD"
        on_newest += sum(bool(s[t][1] != 0 or s[t][2]) for s in strs)
        for n in (1, 3, 64):
            seen |= _compare(ring, strs, t, n, 0.99)
    for n in N.NS:
        for gamma in N.GAMMAS:
            seen |= _compare(ring, strs, steps - 1, n, gamma)
    assert on_newest > 0, "a stream ended exactly on the newest step at least once"
    if (E, size, steps) == (3, 36, 20):
        assert ring.next_index == 24 and ring.stored == 36, "the ring wrapped: 8 steps were overwritten"
        want = {frozenset(w) for w in (("done",), ("end",), ("done", "end"), ("head",), ("n",), ("head", "n"), ("done", "head"), ("end", "head"))}
        assert want <= seen, want - seen


def test_stride_1_is_nstep_refs_walk_on_its_own_scenario():
    stream, ops = N.scenario()
    ref = N.offer(N.Ring(N.SIZE), stream, ops)
    ring = V.VecRing(1, N.SIZE)
    for t in range(len(stream)):
        ring.offer([stream], t)
    assert np.array_equal(ring.flags, ref.flags) and np.array_equal(ring.pos, ref.pos) and np.array_equal(ring.rew, ref.rew)
    for n in N.NS:
        for gamma in N.GAMMAS:
            a, b = ring.walk(np.arange(N.SIZE), n, gamma), ref.walk(np.arange(N.SIZE), n, gamma)
            for k in ("ret64", "disc64", "steps", "tail", "done", "rew", "discount", "tol"):
                assert np.array_equal(a[k], b[k]), (k, n, gamma)
            assert a["why"] == b["why"]


def test_flag_rules_of_the_store_and_of_on_episode_end():
    ring = V.VecRing(2, 6, tracked=False)
    ring.add_vec([0, 0], [0, 0], 0)
    assert ring.flags is None
    ring.track()                                             # tracking that starts late knows only the newest step
    assert ring.flags.tolist() == [N.HEAD, N.HEAD, 0, 0, 0, 0]
    ring.add_vec([0, 0], [0, 0], 1, end=[False, True])
    assert ring.flags.tolist() == [0, 0, N.HEAD, N.HEAD | N.END, 0, 0]
    ring.episode_end(np.array([True, False]))
    assert ring.flags.tolist() == [0, 0, N.HEAD | N.END, N.HEAD | N.END, 0, 0]
    ring.add_vec([0, 0], [0, 0], 2)
    assert ring.flags.tolist() == [0, 0, N.END, N.END, N.HEAD, N.HEAD]
    ring.episode_end([1])
    ring.add_vec([0, 0], [0, 0], 3)                          # wraps: the overwritten slots forget their marks
    assert ring.flags.tolist() == [N.HEAD, N.HEAD, N.END, N.END, 0, N.END]
    whole = V.VecRing(3, 3)
    whole.add_vec([0, 0, 0], [0, 0, 0], 0, end=[1, 0, 0])
    whole.add_vec([0, 0, 0], [0, 0, 0], 1, end=[0, 0, 1])    # the step covers the whole ring: no previous step to take HEAD from
    assert whole.flags.tolist() == [N.HEAD, N.HEAD, N.HEAD | N.END]


def test_add_and_add_batch_point_to_add_vec_without_a_device():
    import dgvit_amd
    from dgvit_amd import replay
    buf = object.__new__(replay.DeviceReplayBuffer)          # no device behind it: the refusal comes first
    buf.num_envs = 3
    z = np.zeros((3, 2), np.float32)
    for call in (buf.add, buf.add_batch):
        with pytest.raises(dgvit_amd.DgvitError, match="add_vec"):
            call(obs=z, pobs=z, act=z, rew=z, next_obs=z, next_pobs=z, done=z)
    with pytest.raises(ValueError, match="envs"):
        buf.on_episode_end()
    buf.num_envs = 1
    with pytest.raises(ValueError, match="envs"):
        buf.on_episode_end(envs=[0])
