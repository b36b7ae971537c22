"""CPU (no GPU): the replay ring as a file -- the entry points dgvit_ring_export and dgvit_per_set_leaves with their
argument checks, replay.export_layout against the numpy restatement tests/replay_file_ref.py, the restatement against the streams alone,
and the keyword checks of save_transitions / load_transitions.  Every library call here fails its argument check before any launch: the
pointers are never dereferenced."""
import ctypes
import os

import numpy as np
import pytest
import torch

import replay_file_ref as F
import shared_next_ref as S
import vec_replay_ref as V

FAKE = ctypes.c_void_p(0x1000)   # non-null, 16-byte aligned, never read: only argument checks run
OFF8 = ctypes.c_void_p(0x1008)
OFF2 = ctypes.c_void_p(0x1002)

NAMES = ("dgvit_ring_export", "dgvit_per_set_leaves")
SHAPES = [(8, 16), (6, 10), (5, 7)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


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
    assert L.SIGNATURES["dgvit_ring_export"] == (I, [L.dgvit_ring_view, P, LL, LL, LL, LL, LL, LL, P])
    assert L.SIGNATURES["dgvit_per_set_leaves"] == (I, [P, LL, LL, LL, P, P])
    assert L.SIGNATURES["dgvit_per_set_range"] == (I, [P, LL, LL, LL, P]), "no existing signature changes"
    names = [n for n, _ in L.dgvit_ring_view._fields_]
    assert names == ["obs", "next_obs", "next_row", "small", "flags", "leaves", "frame_ld", "next_rows", "small_cols", "small_ld", "frame_u8"]
    assert "} dgvit_ring_view;" in header


def test_abi_version_is_unchanged(lib):
    from dgvit_amd import _lib as L
    assert lib.dgvit_abi_version() == 7 and L.ABI_VERSION == 7


def _ids(v):
    return None if isinstance(v, bytes) else "-".join(f"{k}={x if not isinstance(x, ctypes.c_void_p) else x.value}" for k, x in v.items())


def _msg(lib, rc, name, word):
    assert rc == -1, "DGVIT_ERR_ARG"
    msg = lib.dgvit_last_error()
    assert name in msg and word in msg, msg


def _export(lib, obs=FAKE, next_obs=FAKE, next_row=None, small=FAKE, small_at=None, flags=FAKE, leaves=None, frame_ld=60, next_rows=36,
            small_cols=2, small_ld=4, frame_u8=0, out=FAKE, out_bytes=1 << 20, cols=60, nrows=36, oldest=0, a0=0, n=5):
    """a (6, 10) fp32 ring of 36 slots; `small_at` = the one small field that `small`, `small_cols` and `small_ld` are meant for"""
    from dgvit_amd import _lib as L
    v = L.dgvit_ring_view()
    v.obs, v.next_obs, v.next_row, v.flags, v.leaves = obs, next_obs, next_row, flags, leaves
    v.frame_ld, v.next_rows, v.frame_u8 = frame_ld, next_rows, frame_u8
    for f in range(L.SMALL_FIELDS):
        mine = small_at is None or small_at == f
        ptr = small if mine else FAKE
        v.small[f] = None if ptr is None else ptr.value
        v.small_cols[f], v.small_ld[f] = (small_cols, small_ld) if small_at == f else ((2, 2, 1, 2, 1)[f], 4)
    return lib.dgvit_ring_export(v, out, out_bytes, cols, nrows, oldest, a0, n, None)


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in ("obs", "next_obs", "out")] + [
    (dict(small=None, small_at=3), b"small[3]"),
    (dict(n=0), b"n=0"),
    (dict(n=-2), b"n=-2"),
    (dict(n=37), b"n=37"),
    (dict(nrows=0), b"nrows=0"),
    (dict(a0=-1), b"a0=-1"),
    (dict(a0=32, n=5), b"a0=32"),                 # ages 32 .. 37 of a ring of 36
    (dict(a0=36, n=1), b"a0=36"),
    (dict(oldest=36), b"oldest=36"),
    (dict(oldest=-1), b"oldest=-1"),
    (dict(cols=0), b"cols=0"),
    (dict(cols=61), b"frame_ld=60"),              # a ring row shorter than a frame
    (dict(frame_ld=62), b"frame_ld=62"),          # not a multiple of 4 floats
    (dict(frame_u8=1, frame_ld=60), b"frame_ld=60"),   # a byte ring's rows are multiples of 16
    (dict(frame_u8=2), b"frame_u8=2"),
    (dict(next_rows=40), b"next_rows=40"),        # a two-matrix ring has nrows rows of next_obs
    (dict(next_row=FAKE, next_rows=35), b"next_rows=35"),   # an arena holds at least the ring
    (dict(next_row=OFF2, next_rows=40), b"aligned"),
    (dict(small_cols=0, small_at=1), b"small_cols[1]=0"),
    (dict(small_cols=5, small_ld=4, small_at=4), b"small_ld[4]=4"),
    (dict(small=OFF2, small_at=0), b"small[0]"),
    (dict(obs=OFF8), b"aligned"),
    (dict(next_obs=OFF8), b"aligned"),
    (dict(out=OFF8), b"out, the chunk"),          # a misaligned chunk
    (dict(leaves=OFF2), b"leaves"),
    (dict(out_bytes=2623), b"out_bytes=2623"),    # 5 transitions of this ring are 2624 bytes
    (dict(out_bytes=2624, leaves=FAKE), b"out_bytes=2624"),   # ... and 2656 with their leaves
    (dict(n=1 << 20, nrows=1 << 20, next_rows=1 << 20, frame_ld=1 << 25, cols=1 << 25, out_bytes=1 << 62), b"more than one launch"),
], ids=_ids)
def test_ring_export_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _export(lib, **kw), b"ring_export", word)


def test_ring_export_size_check_is_the_layout(lib):
    """out_bytes one short of replay_file_ref.layout's total is refused with the total in the message"""
    for n in (1, 5, 36):
        for pri in (False, True):
            total = F.layout(n, (6, 10), 2, 2, 4, pri)[1]
            rc = _export(lib, n=n, out_bytes=total - 1, leaves=FAKE if pri else None)
            _msg(lib, rc, b"ring_export", f"the {total} bytes".encode())


def _set_leaves(lib, tree=FAKE, capacity=100, first=0, count=10, leaves=FAKE):
    return lib.dgvit_per_set_leaves(tree, capacity, first, count, leaves, None)


@pytest.mark.parametrize("kw, word", [
    (dict(tree=None), b"null"),
    (dict(leaves=None), b"leaves must not be null"),
    (dict(capacity=0), b"capacity=0"),
    (dict(capacity=(1 << 24) + 1), b"capacity=16777217"),
    (dict(first=-1), b"first=-1"),
    (dict(first=100, count=1), b"first=100"),
    (dict(count=0), b"count=0"),
    (dict(count=-4), b"count=-4"),
    (dict(first=95, count=6), b"count=6"),        # a range that would wrap
    (dict(first=1, count=1 << 62), b"first=1"),
    (dict(tree=OFF8), b"aligned"),
    (dict(leaves=OFF2), b"leaves must be 4-byte aligned"),
], ids=_ids)
def test_per_set_leaves_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _set_leaves(lib, **kw), b"per_set_leaves", word)


# ------------------------------------------------------------------------------------------------ the layout
@pytest.mark.parametrize("prioritized", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["fp32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("n", [1, 5, 4096])
def test_export_layout_is_the_restatement(n, shape, dtype, prioritized):
    from dgvit_amd import replay
    blocks, total = replay.export_layout(n, shape, V.PSTATE, V.ACT, dtype, prioritized)
    ref, ref_total = F.layout(n, shape, V.PSTATE, V.ACT, 1 if dtype is torch.uint8 else 4, prioritized)
    assert blocks == ref and total == ref_total and list(blocks) == list(ref)
    assert list(blocks) == list(F.FIELDS) + ["end"] + (["priority"] if prioritized else [])
    ends = [off + nb for off, nb in blocks.values()]
    for (off, nb), before in zip(blocks.values(), [0] + ends[:-1]):
        assert off % 16 == 0 and before <= off < before + 16, "16-byte aligned and no more padding than that"
    assert total % 16 == 0 and ends[-1] <= total < ends[-1] + 16
    assert blocks["obs"][1] == n * shape[0] * shape[1] * (1 if dtype is torch.uint8 else 4) and blocks["end"][1] == n


def test_the_constants_are_the_restatements():
    from dgvit_amd import replay
    assert replay.FILE_FIELDS == F.FIELDS and replay.META_KEYS == F.META_KEYS and replay.FILE_FORMAT_VERSION == 1
    assert replay.FLAG_END == F.END


@pytest.mark.parametrize("n", [0, -1, True, 2.0, "5"], ids=repr)
def test_export_layout_refuses_a_bad_n(n):
    from dgvit_amd import replay
    with pytest.raises(ValueError, match="n must be"):
        replay.export_layout(n, (6, 10), 2, 2, torch.uint8)


# ------------------------------------------------------------------------------------------------ the keyword checks
def _bare():
    from dgvit_amd import replay
    return object.__new__(replay.DeviceReplayBuffer), object.__new__(replay.PrioritizedDeviceReplayBuffer)


@pytest.mark.parametrize("chunk", [0, -5, True, 2.5, "4096", None], ids=repr)
def test_a_bad_chunk_raises_before_any_device_is_touched(chunk, tmp_path):
    for buf in _bare():
        with pytest.raises(ValueError, match="chunk"):
            buf.save_transitions(tmp_path / "ring", chunk=chunk)
    assert not os.listdir(tmp_path)


@pytest.mark.parametrize("kw, word", [(dict(priorities="keep"), "priorities"), (dict(priorities=None), "priorities"),
                                      (dict(priorities=True), "priorities"), (dict(restore_rng=1), "restore_rng"),
                                      (dict(restore_rng="yes"), "restore_rng"), (dict(restore_rng=0.0), "restore_rng")], ids=str)
def test_bad_load_keywords_raise_before_any_device_is_touched(kw, word, tmp_path):
    for buf in _bare():
        with pytest.raises(ValueError, match=word):
            buf.load_transitions(tmp_path / "ring", **kw)


def test_overwrite_must_be_a_bool(tmp_path):
    for buf in _bare():
        with pytest.raises(ValueError, match="overwrite"):
            buf.save_transitions(tmp_path / "ring", overwrite="yes")


# ------------------------------------------------------------------------------------------------ the restatement against the streams
@pytest.mark.parametrize("E, size, steps", [(3, 36, 20), (3, 36, 7), (1, 37, 52), (4, 8, 7)])
def test_the_ages_of_the_restatement_are_the_streams_order(E, size, steps):
    """age order = the last stored / E vector steps, step-major: stated from the ring's slots and from the streams alone"""
    strs = V.streams(E, steps)
    ring = V.VecRing(E, size)
    for t in range(steps):
        ring.offer(strs, t)
    slots, t, e = F.ages(ring)
    t2, e2 = F.stream_order(ring)
    assert np.array_equal(t, t2) and np.array_equal(e, e2)
    assert len(slots) == min(size, E * steps) and t[-1] == steps - 1 and t[0] == max(0, steps - size // E)
    frs = S.all_frames(strs)
    d = F.data(strs, frs, (5, 7))
    out = F.expected(ring, d, (5, 7), True)
    assert out["obs"].dtype == np.uint8 and out["obs"].shape == (len(slots), 5, 7) and out["rew"].shape == (len(slots), 1)
    assert np.array_equal(out["end"], np.array([strs[j][i][2] for i, j in zip(t, e)], np.uint8))
    assert np.array_equal(out["rew"][:, 0], np.array([strs[j][i][0] for i, j in zip(t, e)], np.float32))


def test_a_shared_restatement_resolves_to_the_streams_next_frame():
    """with a pool that cannot overflow, next_obs of every age is its own stream's next frame: the two-matrix file"""
    E, size, steps = 3, 36, 20
    strs = V.streams(E, steps)
    frs = S.all_frames(strs)
    d = F.data(strs, frs, (6, 10))
    plain, shared = V.VecRing(E, size), S.SharedRing(E, size, size)
    for t in range(steps):
        plain.offer(strs, t)
        shared.add_vec_frames(strs, frs, t)
    a, b = F.expected(plain, d, (6, 10), False), F.expected(shared, d, (6, 10), False)
    assert shared.lost == 0 and set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype, k
