"""CPU (no GPU): the random-shift gather's C entry point, its argument checks, the Python checks in front of it, and the statistics of
the host restatement of its draw (tests/replay_shift_ref.py).  Every library call here fails its argument check before any launch: the
pointers are never dereferenced."""
import ctypes
import os

import numpy as np
import pytest
import torch

import replay_shift_ref as R

FAKE = ctypes.c_void_p(0x1000)   # non-null, 16-byte aligned, never read: only argument checks run


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


def test_symbol_is_exported_and_bound(lib):
    from dgvit_amd import _lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(raw, "dgvit_gather_shift_frames")
    res, args = L.SIGNATURES["dgvit_gather_shift_frames"]
    assert res is ctypes.c_int and len(args) == 14
    assert args[11] is ctypes.c_ulonglong and args[4] is ctypes.c_longlong
    with open(os.path.join(os.path.dirname(L.LIB_PATH), os.pardir, "include", "dgvit_hip.h")) as f:
        assert "dgvit_gather_shift_frames(" in f.read()


def test_abi_version_is_unchanged(lib):
    assert lib.dgvit_abi_version() == 7


def _call(lib, src=FAKE, out=FAKE, nsel=8, H=8, W=12, row=96, nrows=16, pad=4, stream_id=0):
    return lib.dgvit_gather_shift_frames(src, None, out, None, nsel, H, W, row, nrows, pad, stream_id, 1, None, None)


@pytest.mark.parametrize("kw, word", [
    (dict(src=None), b"null"),
    (dict(out=None), b"null"),
    (dict(nsel=0), b"nsel=0"),
    (dict(nsel=-3), b"nsel=-3"),
    (dict(nrows=0), b"nrows=0"),
    (dict(H=0), b"H=0"),
    (dict(W=-1), b"W=-1"),
    (dict(row=98), b"row_floats=98"),          # not a multiple of 4
    (dict(row=92), b"row_floats=92"),          # a multiple of 4 below H * W = 96
    (dict(pad=-1), b"pad=-1"),
    (dict(pad=8), b"pad=8"),                   # pad == H
    (dict(H=12, W=8, row=96, pad=8), b"pad=8"),    # pad == W
    (dict(stream_id=-1), b"stream_id=-1"),
    (dict(stream_id=65536), b"stream_id=65536"),
], ids=lambda v: None if isinstance(v, bytes) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_bad_arguments_are_refused_before_any_launch(lib, kw, word):
    assert _call(lib, **kw) != 0
    msg = lib.dgvit_last_error()
    assert b"gather_shift_frames" in msg and word in msg, msg


@pytest.mark.parametrize("bad", [-1, 1.5, "4", None, True, 16, 20])
def test_sample_refuses_bad_random_shift(bad):
    """the check runs before the library is loaded or an index is drawn: a buffer without storage is enough to reach it"""
    from dgvit_amd.replay import DeviceReplayBuffer
    buf = object.__new__(DeviceReplayBuffer)
    buf.shapes = {"obs": (16, 20)}
    with pytest.raises(ValueError, match="random_shift"):
        buf.sample(4, random_shift=bad)


@pytest.mark.parametrize("bad", [-1, 2.0, None, 7, 9])
def test_random_shift_refuses_bad_pad(bad):
    from dgvit_amd import preprocess
    with pytest.raises(ValueError, match="pad"):
        preprocess.random_shift(torch.zeros(3, 7, 9), bad)


def test_random_shift_refuses_cpu_tensors():
    import dgvit_amd
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):
        dgvit_amd.preprocess.random_shift(torch.zeros(3, 8, 12), 2)
    with pytest.raises(dgvit_amd.DgvitError, match=r"\(B, H, W\)"):
        dgvit_amd.preprocess.random_shift(torch.zeros(8, 12), 2)


def test_device_replay_buffer_still_refuses_a_cpu_device():
    import dgvit_amd
    from dgvit_amd.replay import DeviceReplayBuffer
    with pytest.raises(dgvit_amd.DgvitError):
        DeviceReplayBuffer(8, obs_shape=(16, 20), device="cpu")


# ------------------------------------------------------------------------------------------------ the restated draw
@pytest.fixture(scope="module")
def draws():
    return [R.draw_shifts(4096, 4, R.SEED, s) for s in (0, 1)]


@pytest.mark.parametrize("stream", [0, 1])
def test_restated_draw_is_uniform_over_the_nine_shifts(draws, stream):
    """4096 samples over 9 values: expected count 455, sigma = sqrt(4096 * 1/9 * 8/9) = 20; the band 355 .. 555 is 5 sigma"""
    d = draws[stream]
    assert d.dtype == np.int32 and d.shape == (4096, 2)
    for axis in (0, 1):
        counts = np.bincount(d[:, axis] + 4, minlength=9)
        assert counts.size == 9, "a shift outside [-4, 4]"
        assert counts.min() >= 355 and counts.max() <= 555, counts


def test_restated_streams_draw_different_shifts(draws):
    a, b = draws
    assert (a[:, 0] != b[:, 0]).sum() > 2048 and (a[:, 1] != b[:, 1]).sum() > 2048
    assert (a[:, 0] != a[:, 1]).sum() > 2048, "dy and dx come from different Philox words"


def test_restated_draw_covers_the_range_at_other_pads():
    for pad in (1, 3):
        d = R.draw_shifts(2048, pad, R.SEED, 0)
        assert d.min() == -pad and d.max() == pad
    assert not R.draw_shifts(64, 0, R.SEED, 0).any()


def test_ref_shift_is_pad_then_crop():
    """the torch restatement against an element-wise clamp written out in numpy"""
    f = torch.arange(2 * 5 * 6, dtype=torch.float32).reshape(2, 5, 6)
    s = torch.tensor([[-4, 3], [2, -1]], dtype=torch.int32)
    got = R.ref_shift(f, s, 4).numpy()
    for i, (dy, dx) in enumerate(s.tolist()):
        ys = np.clip(np.arange(5) + dy, 0, 4)
        xs = np.clip(np.arange(6) + dx, 0, 5)
        np.testing.assert_array_equal(got[i], f[i].numpy()[np.ix_(ys, xs)])
