"""CPU (no GPU): the C entry points of the uint8 replay ring, their argument checks, the Python checks in front of them, and the host
restatement of the number formats (tests/replay_u8_ref.py) against torch and numpy.  Every library call here fails its argument check
before any launch: the pointers are never dereferenced."""
import ctypes
import os

import numpy as np
import pytest
import torch

import replay_u8_ref as R

FAKE = ctypes.c_void_p(0x1000)   # non-null, 16-byte aligned, never read: only argument checks run
ODD = ctypes.c_void_p(0x1004)    # 4-byte but not 16-byte aligned
ODD1 = ctypes.c_void_p(0x1001)

NAMES = ("dgvit_quantize_rows_u8", "dgvit_gather_rows_u8", "dgvit_gather_shift_frames_u8")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


def test_symbols_are_exported_bound_and_declared(lib):
    from dgvit_amd import _lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    with open(os.path.join(os.path.dirname(L.LIB_PATH), os.pardir, "include", "dgvit_hip.h")) as f:
        header = f.read()
    for name, nargs in zip(NAMES, (9, 9, 15)):
        assert hasattr(raw, name)
        res, args = L.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert name + "(" in header
    assert "q(x) = (uint8) rintf(fminf(fmaxf(x * 255.0f, 0), 255))" in header
    assert "(float)ring[clamp(idx[i], 0, nrows-1)][c] / 255.0f" in header
    assert L.SIGNATURES["dgvit_gather_shift_frames_u8"][1][12] is ctypes.c_ulonglong


def test_abi_version_is_unchanged(lib):
    assert lib.dgvit_abi_version() == 7


def _msg(lib, rc, name, word):
    assert rc == -1, "DGVIT_ERR_ARG"
    msg = lib.dgvit_last_error()
    assert name in msg and word in msg, msg


def _ids(v):
    return None if isinstance(v, bytes) else "-".join(f"{k}={x if not isinstance(x, ctypes.c_void_p) else x.value}" for k, x in v.items())


def _quantize(lib, src=FAKE, src_ld=96, ring=FAKE, n=4, cols=96, row_bytes=96, nrows=16, start=0):
    return lib.dgvit_quantize_rows_u8(src, src_ld, ring, n, cols, row_bytes, nrows, start, None)


@pytest.mark.parametrize("kw, word", [
    (dict(src=None), b"null"),
    (dict(ring=None), b"null"),
    (dict(n=0), b"n=0"),
    (dict(n=-2), b"n=-2"),
    (dict(nrows=0), b"nrows=0"),
    (dict(n=17), b"n=17"),                     # n > nrows
    (dict(cols=0, src_ld=96), b"cols=0"),
    (dict(cols=-4), b"cols=-4"),
    (dict(row_bytes=100), b"row_bytes=100"),   # not a multiple of 16
    (dict(row_bytes=80), b"row_bytes=80"),     # a multiple of 16 below cols
    (dict(src_ld=95), b"src_ld=95"),
    (dict(start=-1), b"start=-1"),
    (dict(start=16), b"start=16"),
    (dict(src=ODD1), b"aligned"),
    (dict(ring=ODD), b"aligned"),
], ids=_ids)
def test_quantize_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _quantize(lib, **kw), b"quantize_rows_u8", word)


def _gather(lib, ring=FAKE, idx=FAKE, out=FAKE, nsel=8, cols=95, row_bytes=96, row_floats=96, nrows=16):
    return lib.dgvit_gather_rows_u8(ring, idx, out, nsel, cols, row_bytes, row_floats, nrows, None)


@pytest.mark.parametrize("kw, word", [
    (dict(ring=None), b"null"),
    (dict(idx=None), b"null"),
    (dict(out=None), b"null"),
    (dict(nsel=0), b"nsel=0"),
    (dict(nsel=-1), b"nsel=-1"),
    (dict(nrows=0), b"nrows=0"),
    (dict(cols=0), b"cols=0"),
    (dict(row_bytes=104), b"row_bytes=104"),
    (dict(row_bytes=80), b"row_bytes=80"),
    (dict(row_floats=98), b"row_floats=98"),   # not a multiple of 4
    (dict(row_floats=92), b"row_floats=92"),   # a multiple of 4 below cols
    (dict(ring=ODD), b"aligned"),
    (dict(out=ODD), b"aligned"),
], ids=_ids)
def test_gather_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _gather(lib, **kw), b"gather_rows_u8", word)


def _shift(lib, ring=FAKE, out=FAKE, nsel=8, H=8, W=12, row_bytes=96, row_floats=96, nrows=16, pad=4, stream_id=0):
    return lib.dgvit_gather_shift_frames_u8(ring, None, out, None, nsel, H, W, row_bytes, row_floats, nrows, pad, stream_id, 1, None, None)


@pytest.mark.parametrize("kw, word", [
    (dict(ring=None), b"null"),
    (dict(out=None), b"null"),
    (dict(nsel=0), b"nsel=0"),
    (dict(nsel=-3), b"nsel=-3"),
    (dict(nsel=1 << 24), b"nsel=16777216"),
    (dict(nrows=0), b"nrows=0"),
    (dict(H=0), b"H=0"),
    (dict(W=-1), b"W=-1"),
    (dict(row_bytes=100), b"row_bytes=100"),
    (dict(row_bytes=80), b"row_bytes=80"),
    (dict(row_floats=98), b"row_floats=98"),
    (dict(row_floats=92), b"row_floats=92"),
    (dict(pad=-1), b"pad=-1"),
    (dict(pad=8), b"pad=8"),                       # pad == H
    (dict(H=12, W=8, pad=8), b"pad=8"),            # pad == W
    (dict(stream_id=-1), b"stream_id=-1"),
    (dict(stream_id=65536), b"stream_id=65536"),
    (dict(ring=ODD), b"aligned"),
    (dict(out=ODD), b"aligned"),
], ids=_ids)
def test_shifted_gather_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _shift(lib, **kw), b"gather_shift_frames_u8", word)


# ------------------------------------------------------------------------------------------------ the Python checks
@pytest.mark.parametrize("bad", [torch.float16, torch.int8, torch.float64, np.uint8, "uint8", None, 8])
def test_bad_frame_dtype_raises_before_the_device_check(bad):
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    for cls in (DeviceReplayBuffer, PrioritizedDeviceReplayBuffer):
        with pytest.raises(ValueError, match="frame_dtype"):
            cls(8, obs_shape=(16, 20), device="cpu", frame_dtype=bad)


def test_frame_dtype_is_keyword_only():
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    with pytest.raises(TypeError):
        DeviceReplayBuffer(8, (16, 20), 2, 2, "cpu", None, torch.uint8)
    with pytest.raises(TypeError):
        PrioritizedDeviceReplayBuffer(8, (16, 20), 2, 2, "cpu", None, 0.6, 1e-4, torch.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_a_cpu_device_is_still_refused(dtype):
    import dgvit_amd
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    for cls in (DeviceReplayBuffer, PrioritizedDeviceReplayBuffer):
        with pytest.raises(dgvit_amd.DgvitError):
            cls(8, obs_shape=(16, 20), device="cpu", frame_dtype=dtype)


# ------------------------------------------------------------------------------------------------ the restatement alone
def test_dequantize_is_torch_and_numpy_division_bit_for_bit():
    k = np.arange(256, dtype=np.uint8)
    d = R.dequantize(k)
    assert d.dtype == np.float32
    want_t = (torch.arange(256, dtype=torch.uint8).float() / 255).numpy()
    want_n = (k / 255).astype(np.float32)                      # the reference: uint8_array / 255 (fp64) -> FloatTensor
    assert np.array_equal(d.view(np.uint32), want_t.view(np.uint32))
    assert np.array_equal(d.view(np.uint32), want_n.view(np.uint32))
    recip = k.astype(np.float32) * (np.float32(1) / np.float32(255))
    assert (recip != d).sum() == 126, "a multiplication by 1/255 is not the division"


def test_the_kernels_newton_step_is_the_division_on_every_code():
    """csrc/replay_ring.hip forms k / 255 as a product with fl(1/255) and one correction in two fused multiply-adds: restated with exact
    rational arithmetic and one rounding per operation, it is the correctly rounded quotient for all 256 codes"""
    assert np.float32(float.fromhex("0x1.010102p-8")) == np.float32(1) / np.float32(255)
    with open(os.path.join(os.path.dirname(__file__), os.pardir, "dgvit-depth-goal-guided-vision-transformer-_amd", "csrc", "replay_ring.hip")) as f:
        assert "0x1.010102p-8f" in f.read()
    got = np.array([R.newton_dequantize(k) for k in range(256)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), R.dequantize(np.arange(256, dtype=np.uint8)).view(np.uint32))
    assert all(R.round_f32(R.Fraction(k, 255)) == got[k] for k in range(256)), "and the quotient itself, rounded once"


def test_quantize_inverts_dequantize_on_every_code():
    k = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.quantize(R.dequantize(k)), k)


def test_quantize_special_values():
    x = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 2.0, -1.0, 1e-9, 1.0 - 2.0 ** -24], dtype=np.float32)
    assert R.quantize(x).tolist() == [0, 0, 255, 0, 0, 0, 255, 255, 0, 0, 255]


def test_tie_inputs_cover_every_half():
    ms, xs = R.tie_inputs()
    assert ms.tolist() == list(range(255)), "an fp32 input whose product with 255 is m + 0.5 exists for every m"
    assert xs.dtype == np.float32 and np.array_equal(xs * np.float32(255), ms.astype(np.float32) + np.float32(0.5))
    even = ms % 2 == 0
    assert even.sum() >= 100
    q = R.quantize(xs)
    assert np.array_equal(q[even], ms[even]), "half to even: m + 0.5 with even m rounds down"
    assert np.array_equal(q[~even], ms[~even] + 1)


def test_round_trip_error_is_inside_the_bound():
    """|dequantize(quantize(x)) - x| <= 1/510 + 2^-23 on 10^6 seeded uniforms plus the ties, evaluated in fp64"""
    x = np.random.default_rng(20260510).random(1_000_000, dtype=np.float32)
    x = np.concatenate([x, R.tie_inputs()[1], np.array([0.0, 1.0], dtype=np.float32)])
    err = np.abs(R.dequantize(R.quantize(x)).astype(np.float64) - x.astype(np.float64))
    assert err.max() <= R.ROUND_TRIP_BOUND, err.max()
    assert err.max() > 1.0 / 512.0, "the ties sit at half a step"


def test_pattern_separates_neighbouring_offsets():
    p = R.pattern([0, 1, 5], 16, 20)
    assert p.dtype == np.uint8 and p.shape == (3, 320) and p.max() <= 250
    assert (p[0] != p[1]).mean() > 0.99
    assert (p[0, :-1] != p[0, 1:]).all() and (p[0, :-20] != p[0, 20:]).mean() > 0.99
