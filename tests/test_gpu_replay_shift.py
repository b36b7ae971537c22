"""GPU: the random-shift gather (dgvit_gather_shift_frames), DeviceReplayBuffer.sample(random_shift=...) and preprocess.random_shift.

References are never the code under test: the shift table is checked against the numpy restatement of the Philox draw
(tests/replay_shift_ref.py) and the pixels against torch's replicate-pad + crop fed the returned shifts -- a copy, so bit-exact.
Source frames hold a distinct value per pixel (arange, exact in fp32 below 2^24), so a wrong offset cannot match by accident."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import replay_shift_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _gather_shift(src, idx, B, H, W, pad, stream_id=0, seed=R.SEED, seed_dev=None):
    """the raw entry point on src (nrows, row): (out (B, row), shifts (B, 2))"""
    from dgvit_amd import _lib as L
    out = torch.full((B, src.shape[1]), float("nan"), device="cuda")
    shifts = torch.full((B, 2), 99, dtype=torch.int32, device="cuda")
    rc = L.load().dgvit_gather_shift_frames(_p(src), _p(idx), _p(out), _p(shifts), B, H, W, src.shape[1], src.shape[0], pad, stream_id,
                                            0 if seed_dev is not None else seed, _p(seed_dev),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    L.check(rc, "dgvit_gather_shift_frames")
    return out, shifts


def _ring(nrows, H, W):
    """(nrows, al4(H*W)) rows of distinct pixel values, padding columns zero (as DeviceReplayBuffer keeps them)"""
    row = (H * W + 3) & ~3
    src = torch.zeros(nrows, row, device="cuda")
    src[:, :H * W] = torch.arange(nrows * H * W, dtype=torch.float32, device="cuda").reshape(nrows, H * W)
    return src


# ------------------------------------------------------------------------------------------------ the shift table
@pytest.mark.parametrize("stream_id", [0, 1])
def test_shift_table_equals_the_restatement(amd, stream_id):
    """B = 4096, pad = 4 on an 8 x 12 frame: the kernel's (dy, dx) are the host restatement's, by value and through seed_dev"""
    B, H, W, pad = 4096, 8, 12, 4
    src = _ring(B, H, W)
    want = R.draw_shifts(B, pad, R.SEED, stream_id)
    _, by_value = _gather_shift(src, None, B, H, W, pad, stream_id)
    np.testing.assert_array_equal(by_value.cpu().numpy(), want)
    seed_dev = torch.tensor([R.SEED], dtype=torch.int64, device="cuda")
    _, by_pointer = _gather_shift(src, None, B, H, W, pad, stream_id, seed_dev=seed_dev)
    np.testing.assert_array_equal(by_pointer.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the pixels
@pytest.mark.parametrize("H, W, pad, B", [
    (8, 12, 4, 64),
    (7, 9, 3, 64),        # H*W = 63: rows padded to 64 floats, float4 groups straddle image rows
    (5, 6, 4, 64),        # pad close to the frame: most pixels clamped
    (128, 160, 4, 33),    # the shipped frame: 20 workgroups per sample
])
def test_pixels_equal_pad_and_crop(amd, H, W, pad, B):
    nrows = 40
    src = _ring(nrows, H, W)
    idx = torch.randint(0, nrows, (B,), device="cuda", generator=torch.Generator("cuda").manual_seed(H * W))
    for stream_id in (0, 1):
        out, shifts = _gather_shift(src, idx, B, H, W, pad, stream_id)
        assert int(shifts.abs().max()) <= pad and int(shifts.abs().max()) > 0
        want = R.ref_shift(src[idx, :H * W].reshape(B, H, W), shifts.cpu(), pad)
        assert torch.equal(out[:, :H * W].reshape(B, H, W), want)
        assert not out[:, H * W:].any(), "padding columns of out must be written as zeros"
    assert not torch.isnan(out).any()


def test_pad_zero_is_gather_rows(amd):
    from dgvit_amd import _lib as L
    H, W, nrows, B = 7, 9, 24, 50
    src = _ring(nrows, H, W)
    idx = torch.randint(0, nrows, (B,), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    out, shifts = _gather_shift(src, idx, B, H, W, 0)
    plain = torch.full_like(out, float("nan"))
    L.check(L.load().dgvit_gather_rows(_p(src), _p(idx), _p(plain), B, src.shape[1], nrows,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "dgvit_gather_rows")
    assert torch.equal(out.view(torch.int32), plain.view(torch.int32))
    assert not shifts.any()


def test_indices_clamp_repeat_and_default_to_the_identity(amd):
    from dgvit_amd import _lib as L
    H, W, pad, nrows = 8, 12, 2, 10
    src = _ring(nrows, H, W)
    idx = torch.tensor([3, 3, -1, nrows, 9, 0, 3, -7, nrows + 5], device="cuda")
    B = idx.numel()
    out, shifts = _gather_shift(src, idx, B, H, W, pad)
    plain = torch.empty_like(out)
    L.check(L.load().dgvit_gather_rows(_p(src), _p(idx), _p(plain), B, src.shape[1], nrows,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "dgvit_gather_rows")
    assert torch.equal(plain, src[idx.clamp(0, nrows - 1)])        # gather_rows clamps; the shifted gather reads the same rows
    assert torch.equal(out.reshape(B, H, W), R.ref_shift(plain.reshape(B, H, W), shifts.cpu(), pad))
    # idx = NULL reads row i, and draws the shifts of samples 0 .. B-1 whatever the rows are
    ident, s2 = _gather_shift(src, None, nrows, H, W, pad)
    assert torch.equal(ident.reshape(nrows, H, W), R.ref_shift(src.reshape(nrows, H, W), s2.cpu(), pad))
    assert torch.equal(s2[:B], shifts)


def test_shifted_gather_from_a_ring_past_2_31_floats(amd):
    """104 960 rows of 128 x 160 frames (2.15e9 floats, 8.6 GB, as test_gpu_large_operands.py takes gather_rows there): the source offset
    `s * row_floats + sy * W + sx` for the rows around element 2^31 and byte offsets 2^31 / 2^32, the last row, and indices that
    clamp.  Only the rows read are filled, row r with (7919 r + c) mod 2^24 (exact in fp32); the rest of the ring is zero."""
    from helpers import GIB, boundary_rows, need_device_memory
    nrows, H, W, pad = 104960, 128, 160, 4
    row = H * W
    need_device_memory(nrows * row * 4 + 2 * GIB)
    idx = np.concatenate([[0, nrows - 1], boundary_rows(nrows, row), [-1, nrows, 1 << 40]]).astype(np.int64)
    assert {104857, 104858} <= set(idx.tolist())
    rows = torch.from_numpy(np.clip(idx, 0, nrows - 1)).cuda()
    src = torch.zeros(nrows, row, device="cuda")
    src[rows] = ((rows[:, None] * 7919 + torch.arange(row, device="cuda")[None, :]) % (1 << 24)).float()
    out, shifts = _gather_shift(src, torch.from_numpy(idx).cuda(), len(idx), H, W, pad)
    want = R.ref_shift(src[rows].reshape(len(idx), H, W), shifts.cpu(), pad)
    assert torch.equal(out.reshape(len(idx), H, W), want)
    del src, out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ DeviceReplayBuffer
def _filled(amd, seed):
    from dgvit_amd.replay import DeviceReplayBuffer
    n, H, W = 64, 16, 20
    buf = DeviceReplayBuffer(n, obs_shape=(H, W), seed=seed)
    g = torch.Generator().manual_seed(5)
    buf.add_batch(obs=torch.arange(n * H * W, dtype=torch.float32).reshape(n, H, W),
                  next_obs=-torch.arange(n * H * W, dtype=torch.float32).reshape(n, H, W) - 1,
                  pobs=torch.randn(n, 2, generator=g), next_pobs=torch.randn(n, 2, generator=g), act=torch.randn(n, 2, generator=g),
                  rew=torch.randn(n, 1, generator=g), done=torch.zeros(n, 1))
    return buf


def _stored(buf, k, idx):
    return buf.store[k][idx, :buf.fields[k]].reshape(idx.numel(), *buf.shapes[k])


def test_buffer_sample_with_random_shift(amd):
    buf = _filled(amd, 3)
    b = buf.sample(32, random_shift=4, return_shifts=True)
    idx = b["indexes"]
    assert b["obs_shift"].shape == (32, 2) and b["obs_shift"].dtype == torch.int32
    for k in ("obs", "next_obs"):
        assert torch.equal(b[k], R.ref_shift(_stored(buf, k, idx), b[k + "_shift"].cpu(), 4))
    assert not torch.equal(b["obs_shift"], b["next_obs_shift"]), "obs and next_obs shift independently"
    for k in ("act", "rew", "pobs", "next_pobs", "done"):
        assert torch.equal(b[k], _stored(buf, k, idx))
    assert set(buf.sample(32, random_shift=4)) == set(buf.sample(32)), "return_shifts=False adds no keys"
    b2 = buf.sample(32, random_shift=4, return_shifts=True)
    assert not torch.equal(b["obs_shift"], b2["obs_shift"]), "every call draws a new seed"


def test_buffer_sample_follows_torch_manual_seed(amd):
    a, c = _filled(amd, 11), _filled(amd, 11)
    torch.manual_seed(1234)
    ba = a.sample(32, random_shift=4, return_shifts=True)
    torch.manual_seed(1234)
    bc = c.sample(32, random_shift=4, return_shifts=True)
    assert set(ba) == set(bc)
    for k in ba:
        assert torch.equal(ba[k], bc[k]), k


def test_random_shift_zero_is_the_plain_sample(amd):
    a, c = _filled(amd, 7), _filled(amd, 7)
    torch.manual_seed(99)
    state = torch.get_rng_state()
    ba, bc = a.sample(32), c.sample(32, random_shift=0)
    assert torch.equal(torch.get_rng_state(), state), "random_shift=0 draws nothing from the CPU generator"
    assert list(ba) == list(bc)
    for k in ba:
        assert torch.equal(ba[k], bc[k]), k
    assert torch.equal(ba["obs"], _stored(a, "obs", ba["indexes"]))


# ------------------------------------------------------------------------------------------------ preprocess.random_shift
def test_preprocess_random_shift(amd):
    frames = torch.arange(3 * 7 * 9, dtype=torch.float32, device="cuda").reshape(3, 7, 9)
    keep = frames.clone()
    out, shifts = amd.preprocess.random_shift(frames, 3, seed=R.SEED, return_shifts=True)
    assert out.shape == frames.shape and out.data_ptr() != frames.data_ptr()
    assert torch.equal(frames, keep), "the input is untouched"
    np.testing.assert_array_equal(shifts.cpu().numpy(), R.draw_shifts(3, 3, R.SEED, 0))
    assert torch.equal(out, R.ref_shift(frames, shifts.cpu(), 3))
    out1 = amd.preprocess.random_shift(frames, 3, seed=R.SEED, stream_id=1)
    assert torch.equal(out1, R.ref_shift(frames, torch.from_numpy(R.draw_shifts(3, 3, R.SEED, 1)), 3))
    # H*W a multiple of 4 (no padded copy), seed drawn from torch's CPU generator
    f2 = torch.arange(4 * 8 * 12, dtype=torch.float32, device="cuda").reshape(4, 8, 12)
    torch.manual_seed(5)
    o2, s2 = amd.preprocess.random_shift(f2, 2, return_shifts=True)
    torch.manual_seed(5)
    o3 = amd.preprocess.random_shift(f2, 2)
    assert torch.equal(o2, R.ref_shift(f2, s2.cpu(), 2)) and torch.equal(o2, o3)


# ------------------------------------------------------------------------------------------------ graph capture
def test_captured_sample_reads_its_seed_from_the_device(amd):
    """sample(random_shift=2) captured on a side stream as runtime.GraphedStep does: the seed is a device tensor the graph draws
    (random_() is part of the capture), so each replay has its own shifts and satisfies the restatement with them"""
    buf = _filled(amd, 2)
    fixed = torch.tensor([5, 63, 0, 17, 17, 40, 8, 31], device="cuda")

    def step():
        return buf.sample(8, indices=fixed, random_shift=2, return_shifts=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert isinstance(buf.shift_seed, int), "outside a capture the seed is a host value"
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    seed_t = buf.shift_seed
    assert isinstance(seed_t, torch.Tensor) and seed_t.dtype == torch.int64 and seed_t.numel() == 1 and seed_t.is_cuda
    tables = []
    for _ in range(2):
        seed_t.random_()          # refilled between replays (the captured random_() of the graph-safe generator redraws it as well)
        graph.replay()
        torch.cuda.synchronize()
        for k in ("obs", "next_obs"):
            assert torch.equal(static[k], R.ref_shift(_stored(buf, k, fixed), static[k + "_shift"].cpu(), 2))
            want = R.draw_shifts(8, 2, int(seed_t.item()) & (2 ** 64 - 1), int(k == "next_obs"))
            np.testing.assert_array_equal(static[k + "_shift"].cpu().numpy(), want)
        assert torch.equal(static["act"], _stored(buf, "act", fixed))
        tables.append(torch.cat([static["obs_shift"], static["next_obs_shift"]]).clone())
    assert not torch.equal(tables[0], tables[1])
