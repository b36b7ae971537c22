"""GPU: the uint8 replay ring -- dgvit_quantize_rows_u8, dgvit_gather_rows_u8, dgvit_gather_shift_frames_u8 and the buffers built with
frame_dtype=torch.uint8.

Every comparison is torch.equal / array_equal against the host restatement (tests/replay_u8_ref.py, tests/replay_shift_ref.py) or a
torch expression evaluated on the CPU, never against the code under test.  Frames hold the codes of replay_u8_ref.pattern: bytes cannot
carry a distinct value per pixel, and its prime modulus makes a wrong offset mismatch almost everywhere."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import replay_shift_ref as RS  # noqa: E402
import replay_u8_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _al4(n):
    return (n + 3) & ~3


def _al16(n):
    return (n + 15) & ~15


def _quantize(src, ring, n, cols, start):
    """the raw entry point: src (n, src_ld) fp32 on the device -> ring rows start .. (mod nrows)"""
    from dgvit_amd import _lib as L
    rc = L.load().dgvit_quantize_rows_u8(_p(src), src.stride(0), _p(ring), n, cols, ring.shape[1], ring.shape[0], start, _st())
    L.check(rc, "dgvit_quantize_rows_u8")


def _gather(ring, idx, cols):
    """the raw entry point on ring (nrows, row_bytes): out (B, al4(cols)), pre-filled with NaN"""
    from dgvit_amd import _lib as L
    B = idx.numel()
    out = torch.full((B, _al4(cols)), float("nan"), device="cuda")
    rc = L.load().dgvit_gather_rows_u8(_p(ring), _p(idx), _p(out), B, cols, ring.shape[1], out.shape[1], ring.shape[0], _st())
    L.check(rc, "dgvit_gather_rows_u8")
    return out


def _shift(ring, idx, B, H, W, pad, stream_id=0, seed=RS.SEED):
    """the raw entry point: (out (B, al4(H*W)) pre-filled with NaN, shifts (B, 2) pre-filled with 99)"""
    from dgvit_amd import _lib as L
    out = torch.full((B, _al4(H * W)), float("nan"), device="cuda")
    shifts = torch.full((B, 2), 99, dtype=torch.int32, device="cuda")
    rc = L.load().dgvit_gather_shift_frames_u8(_p(ring), _p(idx), _p(out), _p(shifts), B, H, W, ring.shape[1], out.shape[1], ring.shape[0],
                                               pad, stream_id, seed, None, _st())
    L.check(rc, "dgvit_gather_shift_frames_u8")
    return out, shifts


def _ring(codes, fill=0xFF):
    """(nrows, al16(cols)) uint8 device ring holding `codes` (nrows, cols); the padding bytes hold `fill`, which no gather may show"""
    nrows, cols = codes.shape
    ring = torch.full((nrows, _al16(cols)), fill, dtype=torch.uint8, device="cuda")
    ring[:, :cols] = torch.from_numpy(codes).cuda()
    return ring


def _deq(codes):
    """torch's own uint8 -> float / 255 on the CPU"""
    return torch.from_numpy(np.ascontiguousarray(codes)).float() / 255


# ------------------------------------------------------------------------------------------------ the quantiser
@pytest.fixture(scope="module")
def quantize_inputs():
    """all j / 65536, the ties, 2^16 normals that spill past [0, 1], the special values; and their codes by the restatement"""
    rng = np.random.default_rng(8)
    x = np.concatenate([np.arange(65537, dtype=np.float32) / np.float32(65536), R.tie_inputs()[1],
                        (0.5 + 0.75 * rng.standard_normal(65536)).astype(np.float32),
                        np.array([np.inf, -np.inf, np.nan, -0.0], dtype=np.float32)])
    want = R.quantize(x)
    assert want[-4:].tolist() == [255, 0, 0, 0] and (want == 0).sum() > 1000 and (want == 255).sum() > 1000
    return x, want


@pytest.mark.parametrize("extra", [0, 5, 8])       # src_ld - cols: rows of the source 16-byte aligned or not, src_ld > cols
@pytest.mark.parametrize("cols", [35, 320, 20480])  # 5 x 7 (W % 4 != 0, H*W % 16 != 0), 16 x 20, 128 x 160
def test_quantize_equals_the_restatement(amd, quantize_inputs, cols, extra):
    x, want = quantize_inputs
    n = -(-x.size // cols)
    xs, ws = np.zeros((n, cols + extra), np.float32), np.zeros((n, cols), np.uint8)
    xs[:, cols:] = 0.5                                  # columns of the source behind `cols` must not reach the ring
    xs[:, :cols].flat[:x.size] = x
    ws.flat[:x.size] = want
    src = torch.from_numpy(xs).cuda()
    row_bytes = _al16(cols)
    for nrows, start in ((n + 3, n + 1), (n, n // 2)):      # start + n wraps the ring; n == nrows
        ring = torch.full((nrows, row_bytes), 0xFF, dtype=torch.uint8, device="cuda")
        _quantize(src, ring, n, cols, start)
        expect = np.full((nrows, row_bytes), 0xFF, np.uint8)
        rows = (start + np.arange(n)) % nrows
        expect[rows, :cols] = ws
        expect[rows, cols:] = 0                             # the padding bytes of a written row are zeros
        assert np.array_equal(ring.cpu().numpy(), expect)


# ------------------------------------------------------------------------------------------------ the plain gather
@pytest.mark.parametrize("B", [1, 3, 37])
@pytest.mark.parametrize("H, W", [(5, 7), (16, 20), (128, 160)])
def test_gather_equals_torch_division(amd, H, W, B):
    nrows, cols = 24, H * W
    codes = np.random.default_rng(H).integers(0, 256, (nrows, cols), dtype=np.uint8)
    codes[0, :35] = np.arange(35)
    codes[1:9].flat[:256] = np.arange(256)                  # every code occurs
    ring = _ring(codes)
    pool = [1, -1, nrows, 1 << 40, 1, 1, 0, nrows - 1, -(1 << 40)] + np.random.default_rng(B).integers(0, nrows, 28).tolist()
    idx = torch.tensor(pool[:B], dtype=torch.int64, device="cuda")
    out = _gather(ring, idx, cols).cpu()
    want = _deq(codes)[idx.cpu().clamp(0, nrows - 1)]
    assert torch.equal(out[:, :cols], want)         # (finite and non-negative: equal values are equal bits)
    assert out.shape[1] == _al4(cols) and not out[:, cols:].any(), "padding floats are zeros, whatever the ring holds there"


# ------------------------------------------------------------------------------------------------ the shifted gather
@pytest.mark.parametrize("H, W, pad, B", [
    (8, 12, 4, 64),
    (7, 9, 3, 64),        # H*W = 63: float4 groups straddle image rows
    (5, 6, 4, 64),        # pad close to the frame: most pixels clamped
    (128, 160, 4, 33),    # the shipped frame
])
def test_shifted_pixels_equal_pad_and_crop(amd, H, W, pad, B):
    from dgvit_amd import _lib as L
    nrows, cols = 40, H * W
    codes = R.pattern(range(nrows), H, W)
    ring = _ring(codes)
    frames = _deq(codes)
    ring32 = torch.zeros(nrows, _al4(cols), device="cuda")      # the fp32 ring holding the same k / 255 frames
    ring32[:, :cols] = frames.cuda()
    idx = torch.randint(0, nrows, (B,), device="cuda", generator=torch.Generator("cuda").manual_seed(H * W))
    for stream_id in (0, 1):
        out, shifts = _shift(ring, idx, B, H, W, pad, stream_id)
        np.testing.assert_array_equal(shifts.cpu().numpy(), RS.draw_shifts(B, pad, RS.SEED, stream_id))
        want = RS.ref_shift(frames[idx.cpu()].reshape(B, H, W), shifts.cpu(), pad)
        assert torch.equal(out.cpu()[:, :cols].reshape(B, H, W), want)
        assert not out[:, cols:].any(), "padding columns of out must be written as zeros"
        out32 = torch.full_like(out, float("nan"))
        rc = L.load().dgvit_gather_shift_frames(_p(ring32), _p(idx), _p(out32), None, B, H, W, out32.shape[1], nrows, pad, stream_id, RS.SEED,
                                                None, _st())
        L.check(rc, "dgvit_gather_shift_frames")
        assert torch.equal(out.view(torch.int32), out32.view(torch.int32)), "the fp32 kernel on the same k / 255 frames"


def test_pad_zero_is_the_plain_gather_and_null_idx_the_identity(amd):
    H, W, nrows, B = 7, 9, 24, 50
    codes = R.pattern(range(nrows), H, W)
    ring = _ring(codes)
    idx = torch.randint(0, nrows, (B,), device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    idx[:4] = torch.tensor([-1, nrows, 1 << 40, -7], device="cuda")
    out, shifts = _shift(ring, idx, B, H, W, 0)
    assert torch.equal(out.view(torch.int32), _gather(ring, idx, H * W).view(torch.int32))
    assert not shifts.any()
    # idx = NULL reads row i and draws the shifts of samples 0 .. nrows-1
    ident, s2 = _shift(ring, None, nrows, H, W, 2)
    np.testing.assert_array_equal(s2.cpu().numpy(), RS.draw_shifts(nrows, 2, RS.SEED, 0))
    assert torch.equal(ident.cpu()[:, :H * W].reshape(nrows, H, W), RS.ref_shift(_deq(codes).reshape(nrows, H, W), s2.cpu(), 2))
    # clamped indices read rows 0 and nrows-1 under the shift as well
    out2, s3 = _shift(ring, idx, B, H, W, 2)
    rows = idx.cpu().clamp(0, nrows - 1)
    assert torch.equal(out2.cpu()[:, :H * W].reshape(B, H, W), RS.ref_shift(_deq(codes)[rows].reshape(B, H, W), s3.cpu(), 2))


# ------------------------------------------------------------------------------------------------ byte offsets past 2^31 and 2^32
def test_ring_past_2_32_bytes(amd):
    """209 920 rows of 128 x 160 byte frames (4.3 GB): the offset `s * row_bytes + ...` for the rows around byte 2^31 and byte 2^32, row 0,
    the last row and indices that clamp, through the plain gather, the shifted gather and a quantise that writes rows on both sides of
    each boundary.  Only the rows read are filled; the rest of the ring is zero."""
    from helpers import GIB, boundary_rows, need_device_memory
    nrows, H, W, pad = 209920, 128, 160, 4
    cols = H * W
    need_device_memory(nrows * cols + 2 * GIB)
    near = boundary_rows(nrows, cols, itemsize=1)
    assert {104857, 104858, 209715, 209716} <= set(near)
    idx = np.concatenate([[0, nrows - 1], near, [-1, nrows, 1 << 40]]).astype(np.int64)
    rows = np.clip(idx, 0, nrows - 1)
    ring = torch.zeros(nrows, cols, dtype=torch.uint8, device="cuda")
    codes = R.pattern(rows, H, W)
    ring[torch.from_numpy(rows).cuda()] = torch.from_numpy(codes).cuda()
    idx_d, n = torch.from_numpy(idx).cuda(), len(idx)
    frames = _deq(codes)
    assert torch.equal(_gather(ring, idx_d, cols).cpu(), frames)
    out, shifts = _shift(ring, idx_d, n, H, W, pad)
    np.testing.assert_array_equal(shifts.cpu().numpy(), RS.draw_shifts(n, pad, RS.SEED, 0))
    assert torch.equal(out.cpu().reshape(n, H, W), RS.ref_shift(frames.reshape(n, H, W), shifts.cpu(), pad))
    # the quantiser: four rows across each boundary take new codes; the rows before and behind them keep theirs
    near = np.array(near)
    for group in np.split(near, np.flatnonzero(np.diff(near) > 1) + 1):
        assert len(group) == 4 and any(group[0] * cols < b < (group[-1] + 1) * cols for b in (1 << 31, 1 << 32)), "rows on both sides"
        new = R.pattern(group + 7, H, W)
        _quantize(_deq(new).cuda(), ring, 4, cols, int(group[0]))
        around = np.concatenate([[group[0] - 1], group, [group[-1] + 1]])
        got = ring[torch.from_numpy(around).cuda()].cpu().numpy()
        assert np.array_equal(got[1:5], new)
        assert not got[0].any() and not got[5].any()
    del ring, out
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ DeviceReplayBuffer
N, H, W = 64, 16, 20


def _transitions(n, seed, exact=False):
    """n transitions on the host: float frames that spill past [0, 1] and include ties (exact: k / 255 frames), seeded small fields"""
    g = np.random.default_rng(seed)
    if exact:
        obs, nxt = (R.dequantize(g.integers(0, 256, (n, H, W), dtype=np.uint8)) for _ in range(2))
    else:
        obs, nxt = ((0.5 + 0.5 * g.standard_normal((n, H, W))).astype(np.float32) for _ in range(2))
        ties = R.tie_inputs()[1]
        obs.reshape(-1)[:ties.size] = ties
    f = lambda *s: g.standard_normal(s).astype(np.float32)      # noqa: E731
    return dict(obs=obs, next_obs=nxt, pobs=f(n, 2), next_pobs=f(n, 2), act=f(n, 2), rew=f(n, 1), done=(g.random((n, 1)) < 0.1).astype(np.float32))


def _as(kind, frames):
    """a float frame batch in the form one add path takes"""
    return {"host_float": lambda: frames, "host_u8": lambda: R.quantize(frames), "host_u8_tensor": lambda: torch.from_numpy(R.quantize(frames)),
            "device_float": lambda: torch.from_numpy(frames).cuda(), "device_u8": lambda: torch.from_numpy(R.quantize(frames)).cuda()}[kind]()


def _codes(buf, k):
    return buf.store[k][:, :buf.fields[k]].cpu().numpy().reshape(buf.size, *buf.shapes[k])


SMALL = ("pobs", "next_pobs", "act", "rew", "done")


@pytest.mark.parametrize("obs_kind, next_kind", [("host_float", "host_float"), ("host_u8", "host_u8"), ("device_float", "device_float"),
                                                 ("device_u8", "device_u8"), ("host_u8_tensor", "device_float"), ("host_float", "device_u8"),
                                                 ("device_float", "host_u8")])
def test_every_add_path_stores_the_restated_codes(amd, obs_kind, next_kind):
    from dgvit_amd.replay import DeviceReplayBuffer
    t = _transitions(N, 3)
    buf = DeviceReplayBuffer(N, obs_shape=(H, W), seed=0, frame_dtype=torch.uint8)
    ref = DeviceReplayBuffer(N, obs_shape=(H, W), seed=0)
    assert buf.store["obs"].dtype == torch.uint8 and tuple(buf.store["next_obs"].shape) == (N, _al16(H * W))
    buf.add_batch(**{**t, "obs": _as(obs_kind, t["obs"]), "next_obs": _as(next_kind, t["next_obs"])})
    ref.add_batch(**t)
    assert buf.get_stored_size() == N and buf.next_index == ref.next_index == 0
    assert np.array_equal(_codes(buf, "obs"), R.quantize(t["obs"]))
    assert np.array_equal(_codes(buf, "next_obs"), R.quantize(t["next_obs"]))
    for k in SMALL:
        assert buf.store[k].dtype == torch.float32 and torch.equal(buf.store[k], ref.store[k]), k


@pytest.mark.parametrize("kind", ["host_float", "host_u8", "device_float", "device_u8"])
def test_add_across_the_wrap_and_add_batch_beyond_the_size(amd, kind):
    from dgvit_amd.replay import DeviceReplayBuffer
    buf = DeviceReplayBuffer(N, obs_shape=(H, W), seed=0, frame_dtype=torch.uint8)
    ref = DeviceReplayBuffer(N, obs_shape=(H, W), seed=0)
    t = _transitions(N - 4, 4)
    expect = {k: np.zeros((N, H, W), np.uint8) for k in ("obs", "next_obs")}

    def feed(t, single):
        fed = {**t, "obs": _as(kind, t["obs"]), "next_obs": _as(kind, t["next_obs"])}
        if single:
            for j in range(len(t["obs"])):
                buf.add(**{k: v[j] for k, v in fed.items()})
                ref.add(**{k: v[j] for k, v in t.items()})
        else:
            buf.add_batch(**fed)
            ref.add_batch(**t)

    feed(t, False)                                   # slots 0 .. 59
    for k in expect:
        expect[k][:N - 4] = R.quantize(t[k])
    one = _transitions(8, 5)
    feed(one, True)                                  # one by one: slots 60 .. 63, 0 .. 3
    for k in expect:
        expect[k][(N - 4 + np.arange(8)) % N] = R.quantize(one[k])
    assert buf.next_index == ref.next_index == 4 and buf.stored == ref.stored == N
    for k in expect:
        assert np.array_equal(_codes(buf, k), expect[k]), k
    wrap = _transitions(10, 6)
    buf.next_index = ref.next_index = N - 3
    feed(wrap, False)                                # one batch across the wrap: slots 61 .. 63, 0 .. 6
    for k in expect:
        expect[k][(N - 3 + np.arange(10)) % N] = R.quantize(wrap[k])
        assert np.array_equal(_codes(buf, k), expect[k]), k
    big = _transitions(N + 36, 7)
    feed(big, False)                                 # n > size: the last 64 stay, from slot 7 on
    assert buf.next_index == ref.next_index == 7 and buf.stored == N
    for k in expect:
        expect[k][(7 + np.arange(N)) % N] = R.quantize(big[k][-N:])
        assert np.array_equal(_codes(buf, k), expect[k]), k
    for k in SMALL:
        assert torch.equal(buf.store[k], ref.store[k]), k


def _pair(seed, exact):
    from dgvit_amd.replay import DeviceReplayBuffer
    t = _transitions(N, 9, exact=exact)
    buf = DeviceReplayBuffer(N, obs_shape=(H, W), seed=seed, frame_dtype=torch.uint8)
    ref = DeviceReplayBuffer(N, obs_shape=(H, W), seed=seed)
    buf.add_batch(**t)
    ref.add_batch(**t)
    return t, buf, ref


def test_sample_returns_the_dequantised_frames(amd):
    t, buf, ref = _pair(1, exact=False)
    idx = torch.tensor([5, 63, 0, 17, 17, 40, -1, N, 1 << 40], device="cuda")
    b, r = buf.sample(0, indices=idx), ref.sample(0, indices=idx)
    rows = idx.cpu().clamp(0, N - 1)
    assert list(b) == list(r)
    for k in ("obs", "next_obs"):
        assert b[k].dtype == torch.float32 and tuple(b[k].shape) == (idx.numel(), H, W)
        assert torch.equal(b[k].cpu(), _deq(R.quantize(t[k]))[rows]), k
    for k in SMALL + ("indexes",):
        assert torch.equal(b[k], r[k]), k
    drawn = buf.sample(32)
    assert torch.equal(drawn["obs"].cpu(), _deq(R.quantize(t["obs"]))[drawn["indexes"].cpu()])


def test_sample_follows_the_fp32_buffer_under_one_seed(amd):
    """the same torch.manual_seed and buffer seed: the same indexes and shift tables as the fp32 ring, and, the stored frames being k / 255,
    the same frames bit for bit"""
    t, buf, ref = _pair(11, exact=True)
    assert torch.equal(_deq(_codes(buf, "obs")), torch.from_numpy(t["obs"])), "k / 255 frames are stored exactly"
    torch.manual_seed(1234)
    b = buf.sample(32, random_shift=4, return_shifts=True)
    torch.manual_seed(1234)
    r = ref.sample(32, random_shift=4, return_shifts=True)
    assert list(b) == list(r) and int(b["obs_shift"].abs().max()) > 0
    for k in b:
        assert torch.equal(b[k], r[k]), k
    for k in ("obs", "next_obs"):
        want = RS.ref_shift(torch.from_numpy(t[k])[b["indexes"].cpu()], b[k + "_shift"].cpu(), 4)
        assert torch.equal(b[k].cpu(), want), k
    np.testing.assert_array_equal(b["obs_shift"].cpu().numpy(), RS.draw_shifts(32, 4, buf.shift_seed, 0))
    np.testing.assert_array_equal(b["next_obs_shift"].cpu().numpy(), RS.draw_shifts(32, 4, buf.shift_seed, 1))
    z = buf.sample(8, return_shifts=True)
    assert not z["obs_shift"].any() and not z["next_obs_shift"].any()


def test_default_buffer_is_the_fp32_ring(amd):
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    t = _transitions(N, 12)
    for cls in (DeviceReplayBuffer, PrioritizedDeviceReplayBuffer):
        buf = cls(N, obs_shape=(H, W), seed=2)
        assert buf.frame_dtype is torch.float32
        assert all(v.dtype == torch.float32 for v in buf.store.values())
        assert tuple(buf.store["obs"].shape) == (N, H * W)
        buf.add_batch(**t)
        assert torch.equal(buf.store["obs"].cpu(), torch.from_numpy(t["obs"]).reshape(N, -1)), "floats are stored as given, not quantised"
        b = buf.sample(16)
        assert torch.equal(b["obs"], buf.store["obs"][b["indexes"]].reshape(16, H, W))
        assert torch.equal(b["next_obs"].cpu(), torch.from_numpy(t["next_obs"])[b["indexes"].cpu()])


# ------------------------------------------------------------------------------------------------ PrioritizedDeviceReplayBuffer
def _per():
    from dgvit_amd.replay import PrioritizedDeviceReplayBuffer
    return PrioritizedDeviceReplayBuffer(N, obs_shape=(H, W), seed=4, alpha=1.0, eps=0.0, frame_dtype=torch.uint8)


def test_prioritized_fresh_slots_take_the_max_priority_on_every_add_path(amd):
    buf = _per()
    t = _transitions(N, 13)
    buf.add_batch(**t)
    assert buf.store["obs"].dtype == torch.uint8 and torch.equal(buf.priorities(), torch.ones(N, device="cuda"))
    everything = torch.arange(N, device="cuda")
    want = np.full(N, 0.25, np.float32)
    pos = 0
    for kind in ("host_float", "host_u8", "device_float", "device_u8"):
        buf.update_priorities(everything, torch.full((N,), 0.25, device="cuda"))
        want[:] = 0.25
        new = _transitions(8, 14 + pos)
        buf.add_batch(**{**new, "obs": _as(kind, new["obs"]), "next_obs": _as(kind, new["next_obs"])})       # slots pos .. pos + 7
        buf.add(**{k: v[0] for k, v in {**new, "obs": _as(kind, new["obs"]), "next_obs": _as(kind, new["next_obs"])}.items()})
        want[pos:pos + 9] = 1.0
        pos += 9
        assert buf.next_index == pos
        np.testing.assert_array_equal(buf.priorities().cpu().numpy(), want)
        assert np.array_equal(_codes(buf, "obs")[pos - 9:pos - 1], R.quantize(new["obs"]))
    buf.update_priorities(everything, torch.full((N,), 0.25, device="cuda"))
    buf.next_index = N - 5
    new = _transitions(12, 30)
    buf.add_batch(**{**new, "obs": _as("device_float", new["obs"])})         # across the wrap: slots 59 .. 63, 0 .. 6
    want[:] = 0.25
    want[(N - 5 + np.arange(12)) % N] = 1.0
    np.testing.assert_array_equal(buf.priorities().cpu().numpy(), want)
    assert float(buf.max_priority) == 1.0 and float(buf.min_priority) == 0.25


def test_prioritized_sample_adds_weights(amd):
    buf = _per()
    t = _transitions(N, 15)
    buf.add_batch(**t)
    b = buf.sample(16, beta=1.0, random_shift=2, return_shifts=True)
    assert tuple(b["weights"].shape) == (16, 1) and torch.equal(b["weights"], torch.ones(16, 1, device="cuda"))
    idx = b["indexes"].cpu()
    for k in ("obs", "next_obs"):
        assert torch.equal(b[k].cpu(), RS.ref_shift(_deq(R.quantize(t[k]))[idx], b[k + "_shift"].cpu(), 2)), k
    assert torch.equal(b["act"].cpu(), torch.from_numpy(t["act"])[idx])


def test_prioritized_sample_and_update_in_one_captured_graph(amd):
    """uniforms.uniform_(), sample(random_shift=2) and update_priorities captured in one graph and replayed twice: each replay's frames are
    the stored frames at the drawn indices (an eager sample(indices=...) outside the graph) with the returned shifts applied by the
    restatement, and the priorities written back are at the drawn indices"""
    from dgvit_amd.replay import DeviceReplayBuffer
    B = 16
    buf = _per()
    t = _transitions(N, 16)
    buf.add_batch(**t)
    u = torch.zeros(B, device="cuda")
    pr = torch.full((B,), 3.0, device="cuda")

    def step():
        u.uniform_()
        b = buf.sample(B, beta=0.5, uniforms=u, random_shift=2, return_shifts=True)
        buf.update_priorities(b["indexes"], pr)
        return b
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    drawn = []
    for _ in range(2):
        buf.update_priorities(torch.arange(N, device="cuda"), torch.ones(N, device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        idx = static["indexes"].clone()
        eager = DeviceReplayBuffer.sample(buf, B, indices=idx)
        for k in ("obs", "next_obs"):
            assert torch.equal(eager[k].cpu(), _deq(R.quantize(t[k]))[idx.cpu()]), k
            assert torch.equal(static[k].cpu(), RS.ref_shift(eager[k].cpu(), static[k + "_shift"].cpu(), 2)), k
            want = RS.draw_shifts(B, 2, int(buf.shift_seed.item()) & (2 ** 64 - 1), int(k == "next_obs"))
            np.testing.assert_array_equal(static[k + "_shift"].cpu().numpy(), want)
        assert torch.equal(static["rew"], eager["rew"])
        leaves = np.ones(N, np.float32)
        leaves[idx.cpu().numpy()] = 3.0
        np.testing.assert_array_equal(buf.priorities().cpu().numpy(), leaves)
        drawn.append(torch.cat([idx, static["obs_shift"].reshape(-1).long()]))
    assert not torch.equal(drawn[0], drawn[1])


def test_both_rings_hold_the_same_transitions_after_the_same_adds(amd):
    """An fp32 and a uint8 ring, and a prioritized twin of each, fed the same k / 255 transitions through the one store path: 5 single
    adds, an add_batch of 16 that wraps, an add_batch of 21 > size.  The frame fields rotate through the four forms a uint8 ring takes
    (the fp32 ring gets the same frames as floats, on the host or on the device).  After every step the two rings agree in next_index,
    stored, every non-frame field and every field of sample(indices = all slots), bit for bit; the slots just written hold the frames
    given and, in the prioritized twins, the max priority.  (12, 10) frames: W % 4 != 0, and row_bytes = al16(120) = 128 leaves 8 padding
    bytes per ring row (the fp32 row is al4(120) = 120 floats)."""
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    S, h, w = 16, 12, 10
    pairs = [tuple(cls(S, obs_shape=(h, w), seed=0, frame_dtype=dt, **kw) for dt in (torch.float32, torch.uint8))
             for cls, kw in ((DeviceReplayBuffer, {}), (PrioritizedDeviceReplayBuffer, dict(alpha=1.0, eps=0.0)))]
    g = np.random.default_rng(21)
    every = torch.arange(S, device="cuda")
    frames = ("obs", "next_obs")
    forms = ("host_float", "host_u8", "device_float", "device_u8")
    f = lambda *s: g.standard_normal(s).astype(np.float32)      # noqa: E731
    pos = total = 0
    for step, n in enumerate([1, 1, 1, 1, 1, 16, 21]):
        codes = {k: g.integers(0, 256, (n, h, w), dtype=np.uint8) for k in frames}
        exact = {k: R.dequantize(codes[k]) for k in frames}
        t = dict(pobs=f(n, 2), next_pobs=f(n, 2), act=f(n, 2), rew=f(n, 1), done=(g.random((n, 1)) < 0.5).astype(np.float32))
        form = {k: forms[(step + j) % 4] for j, k in enumerate(frames)}
        to_u8 = {k: {"host_float": exact[k], "host_u8": codes[k], "device_float": torch.from_numpy(exact[k]).cuda(),
                     "device_u8": torch.from_numpy(codes[k]).cuda()}[form[k]] for k in frames}
        to_f32 = {k: torch.from_numpy(exact[k]).cuda() if form[k].startswith("device") else exact[k] for k in frames}
        kept = min(n, S)
        slots = torch.from_numpy((pos + np.arange(kept)) % S)
        for f32, u8 in pairs:
            for buf, fr in ((f32, to_f32), (u8, to_u8)):
                if hasattr(buf, "tree") and buf.stored:
                    buf.update_priorities(every, torch.full((S,), 0.25, device="cuda"))
                if n == 1:
                    buf.add(**{k: v[0] for k, v in {**t, **fr}.items()})
                else:
                    buf.add_batch(**t, **fr)
            assert f32.next_index == u8.next_index == (pos + kept) % S, (step, form)
            assert f32.stored == u8.stored == min(total + n, S), (step, form)
            for k in SMALL:
                assert torch.equal(f32.store[k], u8.store[k]), (step, k)
            a, b = (DeviceReplayBuffer.sample(buf, S, indices=every) for buf in (f32, u8))
            assert list(a) == list(b)
            for k in a:
                assert torch.equal(a[k], b[k]), (step, form, k)
            for k in frames:
                assert torch.equal(b[k].cpu()[slots], torch.from_numpy(exact[k][-kept:])), (step, form, k)
                assert u8.store[k].shape[1] == 128 and not u8.store[k][:, h * w:].any(), (step, form, k)
                assert not f32.store[k][:, h * w:].any(), (step, form, k)
            for k in SMALL:
                assert torch.equal(b[k].cpu()[slots], torch.from_numpy(t[k][-kept:])), (step, k)
            if hasattr(f32, "tree"):
                assert torch.equal(f32.priorities(), u8.priorities()), (step, form)
                assert float(f32.max_priority) == float(u8.max_priority) == 1.0
                assert torch.equal(u8.priorities().cpu()[slots], torch.ones(kept)), (step, form)
                if total and kept < S:
                    assert float(u8.min_priority) == 0.25, "slots not written keep the priority they had"
        pos, total = (pos + kept) % S, total + n
