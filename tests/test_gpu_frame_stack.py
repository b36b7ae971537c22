"""GPU: frame stacks from the replay ring and on the acting side -- sample(..., frame_stack=K) through
dgvit_ring_stack_rows, dgvit_gather_stack_frames and dgvit_gather_shift_stack_frames, and replay.FrameStack through
dgvit_frame_stack_push.

The reference is tests/frame_stack_ref.py, which tests/test_frame_stack_host.py checks against every environment's own stream: a ring
model driven by the same add_vec stream, a frame being one integer id that shared_next_ref.pixels turns into a k / 255 frame.  Every
comparison is bit-exact: the stacks are copies (uint8: code / 255).  Frames are 6 x 10 (W % 4 != 0: float4 groups straddle image rows)
and 5 x 7 (H W and H W K are no multiples of 4: padding columns).  The streams have episodes of 1, 2, 5 and 3 steps that end by END, by
done != 0 without END, or by both; every slot is sampled, with the ring partly filled, exactly full and wrapped."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import frame_stack_ref as R  # noqa: E402
import shared_next_ref as S  # noqa: E402

FIELDS = ("obs", "pobs", "act", "rew", "next_obs", "next_pobs", "done")
FRAMES = ("obs", "next_obs")
SHAPES = [(6, 10), (5, 7)]
DTYPES = [torch.float32, torch.uint8]
KS = (1, 2, 3, 4, 5, 16)
RINGS = [(1, 24), (3, 36), (3, 3)]          # (E, size); the last is a ring shorter than K steps per lane
KINDS = ("two", "shared", "small_pool")     # small_pool: terminal_frames = 1, so that the lost-frame fallback is hit
LENGTHS = (1, 2, 5, 3)
HOW = ("end", "done", "both")


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


def _streams(E, T):
    """E streams of (rew, done, end): episode lengths cycle through 1, 2, 5, 3 from a different start per environment, ends cycle through
    END alone, done != 0 alone (no END) and both"""
    out = []
    for e in range(E):
        stream, j = [], e
        while len(stream) < T:
            length, how = LENGTHS[j % 4], HOW[(j + e) % 3]
            for i in range(length):
                last = i == length - 1
                stream.append((np.float32((len(stream) % 9 - 4) / 8.0), np.float32(1.0 if last and how != "end" else 0.0),
                               bool(last and how != "done")))
            j += 1
        out.append(stream[:T])
    return out


@functools.lru_cache(maxsize=None)
def _world(E, T, shape):
    """(streams, frame ids, data[k][t, e]), computed once per shape and left unchanged"""
    strs = _streams(E, T)
    frs = S.all_frames(strs)
    g = np.random.default_rng(100 * E + T)
    d = {"codes": {}}
    for j, k in enumerate(FRAMES):
        d["codes"][k] = np.stack([np.stack([S.pixels(frs[e][t][j], shape, codes=True) for e in range(E)]) for t in range(T)])
        d[k] = d["codes"][k].astype(np.float32) / np.float32(255.0)
    d.update({k: g.standard_normal((T, E, 2)).astype(np.float32) for k in ("pobs", "next_pobs", "act")})
    d["rew"] = np.array([[[s[t][0]] for s in strs] for t in range(T)], np.float32)
    d["done"] = np.array([[[s[t][1]] for s in strs] for t in range(T)], np.float32)
    d["end"] = np.array([[s[t][2] for s in strs] for t in range(T)], bool)
    return strs, frs, d


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _step(d, t):
    return {k: _dev(d[k][t]) for k in FIELDS}


def _buffer(kind, E, size, shape, dtype, cls=None):
    from dgvit_amd.replay import DeviceReplayBuffer
    kw = dict(obs_shape=shape, seed=3, frame_dtype=dtype, num_envs=E)
    if kind != "two":
        kw.update(shared_next_obs=True, terminal_frames=1 if kind == "small_pool" else None)
    return (cls or DeviceReplayBuffer)(size, **kw)


class Twin:
    """a buffer and its numpy models, driven together"""

    def __init__(self, kind, E, size, shape, dtype, cls=None, tracked=True):
        self.kind, self.shape, self.E, self.size = kind, shape, E, size
        self.buf = _buffer(kind, E, size, shape, dtype, cls)
        self.ring = R.StackRing(E, size, tracked=tracked or kind != "two")
        self.shared = None if kind == "two" else S.SharedRing(E, size, 1 if kind == "small_pool" else None)

    def add(self, strs, frs, d, t, ends=True):
        if ends:
            self.buf.add_vec(**_step(d, t), episode_end=_dev(d["end"][t]) if t % 2 else d["end"][t])
        else:
            self.buf.add_vec(**_step(d, t))
        self.ring.add_vec_frames(strs, frs, t, ends=ends)
        if self.shared is not None:
            self.shared.add_vec_frames(strs, frs, t)

    def want(self, idx, K, n_step=None, shifts=None, full=None):
        """the reference batch {obs, next_obs} at the slots idx"""
        nf = None if self.shared is None else self.shared.next_frame
        tails = [None] * len(idx) if n_step is None else self.ring.walk(idx, n_step, 0.5)["tail"]
        obs = [self.ring.obs_stack(s, K, full) for s in idx]
        nxt = [self.ring.next_stack(s, K, tail=t, next_frame=nf, full=full) for s, t in zip(idx, tails)]
        sh = {k: None if shifts is None else shifts[k] for k in FRAMES}
        return {"obs": R.render_batch(obs, self.shape, sh["obs"]), "next_obs": R.render_batch(nxt, self.shape, sh["next_obs"])}

    def check(self, K, n_step=None, what=None, **kw):
        idx = np.arange(self.buf.stored)
        from dgvit_amd.replay import DeviceReplayBuffer
        out = DeviceReplayBuffer.sample(self.buf, len(idx), indices=_dev(idx), frame_stack=K, n_step=n_step, gamma=0.5, **kw)
        shifts = {k: out[k + "_shift"].cpu().numpy() for k in FRAMES} if kw.get("random_shift") else None
        want = self.want(idx, K, n_step, shifts)
        for k in FRAMES:
            got = out[k]
            assert got.shape == (len(idx), *self.shape, K) and got.dtype == torch.float32 and got.is_contiguous(), (k, what)
            assert np.array_equal(got.cpu().numpy().view(np.int32), want[k].view(np.int32)), (k, K, n_step, what)
        return out


# ------------------------------------------------------------------------------------------------ 1. every slot, every K
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("E, size", RINGS)
def test_every_slot_has_the_stack_of_the_ring_model(amd, E, size, shape, dtype, kind):
    """partly filled (5 steps), exactly full (size / E steps) and wrapped (2 size / E + 3 steps), K in {1, 2, 3, 4, 5, 16}, n_step
    None and 3; K = 1 equals the plain sample's unsqueeze(-1) and every other key is the plain sample's"""
    depth = size // E
    T = 2 * depth + 3
    strs, frs, d = _world(E, T, shape)
    tw = Twin(kind, E, size, shape, dtype)
    stops = {min(5, depth) - 1, depth - 1, T - 1} | ({depth, depth + 1} if depth == 1 else set())
    for t in range(T):
        tw.add(strs, frs, d, t)
        if t not in stops:
            continue
        assert (tw.buf.stored == size) == (t >= depth - 1)
        idx = _dev(np.arange(tw.buf.stored))
        for n_step in (None, 3):
            plain = tw.buf.sample(len(idx), indices=idx, n_step=n_step, gamma=0.5)
            for K in KS:
                out = tw.check(K, n_step, (t, kind))
                assert set(out) == set(plain)
                for k in plain:
                    ref = plain[k].unsqueeze(-1) if k in FRAMES else plain[k]
                    if k not in FRAMES or K == 1:
                        assert torch.equal(out[k], ref), (k, K, n_step, t)
                    else:
                        assert torch.equal(out[k][..., -1], plain[k]), "channel K - 1 is the single frame"
    if kind == "small_pool" and depth > 1:
        assert tw.buf.lost_terminal_frames() == tw.shared.lost > 0, "the lost-frame fallback was part of the comparison"
    if depth > 5:
        depths = {len(tw.ring.preds(s, 16)) for s in range(size)}
        assert {1, 2, 5} <= depths, "episodes of 1, 2 and 5 steps cut their stacks"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
def test_tracking_started_late(amd, dtype):
    """six steps stored before anything tracked episodes: their ends are unknown apart from done, and the first stacked sample starts
    tracking with HEAD on the newest step"""
    E, size, shape = 3, 36, (5, 7)
    strs, frs, d = _world(E, 27, shape)
    tw = Twin("two", E, size, shape, dtype, tracked=False)
    for t in range(6):
        tw.add(strs, frs, d, t, ends=False)
    assert tw.buf.episode_flags is None
    tw.check(4, None, "late")
    assert tw.buf.episode_flags is not None and tw.buf.episode_flags.tolist() == tw.ring.flags.tolist()
    crossed = [s for s in range(18) if strs[s % 3][s // 3 - 1][2] and not strs[s % 3][s // 3 - 1][1] and s >= 3]
    assert crossed and all(len(tw.ring.preds(s, 2)) == 2 for s in crossed), "an END nobody told the ring is crossed"
    for t in range(6, 27):
        tw.add(strs, frs, d, t)
        if t in (8, 11, 26):
            for K in (3, 16):
                tw.check(K, None, t), tw.check(K, 3, t)


# ------------------------------------------------------------------------------------------------ 2. the random shift
@pytest.mark.parametrize("kind", KINDS[:2])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_one_shift_per_sample_for_all_channels_and_the_unstacked_draw(amd, shape, dtype, kind):
    E, size = 3, 36
    strs, frs, d = _world(E, 27, shape)
    tw = Twin(kind, E, size, shape, dtype)
    for t in range(17):
        tw.add(strs, frs, d, t)
    idx = _dev(np.arange(size))
    for K, n_step in ((1, None), (3, None), (4, 3), (16, None)):
        torch.manual_seed(11)
        out = tw.check(K, n_step, "shift", random_shift=2, return_shifts=True)
        torch.manual_seed(11)
        plain = tw.buf.sample(size, indices=idx, random_shift=2, return_shifts=True, n_step=n_step, gamma=0.5)
        for k in FRAMES:
            assert torch.equal(out[k + "_shift"], plain[k + "_shift"]), "the unstacked call's draw"
            assert torch.equal(out[k][..., -1], plain[k])
        assert out["obs_shift"].abs().max() > 0 and not torch.equal(out["obs_shift"], out["next_obs_shift"])
    out = tw.buf.sample(size, indices=idx, frame_stack=2, return_shifts=True)
    assert not out["obs_shift"].any() and out["obs_shift"].shape == (size, 2)


# ------------------------------------------------------------------------------------------------ 3. prioritized draws
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
def test_the_prioritized_buffer_returns_the_stacks_of_its_drawn_slots(amd, dtype):
    from dgvit_amd.replay import PrioritizedDeviceReplayBuffer
    E, size, shape = 3, 36, (6, 10)
    strs, frs, d = _world(E, 27, shape)
    tw = Twin("shared", E, size, shape, dtype, cls=PrioritizedDeviceReplayBuffer)
    for t in range(15):
        tw.add(strs, frs, d, t)
    tw.buf.update_priorities(torch.arange(size, device="cuda"), torch.rand(size, device="cuda"))
    for n_step in (None, 3):
        out = tw.buf.sample(64, 0.7, frame_stack=3, n_step=n_step, gamma=0.5)
        idx = out["indexes"].cpu().numpy()
        assert out["weights"].shape == (64, 1) and len(set(idx.tolist())) > 8
        want = tw.want(idx, 3, n_step)
        for k in FRAMES:
            assert np.array_equal(out[k].cpu().numpy(), want[k]), (k, n_step)


# ------------------------------------------------------------------------------------------------ 4. a captured sample
def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fn()
    return graph, static


@pytest.mark.parametrize("kind", KINDS[:2])
def test_a_captured_stacked_sample_follows_the_ring_and_keeps_its_full_bit(amd, kind):
    E, size, shape = 3, 36, (5, 7)
    strs, frs, d = _world(E, 27, shape)
    tw = Twin(kind, E, size, shape, torch.uint8)
    for t in range(8):                           # 24 of 36 slots: captured before the ring first fills
        tw.add(strs, frs, d, t)
    idx = np.arange(size)
    on_dev = _dev(idx)
    early, early_out = _capture(lambda: tw.buf.sample(size, indices=on_dev, frame_stack=3, n_step=2, gamma=0.5))
    for t in range(8, 14):                       # 42 slots offered: full and wrapped
        tw.add(strs, frs, d, t)
    late, late_out = _capture(lambda: tw.buf.sample(size, indices=on_dev, frame_stack=3, n_step=2, gamma=0.5))
    before = {k: v.clone() for k, v in late_out.items()}
    for t in range(14, 20):
        tw.add(strs, frs, d, t)
    late.replay()
    early.replay()
    torch.cuda.synchronize()
    eager = tw.buf.sample(size, indices=_dev(idx), frame_stack=3, n_step=2, gamma=0.5)
    for k in eager:
        assert torch.equal(late_out[k], eager[k]), ("a graph captured on the full ring follows later add_vec()s", k)
    assert not torch.equal(before["obs"], late_out["obs"]), "the ring has moved on"
    want, frozen = tw.want(idx, 3, 2), tw.want(idx, 3, 2, full=False)
    for k in FRAMES:
        assert np.array_equal(eager[k].cpu().numpy(), want[k]), k
        assert np.array_equal(early_out[k].cpu().numpy(), frozen[k]), ("captured before the first fill: the seam stays an episode start", k)
    assert not np.array_equal(want["obs"], frozen["obs"]), "and that is visible at the seam"
    for k in eager:
        if k not in FRAMES:
            assert torch.equal(early_out[k], eager[k]), k


def test_a_stacked_sample_inside_a_capture_needs_the_flags(amd, monkeypatch):
    """like n_step: the flags cannot be allocated while a stream is capturing (the question is answered by a stand-in: nothing is
    captured here)"""
    import dgvit_amd
    strs, frs, d = _world(3, 27, (5, 7))
    buf = _buffer("two", 3, 36, (5, 7), torch.float32)
    buf.add_vec(**_step(d, 0))
    idx = torch.arange(3, device="cuda")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(dgvit_amd.DgvitError, match="track_episodes"):
        buf.sample(3, indices=idx, frame_stack=2)
    assert buf.episode_flags is None


# ------------------------------------------------------------------------------------------------ 5. the acting side
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
@pytest.mark.parametrize("K", [1, 4, 16])
def test_frame_stack_push_is_what_sample_returns_for_the_slot(amd, K, dtype):
    """the usual loop for 20 steps of 3 environments with staggered episode ends: push the observation, store the transition; the reset
    mask of a step -- the environments whose last transition ended their episode -- is given on the host (even steps) or on the device"""
    from dgvit_amd.replay import FrameStack
    E, size, shape, T = 3, 36, (6, 10), 20
    strs, frs, d = _world(E, 27, shape)
    tw = Twin("two", E, size, shape, dtype)
    fs = FrameStack(num_envs=E, obs_shape=shape, frames=K, device="cuda")
    pushed, resets = [], []
    for t in range(T):
        reset = np.array([t == 0 or S.terminal(strs[e][t - 1]) for e in range(E)])
        frame = d["obs"][t] if t % 3 == 0 else _dev(d["obs"][t])
        got = fs.push(frame, reset=None if t == 0 else (reset if t % 2 == 0 else _dev(reset)))
        assert got.data_ptr() == fs.stack.data_ptr() and got.shape == (E, *shape, K) and got.is_contiguous()
        pushed.append(got.clone()), resets.append(reset)
        tw.add(strs, frs, d, t)
        slots = np.arange(t * E, (t + 1) * E) % size
        now = tw.buf.sample(E, indices=_dev(slots), frame_stack=K)
        if t < size // E:                        # nothing the stack holds has left the ring yet
            assert torch.equal(now["obs"], pushed[t]), t
        if t:
            keep = _dev(~reset)
            assert torch.equal(pushed[t][keep], before["next_obs"][keep]), "the next step's unreset stack is next_obs"
        before = now
    assert any(r.any() and not r.all() for r in resets[1:]), "staggered ends"
    compared = 0
    for t in range(T):                           # against the streams alone, and against the ring at the end where it still can know
        for e in range(E):
            ids = R.truth_obs(strs, frs, e, t, T - 1, K, E, 10 ** 6)
            assert np.array_equal(pushed[t][e].cpu().numpy(), R.render(ids, shape)), (t, e)
            if t > T - 1 - size // E and ids == R.truth_obs(strs, frs, e, t, T - 1, K, E, size):
                got = tw.buf.sample(1, indices=_dev(np.array([(t * E + e) % size])), frame_stack=K)["obs"][0]
                assert torch.equal(got, pushed[t][e]), (t, e)
                compared += 1
    assert compared >= 12
    fs.reset()
    assert not fs.stack.any()
    again = fs.push(_dev(d["obs"][3]))
    assert torch.equal(again, _dev(d["obs"][3]).unsqueeze(-1).expand(E, *shape, K)), "the first push after reset() fills every channel"
    assert torch.equal(fs.push(_dev(d["obs"][4]), reset=True), _dev(d["obs"][4]).unsqueeze(-1).expand(E, *shape, K))


def test_frame_stack_of_one_environment_takes_a_bare_frame_and_is_capturable(amd):
    from dgvit_amd.replay import FrameStack
    shape, K = (5, 7), 3
    fs = FrameStack(num_envs=1, obs_shape=shape, frames=K, device="cuda")
    frames = [_dev(S.pixels(i, shape)) for i in range(5)]
    assert torch.equal(fs.push(frames[0])[0], torch.stack([frames[0]] * 3, dim=-1))
    assert torch.equal(fs.push(frames[1].cpu().numpy())[0], torch.stack([frames[0], frames[0], frames[1]], dim=-1))
    static, mask = torch.zeros(1, *shape, device="cuda"), torch.zeros(1, dtype=torch.bool, device="cuda")
    graph, out = _capture(lambda: fs.push(static, reset=mask))
    fs.reset()
    fs.push(frames[0])
    for i in (1, 2, 3):
        static.copy_(frames[i][None])
        graph.replay()
    assert torch.equal(out[0], torch.stack(frames[1:4], dim=-1))
    mask.fill_(True)
    static.copy_(frames[4][None])
    graph.replay()
    assert torch.equal(out[0], torch.stack([frames[4]] * 3, dim=-1))
    with pytest.raises(ValueError, match="frame"):
        fs.push(torch.zeros(2, *shape, device="cuda"))
    with pytest.raises(ValueError, match="reset"):
        fs.push(frames[0], reset=np.zeros(2, bool))


# ------------------------------------------------------------------------------------------------ 6. nothing else moved
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
def test_a_sample_without_the_keyword_is_the_existing_gathers_output(amd, dtype):
    from dgvit_amd import _lib, preprocess
    from dgvit_amd.functional import _ptr, _stream
    E, size, shape = 3, 36, (5, 7)
    strs, frs, d = _world(E, 27, shape)
    buf = _buffer("two", E, size, shape, dtype)
    for t in range(9):
        buf.add_vec(**_step(d, t))
    idx = torch.arange(27, device="cuda")
    out = buf.sample(27, indices=idx)
    lib, u8 = _lib.load(), dtype is torch.uint8
    for k in FRAMES:
        raw = torch.empty(27, 36, device="cuda")
        if u8:
            rc = lib.dgvit_gather_rows_u8(_ptr(buf.store[k]), _ptr(idx), _ptr(raw), 27, 35, buf.row_bytes, 36, size, _stream())
        else:
            rc = lib.dgvit_gather_rows(_ptr(buf.store[k]), _ptr(idx), _ptr(raw), 27, 36, size, _stream())
        assert rc == 0 and torch.equal(out[k], raw[:, :35].reshape(27, 5, 7)), k
    torch.manual_seed(5)
    out = buf.sample(27, indices=idx, random_shift=2, return_shifts=True)
    for j, k in enumerate(FRAMES):
        raw, shifts = torch.empty(27, 36, device="cuda"), torch.empty(27, 2, dtype=torch.int32, device="cuda")
        preprocess._gather_shift(buf.store[k], idx, raw, shifts, shape, size, 2, j, buf.shift_seed)
        assert torch.equal(out[k], raw[:, :35].reshape(27, 5, 7)) and torch.equal(out[k + "_shift"], shifts), k
    assert buf.episode_flags is None, "no flags on a buffer that never asked for them"
    assert set(out) == set(FIELDS) | {"obs_shift", "next_obs_shift", "indexes"}


# ------------------------------------------------------------------------------------------------ 7. a row longer than the stack
@pytest.mark.parametrize("shifted", [False, True], ids=["plain", "shifted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "u8"])
@pytest.mark.parametrize("shape, K, row_floats", [((6, 10), 4, 256), ((5, 7), 3, 3200), ((6, 10), 16, 16448), ((5, 7), 1, 36), ((5, 7), 1, 1064)],
                         ids=str)
def test_every_float_up_to_row_floats_is_written_zeros_behind_the_stack(amd, shape, K, row_floats, dtype, shifted):
    """the entry points themselves with a row_floats beyond al4(H W K), as include/dgvit_hip.h allows: 256 floats for a 240-float stack
    (groups that no thread formed inside the first workgroup's range), and rows that reach into a second workgroup's range (more than
    1024 K floats); out starts as NaN, the row behind the last sample must stay NaN"""
    from dgvit_amd import _lib
    from dgvit_amd.functional import _ptr, _stream
    B, nrows, cols = 5, 9, shape[0] * shape[1]
    u8 = dtype is torch.uint8
    ld = (cols + 15) & ~15 if u8 else (cols + 3) & ~3
    g = torch.Generator().manual_seed(K * row_floats)
    codes = torch.randint(0, 256, (2, nrows, ld), generator=g, dtype=torch.uint8)
    codes[..., cols:] = 255                      # what lies in a ring row's padding must not come out
    src = [(c if u8 else c.float() / 255.0).cuda() for c in codes]
    rows = torch.randint(0, nrows, (B, K), generator=g).cuda()
    out = torch.full((B + 1, row_floats), float("nan"), device="cuda")
    lib = _lib.load()
    if shifted:
        rc = lib.dgvit_gather_shift_stack_frames(_ptr(src[0]), _ptr(src[1]), _ptr(rows), _ptr(out), None, B, shape[0], shape[1], K, int(u8), ld,
                                                 row_floats, nrows, nrows, 0, 0, 0, None, _stream())
    else:
        rc = lib.dgvit_gather_stack_frames(_ptr(src[0]), _ptr(src[1]), _ptr(rows), _ptr(out), B, cols, K, int(u8), ld, row_floats, nrows, nrows,
                                           _stream())
    assert rc == 0, lib.dgvit_last_error()
    frames = codes.float() / 255.0
    want = torch.zeros(B, row_floats)
    for b in range(B):
        chans = [frames[int(c == K - 1), int(rows[b, c]), :cols] for c in range(K)]
        want[b, :cols * K] = torch.stack(chans, dim=-1).reshape(-1)
    got = out.cpu()
    assert torch.equal(got[:B].view(torch.int32), want.view(torch.int32))
    assert bool(got[B].isnan().all()), "nothing is written behind the last sample's row"
