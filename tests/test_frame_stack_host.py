"""CPU (no GPU): frame stacks -- the numpy restatement tests/frame_stack_ref.py against the truth computed from each
environment's stream alone, the ``frame_stack`` / ``frames`` / ``frame_channels`` checks, the entry points dgvit_ring_stack_rows,
dgvit_gather_stack_frames, dgvit_gather_shift_stack_frames and dgvit_frame_stack_push with their argument checks, and the layout argument
of ``GoT(frame_channels=K)`` in plain torch.  Every library call here fails its argument check before any launch: the pointers are never
dereferenced."""
import ctypes
import os

import numpy as np
import pytest
import torch

import frame_stack_ref as R
import shared_next_ref as S
import vec_replay_ref as V

FAKE = ctypes.c_void_p(0x1000)   # non-null, 16-byte aligned, never read: only argument checks run
OFF8 = ctypes.c_void_p(0x1008)
OFF4 = ctypes.c_void_p(0x1004)
OFF2 = ctypes.c_void_p(0x1002)

NAMES = ("dgvit_ring_stack_rows", "dgvit_gather_stack_frames", "dgvit_gather_shift_stack_frames", "dgvit_frame_stack_push")
SCENARIOS = [(3, 36, 20), (1, 37, 52), (4, 8, 7), (4, 4, 6)]
KS = (1, 2, 3, 4, 5, 16)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


# ------------------------------------------------------------------------------------------------ the restatement against the streams
@pytest.mark.parametrize("E, size, steps", SCENARIOS)
def test_the_ring_model_gives_every_slot_the_stack_of_its_own_stream(E, size, steps):
    """after every step, every written slot, every K: obs and next_obs stacks (one-step and 3-step) equal the truth from the slot's own
    stream; over the run some stack is cut by an episode start, some by the ring's seam, and some reaches its full depth"""
    strs = V.streams(E, steps)
    frs = S.all_frames(strs)
    ring = R.StackRing(E, size)
    cut_by_episode = cut_by_seam = whole = 0
    for newest in range(steps):
        ring.add_vec_frames(strs, frs, newest)
        tails = ring.walk(np.arange(size), 3, 0.5)["tail"]
        for s in np.flatnonzero(ring.pos >= 0):
            e, t = int(s) % E, int(ring.pos[s])
            for K in KS:
                want = R.truth_obs(strs, frs, e, t, newest, K, E, size)
                assert ring.obs_stack(s, K) == want, (newest, s, K)
                assert ring.next_stack(s, K) == R.truth_next(strs, frs, e, t, newest, K, E, size), (newest, s, K)
                assert ring.next_stack(s, K, tail=tails[s]) == R.truth_next(strs, frs, e, t, newest, K, E, size, n=3), (newest, s, K)
                assert want[-1] == frs[e][t][0] and len(want) == K
            d = len(ring.preds(s, 4)) - 1
            start, oldest = R.episode_start(strs[e], t), newest - size // E + 1
            whole += d == 3
            cut_by_episode += d < 3 and t - d == start and start > oldest
            cut_by_seam += d < 3 and t - d == oldest and start < oldest
    if size > 4 * E:
        assert whole and cut_by_episode
    if steps * E > size > E:
        assert cut_by_seam, "the oldest slot's stack repeats its own frame although its episode is older"
    if size == E:
        assert not whole and all(len(ring.preds(s, 16)) == 1 for s in range(size)), "a ring of one step per lane: every stack is one frame"


def test_k1_is_the_single_frame_and_shifted_tables():
    strs = V.streams(3, 20)
    frs = S.all_frames(strs)
    ring = R.StackRing(3, 36)
    for t in range(20):
        ring.add_vec_frames(strs, frs, t)
    for s in range(36):
        assert ring.obs_stack(s, 1) == [ring.obs[s]] and ring.next_stack(s, 1) == [ring.nxt[s]]
        for K in (2, 5):
            assert ring.next_stack(s, K)[:-1] == ring.obs_stack(s, K)[1:], "without n_step the next table is the obs table moved by one"


def test_a_ring_that_is_not_full_stops_at_slot_zero_and_the_frozen_bit_is_conservative():
    strs = [[(np.float32(0), np.float32(0), False)] * 30]
    frs = S.all_frames(strs)
    ring = R.StackRing(1, 8)
    for t in range(5):
        ring.add_vec_frames(strs, frs, t)
    assert ring.obs_stack(1, 4) == [frs[0][0][0]] * 3 + [frs[0][1][0]] and len(ring.preds(4, 4)) == 4
    for t in range(5, 11):                    # wrapped: slot 0 holds step 8, slot 7 step 7
        ring.add_vec_frames(strs, frs, t)
    assert ring.obs_stack(0, 3) == [frs[0][t][0] for t in (6, 7, 8)]
    assert ring.obs_stack(0, 3, full=False) == [frs[0][8][0]] * 3, "a bit frozen before the first fill: the seam is an episode start"
    newest = int(np.argmax(ring.pos))
    oldest = (newest + 1) % 8
    assert ring.flags[newest] == R.HEAD and ring.obs_stack(oldest, 4) == [int(ring.obs[oldest])] * 4, "the known limit at the oldest slot"


def test_render_is_the_replicate_pad_shift_of_every_channel():
    import replay_shift_ref as SH
    ids, shape = [3, 700, 41], (5, 7)
    for shift in ((0, 0), (2, -1), (-2, 2)):
        got = R.render(ids, shape, shift)
        assert got.shape == (5, 7, 3) and got.dtype == np.float32
        frames = torch.from_numpy(np.stack([S.pixels(i, shape) for i in ids]))
        want = SH.ref_shift(frames, torch.tensor([shift] * 3), 2)
        assert np.array_equal(got, want.permute(1, 2, 0).numpy())


# ------------------------------------------------------------------------------------------------ the Python checks
@pytest.mark.parametrize("bad", [0, 17, -1, True, 2.0, "4", np.float32(3)], ids=repr)
def test_bad_values_raise_before_any_device_is_touched(bad):
    """no GPU is needed to get here: on the parent commit these keywords are TypeErrors"""
    from dgvit_amd import replay
    from dgvit_amd.GoalFormer import GoT
    from dgvit_amd.sac_networks import DeterministicGoTPolicy, GoTPolicy, GoTQNetwork
    for cls in (replay.DeviceReplayBuffer, replay.PrioritizedDeviceReplayBuffer):
        buf = object.__new__(cls)
        buf.shapes, buf.alpha, buf.eps = {"obs": (6, 10)}, 0.6, 1e-4
        with pytest.raises(ValueError, match="frame_stack"):
            buf.sample(4, frame_stack=bad)
    with pytest.raises(ValueError, match="frames"):
        replay.FrameStack(num_envs=3, obs_shape=(6, 10), frames=bad, device="cpu")
    with pytest.raises(ValueError, match="frame_channels"):
        GoT(image_size=(12, 20), patch_size=(3, 5), num_classes=2, dim=64, depth=1, heads=2, mlp_dim=64, frame_channels=bad)
    for net in (GoTPolicy, GoTQNetwork, DeterministicGoTPolicy):
        with pytest.raises(ValueError, match="frame_channels"):
            net(2, 2, 1, 2, 64, image_size=(12, 20), patch_size=(3, 5), frame_channels=bad)


def test_frame_stack_arguments_are_checked_on_the_host():
    import dgvit_amd
    from dgvit_amd import replay
    assert replay._frame_stack(None) is None and replay._frame_stack(np.int64(16)) == 16 and replay.STACK_MAX == 16
    for kw in (dict(num_envs=0), dict(num_envs=True), dict(obs_shape=(6,)), dict(obs_shape=(6, 0)), dict(obs_shape=6)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            replay.FrameStack(**{**dict(num_envs=3, obs_shape=(6, 10), frames=4, device="cpu"), **kw})
    with pytest.raises(dgvit_amd.DgvitError, match="HBM"):
        replay.FrameStack(num_envs=3, obs_shape=(6, 10), frames=4, device="cpu")


# ------------------------------------------------------------------------------------------------ GoT(frame_channels=K), host side
def _rearrange(x, p1, p2):
    """einops' 'b (h p1) (w p2) c -> b (h w) (p1 p2 c)' in torch ops"""
    B, H, W, C = x.shape
    h, w = H // p1, W // p2
    return x.reshape(B, h, p1, w, p2, C).permute(0, 1, 3, 2, 4, 5).reshape(B, h * w, p1 * p2 * C)


@pytest.mark.parametrize("H, W, ph, pw, K", [(12, 20, 3, 5, 2), (12, 20, 3, 5, 3), (16, 16, 4, 4, 4), (6, 10, 3, 2, 16)])
def test_the_widened_single_channel_patchify_is_the_channel_last_rearrangement(H, W, ph, pw, K):
    x = torch.arange(2 * H * W * K, dtype=torch.float32).reshape(2, H, W, K)
    wide = x.reshape(2, H, W * K)
    single = _rearrange(wide.unsqueeze(-1), ph, pw * K)           # the (H, W K) / (ph, pw K) single-channel encoder's patches
    assert torch.equal(single, _rearrange(x, ph, pw))
    py, px, c = ph - 2, pw - 1, K - 1
    assert single[1, 3, (py * pw + px) * K + c] == x[1, (3 // (W // pw)) * ph + py, (3 % (W // pw)) * pw + px, c]


def test_got_frame_channels_builds_the_wider_linear_and_k1_is_todays_module():
    from dgvit_amd.GoalFormer import GoT
    kw = dict(image_size=(12, 20), patch_size=(3, 5), num_classes=2, dim=64, depth=2, heads=2, mlp_dim=128)
    torch.manual_seed(0)
    plain = GoT(**kw)
    torch.manual_seed(0)
    one = GoT(**kw, frame_channels=1)
    assert one._cfg == plain._cfg and one.frame_channels == 1
    a, b = plain.state_dict(), one.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in a)
    for K in (2, 3, 4):
        m = GoT(**kw, channels=7, frame_channels=K)
        lin = m.to_patch_embedding[1]
        assert isinstance(lin, torch.nn.Linear) and (lin.in_features, lin.out_features) == (3 * 5 * K, 64)
        wide = GoT(**{**kw, "image_size": (12, 20 * K), "patch_size": (3, 5 * K)})
        assert m._cfg == wide._cfg, "the config of the (H, W K) / (ph, pw K) single-channel encoder"
        assert {k: v.shape for k, v in m.state_dict().items()} == {k: v.shape for k, v in wide.state_dict().items()}
        for bad in (torch.zeros(2, 12, 20), torch.zeros(2, 12, 20, K + 1), torch.zeros(2, K, 12, 20), torch.zeros(2, 12, 20 * K),
                    torch.zeros(2, K, 12, 20).permute(0, 2, 3, 1)):
            with pytest.raises(ValueError, match=r"channel-last \(B, H, W, K\)"):
                m._frames(bad)
        x = torch.zeros(2, 12, 20, K)
        assert m._frames(x).shape == (2, 12, 20 * K) and m._frames(x).data_ptr() == x.data_ptr()
    x3 = torch.zeros(2, 12, 20)
    assert plain._frames(x3) is x3


def test_the_sac_networks_hand_frame_channels_to_the_encoder():
    from dgvit_amd.sac_networks import DeterministicGoTPolicy, GoTPolicy, GoTQNetwork
    for net in (GoTPolicy, GoTQNetwork, DeterministicGoTPolicy):
        m = net(2, 2, 1, 2, 64, image_size=(12, 20), patch_size=(3, 5), frame_channels=3)
        assert m.trans.frame_channels == 3 and m.trans.to_patch_embedding[1].in_features == 45
        plain, one = (net(2, 2, 1, 2, 64, image_size=(12, 20), patch_size=(3, 5), **kw) for kw in ({}, {"frame_channels": 1}))
        assert {k: v.shape for k, v in plain.state_dict().items()} == {k: v.shape for k, v in one.state_dict().items()}


# ------------------------------------------------------------------------------------------------ the entry points
def test_symbols_are_exported_bound_and_declared(lib):
    from dgvit_amd import _lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    with open(os.path.join(os.path.dirname(L.LIB_PATH), os.pardir, "include", "dgvit_hip.h")) as f:
        header = f.read()
    P, I, LL, ULL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_ulonglong
    for name in NAMES:
        assert hasattr(raw, name)
        assert "int " + name + "(" in header
    assert L.SIGNATURES["dgvit_ring_stack_rows"] == (I, [P, P, P, P, LL, P, P, P, LL, LL, LL, I, I, LL, P])
    assert L.SIGNATURES["dgvit_gather_stack_frames"] == (I, [P, P, P, P, LL, LL, I, I, LL, LL, LL, LL, P])
    assert L.SIGNATURES["dgvit_gather_shift_stack_frames"] == (I, [P, P, P, P, P, LL, I, I, I, I, LL, LL, LL, LL, I, I, ULL, P, P])
    assert L.SIGNATURES["dgvit_frame_stack_push"] == (I, [P, P, LL, P, I, LL, LL, I, P])
    # no existing signature changes
    assert L.SIGNATURES["dgvit_gather_shift_frames"] == (I, [P, P, P, P, LL, I, I, LL, LL, I, I, ULL, P, P])
    assert L.SIGNATURES["dgvit_gather_shift_frames_u8"] == (I, [P, P, P, P, LL, I, I, LL, LL, LL, I, I, ULL, P, P])
    assert L.SIGNATURES["dgvit_gather_rows"] == (I, [P, P, P, LL, LL, LL, P])
    assert L.SIGNATURES["dgvit_gather_rows_u8"] == (I, [P, P, P, LL, LL, LL, LL, LL, P])
    assert L.SIGNATURES["dgvit_ring_next_rows"] == (I, [P, P, P, LL, LL, P])
    assert L.SIGNATURES["dgvit_nstep_walk_strided"][1][:4] == [P, LL, P, LL] and len(L.SIGNATURES["dgvit_nstep_walk_strided"][1]) == 20


def test_abi_version_is_unchanged(lib):
    from dgvit_amd import _lib as L
    assert lib.dgvit_abi_version() == 7 and L.ABI_VERSION == 7


def _ids(v):
    return None if isinstance(v, bytes) else "-".join(f"{k}={x if not isinstance(x, ctypes.c_void_p) else x.value}" for k, x in v.items())


def _msg(lib, rc, name, word):
    assert rc == -1, "DGVIT_ERR_ARG"
    msg = lib.dgvit_last_error()
    assert name in msg and word in msg, msg


def _rows(lib, idx=FAKE, tail=None, flags=FAKE, done=FAKE, done_ld=4, next_row=None, obs_rows=FAKE, next_rows=FAKE, nsel=8, nrows=36, envs=3,
          frames=4, full=0, arena_rows=36):
    return lib.dgvit_ring_stack_rows(idx, tail, flags, done, done_ld, next_row, obs_rows, next_rows, nsel, nrows, envs, frames, full, arena_rows,
                                     None)


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in ("idx", "flags", "done", "obs_rows", "next_rows")] + [
    (dict(nsel=0), b"nsel=0"),
    (dict(nsel=1 << 31), b"nsel=2147483648"),
    (dict(nrows=0), b"nrows=0"),
    (dict(nrows=1 << 56, arena_rows=1 << 56), b"nrows="),
    (dict(envs=0), b"envs=0"),
    (dict(envs=72), b"envs=72"),
    (dict(envs=5), b"envs=5"),                    # size % E != 0
    (dict(frames=0), b"frames=0"),
    (dict(frames=17), b"frames=17"),
    (dict(full=2), b"full=2"),
    (dict(done_ld=0), b"done_ld=0"),
    (dict(arena_rows=40), b"arena_rows=40"),      # without next_row the next_obs matrix has nrows rows
    (dict(next_row=FAKE, arena_rows=35), b"arena_rows=35"),
    (dict(next_row=FAKE, arena_rows=1 << 31), b"arena_rows=2147483648"),
    (dict(idx=OFF4), b"aligned"),
    (dict(tail=OFF4), b"aligned"),
    (dict(obs_rows=OFF4), b"aligned"),
    (dict(next_rows=OFF4), b"aligned"),
    (dict(done=OFF2), b"aligned"),
    (dict(next_row=OFF2, arena_rows=40), b"aligned"),
], ids=_ids)
def test_ring_stack_rows_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _rows(lib, **kw), b"ring_stack_rows", word)


STACK = [                                         # check_stack: asked by both gathers
    (dict(nsel=0), b"nsel=0"),
    (dict(nsel=1 << 24), b"nsel=16777216"),
    (dict(nrows0=0), b"nrows0=0"),
    (dict(nrows1=-1), b"nrows1=-1"),
    (dict(frames=0), b"frames=0"),
    (dict(frames=17), b"frames=17"),
    (dict(ring_u8=2), b"ring_u8=2"),
    (dict(ring_ld=62), b"ring_ld=62"),            # not a multiple of 4 floats
    (dict(ring_ld=56), b"ring_ld=56"),            # shorter than a frame
    (dict(ring_u8=1, ring_ld=60), b"ring_ld=60"),  # a byte ring's rows are multiples of 16
    (dict(row_floats=236), b"row_floats=236"),    # less than cols * frames = 240
    (dict(row_floats=242), b"row_floats=242"),
    (dict(src0=OFF8), b"aligned"),
    (dict(src1=OFF8), b"aligned"),
    (dict(out=OFF8), b"aligned"),
    (dict(rows=OFF4), b"aligned"),
]


def _gather(lib, src0=FAKE, src1=FAKE, rows=FAKE, out=FAKE, nsel=8, cols=60, frames=4, ring_u8=0, ring_ld=60, row_floats=240, nrows0=36,
            nrows1=36):
    return lib.dgvit_gather_stack_frames(src0, src1, rows, out, nsel, cols, frames, ring_u8, ring_ld, row_floats, nrows0, nrows1, None)


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in ("src0", "src1", "rows", "out")] + STACK + [
    (dict(cols=0), b"cols=0"),
    (dict(cols=(1 << 23) + 4, frames=16, ring_ld=(1 << 23) + 4, row_floats=(1 << 27) + 64), b"2^27"),   # H W K past the index width
], ids=_ids)
def test_gather_stack_frames_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _gather(lib, **kw), b"gather_stack_frames", word)


def _shift(lib, src0=FAKE, src1=FAKE, rows=FAKE, out=FAKE, shifts_out=None, nsel=8, H=6, W=10, frames=4, ring_u8=0, ring_ld=60,
           row_floats=240, nrows0=36, nrows1=36, pad=2, stream_id=0, seed=1, seed_dev=None):
    return lib.dgvit_gather_shift_stack_frames(src0, src1, rows, out, shifts_out, nsel, H, W, frames, ring_u8, ring_ld, row_floats, nrows0,
                                               nrows1, pad, stream_id, seed, seed_dev, None)


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in ("src0", "src1", "rows", "out")] + STACK + [
    (dict(H=0), b"H=0"),
    (dict(W=-1), b"W=-1"),
    (dict(pad=-1), b"pad=-1"),
    (dict(pad=6), b"pad=6"),
    (dict(stream_id=-1), b"stream_id=-1"),
    (dict(stream_id=1 << 20), b"stream_id="),
    (dict(shifts_out=OFF2), b"aligned"),
    (dict(seed_dev=OFF4), b"aligned"),
    (dict(H=1 << 12, W=(1 << 11) + 1, frames=16, ring_ld=(1 << 23) + (1 << 12), row_floats=(1 << 27) + (1 << 16)), b"2^27"),
], ids=_ids)
def test_gather_shift_stack_frames_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _shift(lib, **kw), b"gather_shift_stack_frames", word)


def _push(lib, stack=FAKE, frame=FAKE, frame_ld=60, reset=None, reset_all=0, envs=3, cols=60, frames=4):
    return lib.dgvit_frame_stack_push(stack, frame, frame_ld, reset, reset_all, envs, cols, frames, None)


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in ("stack", "frame")] + [
    (dict(envs=0), b"envs=0"),
    (dict(envs=1 << 24), b"envs=16777216"),
    (dict(frames=0), b"frames=0"),
    (dict(frames=17), b"frames=17"),
    (dict(cols=0), b"cols=0"),
    (dict(cols=(1 << 23) + 1, frames=16, frame_ld=1 << 24), b"2^27"),
    (dict(frame_ld=59), b"frame_ld=59"),
    (dict(reset_all=2), b"reset_all=2"),
    (dict(stack=OFF2), b"aligned"),
    (dict(frame=OFF2), b"aligned"),
], ids=_ids)
def test_frame_stack_push_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _push(lib, **kw), b"frame_stack_push", word)
