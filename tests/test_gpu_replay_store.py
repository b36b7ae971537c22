"""GPU: every kind of input that ``add`` / ``add_batch`` accept, through the one store path of DESIGN 3.36 (``_travel`` + ``_commit``:
dgvit_ring_store_frames, dgvit_ring_store_small and, for add_batch with tracked episodes, dgvit_ring_mark).

After every call the WHOLE ring, padding columns included, is compared bit for bit with a numpy expectation built here -- an fp32 ring
holds the float32 value of what was given (uint8 means 0..255), a uint8 ring's frame fields hold tests/replay_u8_ref.py's codes of that
value, or the codes given -- and the episode flags, next_index and stored with tests/nstep_ref.py's ring.  Frames are 5 x 7 in a ring of 7
slots (the element-wise path and the zeroed tail) and 6 x 10 in a ring of 36."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nstep_ref as N  # noqa: E402
import replay_u8_ref as R  # noqa: E402

FRAMES = ("obs", "next_obs")
FIELDS = ("obs", "pobs", "act", "rew", "next_obs", "next_pobs", "done")
# the forms a field rotates through, so every call mixes host and device inputs; the first five are the ones an fp32 ring never saw
KINDS = ("dev32", "dev64", "devu8", "view", "host64", "hostu8", "host32", "list")


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


def _input(kind, g, shape):
    """one field in one form -> (what add / add_batch is given, what it means: float32 values, or uint8 where bytes were given)"""
    if kind.endswith("u8"):
        c = g.integers(0, 256, shape, dtype=np.uint8)
        return (torch.from_numpy(c).cuda() if kind == "devu8" else c), c
    a = 1.5 * g.random(shape) - 0.25                   # float64 that must be rounded to fp32; frames spill past [0, 1]
    f = a.astype(np.float32)
    if kind == "view":                                 # a strided device view: every other element of a wider tensor
        v = torch.from_numpy(np.stack([f, f + 1], axis=-1)).cuda()[..., 0]
        assert f.size == 1 or not v.is_contiguous()
        return v, f
    return {"dev32": lambda: torch.from_numpy(f).cuda(), "dev64": lambda: torch.from_numpy(a).cuda(), "host64": lambda: a,
            "host32": lambda: f, "list": lambda: a.tolist()}[kind](), f


def _stored(buf, k, meant):
    """the ring rows (n, row) that hold ``meant`` (n, ...) in field k: zeros behind the field's columns"""
    n, cnt = meant.shape[0], buf.fields[k]
    m = meant.reshape(n, cnt)
    if buf.store[k].dtype == torch.uint8:
        m = m if m.dtype == np.uint8 else R.quantize(m)
    else:
        m = m.astype(np.float32)                       # bytes given to an fp32 matrix are the values 0 .. 255
    out = np.zeros((n, buf.store[k].shape[1]), m.dtype)
    out[:, :cnt] = m
    return out


@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8], ids=["fp32", "u8"])
@pytest.mark.parametrize("S, H, W", [(7, 5, 7), (36, 6, 10)], ids=["7x5x7", "36x6x10"])
def test_every_input_kind_through_add_and_add_batch(amd, S, H, W, dtype, prioritized):
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    kw = dict(alpha=1.0, eps=0.0) if prioritized else {}
    buf = (PrioritizedDeviceReplayBuffer if prioritized else DeviceReplayBuffer)(S, obs_shape=(H, W), seed=0, frame_dtype=dtype, **kw)
    buf.track_episodes()
    ring = N.Ring(S)
    want = {k: np.zeros(tuple(v.shape), np.uint8 if v.dtype == torch.uint8 else np.float32) for k, v in buf.store.items()}
    g = np.random.default_rng(1000 * S + int(dtype is torch.uint8))
    shapes = {"obs": (H, W), "next_obs": (H, W), "pobs": (2,), "next_pobs": (2,), "act": (2,), "rew": (1,), "done": (1,)}
    pos = calls = 0
    seen = set()
    # three adds; a batch that crosses the ring's end (and whose n divides neither 7 nor 36); 2 size + 3 rows, of which the last `size`
    # stay; a batch of 5, which does not divide the size, from wherever the ring stands; two adds that end an episode each; a batch of 1
    for n in (None, None, None, S - 2, 2 * S + 3, 5, None, None, 1):
        given, meant = {}, {}
        for j, k in enumerate(FIELDS):
            kind = KINDS[(calls + 3 * j) % len(KINDS)]
            if n is None and k in ("rew", "done") and calls % 2 == 0:          # Python scalars, a float and a bool
                x = float(g.integers(-256, 257)) / 256.0 if k == "rew" else bool(g.integers(2))
                given[k], meant[k] = x, np.full((1, 1), x, np.float32)
                seen.add("scalar")
                continue
            given[k], m = _input(kind, g, shapes[k] if n is None else (n,) + shapes[k])
            meant[k] = m.reshape(1, -1) if n is None else m
            seen.add((kind, k in FRAMES))
        start, rows = buf.next_index, 1 if n is None else n
        assert start == ring.next_index
        if n is None:
            buf.add(**given)
        else:
            buf.add_batch(**given)
        kept = min(rows, S)
        slots = (start + np.arange(kept)) % S
        if calls == 3:
            assert n == S - 2 and start == 3 and start + kept > S, "this batch crosses the ring's end"
        for k in FIELDS:
            want[k][slots] = _stored(buf, k, meant[k][-kept:])
        ring.store(meant["rew"].astype(np.float32).reshape(-1), meant["done"].astype(np.float32).reshape(-1), pos + np.arange(rows))
        pos += rows
        if n is None and calls >= 6:
            buf.on_episode_end()
            ring.episode_end()
        for k in FIELDS:
            got = buf.store[k].cpu().numpy()
            assert got.dtype == want[k].dtype and np.array_equal(got.view(np.uint8), want[k].view(np.uint8)), (k, calls, n)
        assert np.array_equal(buf.episode_flags.cpu().numpy(), ring.flags), (calls, n)
        assert (buf.next_index, buf.stored) == (ring.next_index, ring.stored), (calls, n)
        assert np.array_equal(want["rew"][:, 0], ring.rew), "the reference ring holds the same rewards"
        if prioritized:
            leaves = buf.priorities().cpu().numpy()
            assert leaves.shape == (ring.stored,) and (leaves == 1.0).all(), "every written slot took the max priority"
        calls += 1
    assert {(kind, frame) for kind in KINDS for frame in (False, True)} <= seen and "scalar" in seen, "every form reached both kinds of field"
    assert np.count_nonzero(ring.flags & N.END) >= 1 and np.count_nonzero(ring.flags & N.HEAD) == 1
