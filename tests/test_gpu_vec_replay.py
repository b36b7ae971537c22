"""GPU: the replay ring of E parallel environments -- DeviceReplayBuffer(num_envs=E), add_vec, on_episode_end(envs=) and
sample(n_step=) through dgvit_ring_store_frames, dgvit_ring_store_small and dgvit_nstep_walk_strided.

What is stored is compared bit for bit with what was given (uint8 rings: with replay_u8_ref's quantisation), the flags with the numpy
restatement tests/vec_replay_ref.py, and every n-step value with ``vec_replay_ref.truth``: nstep_ref.truth on the sampled slot's own
environment stream, cut behind the newest step -- no ring in it.  ``rew`` must be within nstep_ref's derived tolerance
2^-23 |ref| + m 2^-52 sum_k gamma^k |r_k| of the float64 sum, ``discount`` within 2^-23 relative of gamma^m, and both bit-equal where the
arithmetic is exact (nstep_ref.exact); steps, done, obs, pobs, act, next_obs and next_pobs are exact and always the same environment's.
Frames are 6 x 10 (H W a multiple of 4) and 5 x 7 (the element-wise path and the zeroed tail); E = 3 in a ring of 36 slots (fewer than
64 E: the walk's modulo path) and of 300 (more: its subtraction path), E = 4 in rings of 4 and 8 slots.

Measured on an MI355X (the tests print the figures): largest |rew - ref64| / tolerance 0.426 on the 36-slot rings, 0.489 on the 300-slot
ring; torch.cuda.set_sync_debug_mode("error") does raise on .item() in this ROCm build, so the all-device calls also ran under it."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import nstep_ref as N  # noqa: E402
import replay_shift_ref as RS  # noqa: E402
import replay_u8_ref as R  # noqa: E402
import vec_replay_ref as V  # noqa: E402

FIELDS = ("obs", "pobs", "act", "rew", "next_obs", "next_pobs", "done")
FRAMES = ("obs", "next_obs")
E3, SIZE, STEPS = 3, 36, 20


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


@functools.lru_cache(maxsize=None)
def _world(E, T, H=6, W=10):
    """(streams, data): data[k][t, e] is field k of environment e's transition t; frames as ``codes`` and as the exact floats code / 255.
    Computed once per shape and left unchanged."""
    strs = V.streams(E, T)
    g = np.random.default_rng(1000 * E + T)
    rows = np.arange(T * E)
    codes = {"obs": R.pattern(rows, H, W).reshape(T, E, H, W), "next_obs": R.pattern(5000 + rows, H, W).reshape(T, E, H, W)}
    d = {k: R.dequantize(v) for k, v in codes.items()}
    d.update({k: g.standard_normal((T, E, 2)).astype(np.float32) for k in ("pobs", "next_pobs", "act")})
    d["rew"] = np.array([[[s[t][0]] for s in strs] for t in range(T)], np.float32)
    d["done"] = np.array([[[s[t][1]] for s in strs] for t in range(T)], np.float32)
    d["end"] = np.array([[s[t][2] for s in strs] for t in range(T)], bool)
    d["codes"] = codes
    return strs, d


def _buffer(E, size, H=6, W=10, cls=None, **kw):
    from dgvit_amd.replay import DeviceReplayBuffer
    return (cls or DeviceReplayBuffer)(size, obs_shape=(H, W), pstate_dim=V.PSTATE, act_dim=V.ACT, seed=0, num_envs=E, **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _step(d, t, mode, u8):
    """the keywords of add_vec for step t -> (kw, on_episode_end argument or None)"""
    f = {k: d[k][t] for k in FIELDS}
    end = d["end"][t]
    if mode == "device":          # every field and the ends on the device; rew (E,), done (E, 1); the three dtypes of episode_end in turn
        kw = {k: _dev(v) for k, v in f.items()}
        kw["rew"] = kw["rew"].reshape(-1)
        kw["episode_end"] = (_dev(end), _dev(end.astype(np.uint8) * 7), _dev(end.astype(np.float32) * -2.5))[t % 3]
        return kw, None
    if mode == "codes":           # a uint8 ring given its codes on the device
        kw = {k: _dev(d["codes"][k][t] if k in FRAMES else v) for k, v in f.items()}
        kw["episode_end"] = _dev(end)
        return kw, None
    if mode == "host":            # nothing on the device: arrays, a CPU tensor, lists; a uint8 ring gets next_obs as host codes
        kw = dict(f)
        kw["pobs"], kw["act"], kw["done"] = torch.from_numpy(f["pobs"].copy()), f["act"].tolist(), f["done"].reshape(-1)
        if u8:
            kw["next_obs"] = d["codes"]["next_obs"][t]
        kw["episode_end"] = end.tolist()
        return kw, None
    assert mode == "mixed"        # per field; pobs is a strided view, made contiguous on the device; the ends come by on_episode_end
    kw = dict(f)
    wide = _dev(np.concatenate([f["pobs"], f["pobs"] + 1], axis=1))
    kw["obs"], kw["pobs"], kw["done"], kw["rew"] = _dev(f["obs"]), wide[:, :2], _dev(f["done"]), torch.from_numpy(f["rew"].copy())
    assert not kw["pobs"].is_contiguous()
    if u8:
        kw["obs"], kw["next_obs"] = _dev(d["codes"]["obs"][t]), f["next_obs"]
    ends = (_dev(end), end, _dev(np.flatnonzero(end)), np.flatnonzero(end).tolist())[t % 4]
    return kw, ends


def _rows(buf):
    """what the ring holds, as numpy: {field: (size, row)}"""
    return {k: v.cpu().numpy() for k, v in buf.store.items()}


def _feed(buf, d, steps, mode, first=0, want=None, ring=None):
    """steps first .. first + steps - 1 through add_vec; after every step the WHOLE ring (so a stray write shows) against the expected
    rows ``want`` and the flags against the restatement ``ring`` -> (want, ring)"""
    E, size, u8 = buf.num_envs, buf.size, buf.frame_dtype is torch.uint8
    if want is None:
        want = {k: np.zeros(tuple(v.shape), np.uint8 if v.dtype == torch.uint8 else np.float32) for k, v in buf.store.items()}
        ring = V.VecRing(E, size, tracked=False)
    for t in range(first, first + steps):
        kw, ends = _step(d, t, mode, u8)
        base = buf.next_index
        assert base == (t * E) % size
        buf.add_vec(**kw)
        ring.add_vec(d["rew"][t], d["done"][t], t, d["end"][t] if ends is None else None)
        if ends is not None:
            buf.on_episode_end(envs=ends)
            ring.episode_end(d["end"][t])
        for k in FIELDS:
            src = d["codes"][k][t] if (u8 and k in FRAMES) else d[k][t]
            want[k][base:base + E] = 0
            want[k][base:base + E, :buf.fields[k]] = src.reshape(E, -1)
        got = _rows(buf)
        for k in FIELDS:
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (k, t, mode)
        assert np.array_equal(buf.episode_flags.cpu().numpy(), ring.flags), (t, mode)
        assert (buf.next_index, buf.stored) == (ring.next_index, ring.stored) == (((t + 1) * E) % size, min((t + 1) * E, size))
    return want, ring


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _positions(E, size, newest):
    """per slot, the step it holds once steps 0 .. newest are stored (-1: never written)"""
    pos = np.full(size, -1)
    for t in range(newest + 1):
        pos[(t * E) % size:(t * E) % size + E] = t
    return pos


def _against_truth(buf, strs, d, newest, idx=None, ns=N.NS, gammas=N.GAMMAS, frames=True, **kw):
    """sample(n_step=n, gamma=g) at the slots idx (default: every stored slot) for every n and g against the truth of each slot's own
    environment stream -> (the largest |rew - ref| / tolerance, the last batch)"""
    from dgvit_amd.replay import DeviceReplayBuffer
    E, size = buf.num_envs, buf.size
    pos = _positions(E, size, newest)
    idx = np.arange(buf.stored) if idx is None else np.asarray(idx)
    assert (pos[idx] >= 0).all()
    idx_d, worst, b = _dev(idx.astype(np.int64)), 0.0, None
    for n in ns:
        for gamma in gammas:
            b = DeviceReplayBuffer.sample(buf, 0, indices=idx_d, n_step=n, gamma=gamma, **kw)      # (the prioritized sample() draws its own)
            got = {k: v.cpu().numpy() for k, v in b.items()}
            assert np.array_equal(got["indexes"], idx), "indexes stay the start slots"
            for j, s in enumerate(idx):
                e, t = int(s) % E, int(pos[s])
                ret, disc, m, tail, done, _ = V.truth(strs, e, t, newest, n, gamma)
                where = (s, e, t, n, gamma)
                assert got["steps"][j] == m and got["done"][j, 0] == done, where
                err, tol = abs(float(got["rew"][j, 0]) - ret), V.tolerance(strs[e], t, m, gamma, ret)
                assert err <= tol, (where, err, tol)
                assert abs(float(got["discount"][j, 0]) - disc) <= 2.0 ** -23 * disc, where
                if N.exact(n, gamma):
                    assert _bits(got["rew"][j]) == _bits(np.float32(ret)) and _bits(got["discount"][j]) == _bits(np.float32(disc)), where
                worst = max(worst, err / tol if tol > 0 else 0.0)
                for k, at in (("pobs", t), ("act", t), ("next_pobs", tail)) + ((("obs", t), ("next_obs", tail)) if frames else ()):
                    assert np.array_equal(_bits(got[k][j]), _bits(d[k][at, e])), (k, where, "another transition's, or another environment's")
    return worst, b


# ------------------------------------------------------------------------------------------------ 1. the store, 3. n-step against the truth
@pytest.mark.parametrize("H, W", [(6, 10), (5, 7)], ids=["6x10", "5x7"])
@pytest.mark.parametrize("dtype, mode", [(torch.float32, "device"), (torch.uint8, "device"), (torch.uint8, "codes"), (torch.float32, "host"),
                                         (torch.uint8, "host"), (torch.float32, "mixed"), (torch.uint8, "mixed")],
                         ids=["fp32-device", "u8-device", "u8-codes", "fp32-host", "u8-host", "fp32-mixed", "u8-mixed"])
def test_store_and_n_step_after_5_12_and_20_steps(amd, dtype, mode, H, W):
    """E = 3, 36 slots: after step 5 the ring is partially filled, after step 12 exactly full, after step 20 it has wrapped"""
    strs, d = _world(E3, STEPS, H, W)
    buf = _buffer(E3, SIZE, H, W, frame_dtype=dtype)
    want = ring = None
    worst, done = 0.0, 0
    full = mode == "device" and (H, W) == (6, 10)         # every n and gamma there; elsewhere the store is the subject
    for upto in (5, 12, 20):
        want, ring = _feed(buf, d, upto - done, mode, done, want, ring)
        done = upto
        w, _ = _against_truth(buf, strs, d, upto - 1, ns=N.NS if full else (3,), gammas=N.GAMMAS if full else (0.99,))
        worst = max(worst, w)
    assert buf.stored == SIZE and buf.next_index == 24
    pad = {k: v[:, buf.fields[k]:] for k, v in _rows(buf).items()}
    assert all(not p.any() for p in pad.values()) and pad["obs"].shape[1] == {60: 4 if dtype is torch.uint8 else 0, 35: 13 if dtype is torch.uint8 else 1}[H * W]
    print(f"\n{mode} {dtype} {H}x{W}: largest |rew - ref64| / tolerance = {worst:.3f}")


def test_uint8_ring_quantises_fp32_frames_as_the_reference(amd):
    """halves (ties to even), NaN, infinities, negative zero and values outside [0, 1], from the device and through the staged matrix"""
    ms, ties = R.tie_inputs()
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, -0.5, 1.5, 300.0, 0.5, 1e-9, 0.999999], np.float32)
    for H, W in ((6, 10), (5, 7)):
        vals = np.resize(np.concatenate([special, ties, np.random.default_rng(9).random(97).astype(np.float32)]), (2, E3, H, W))
        z = np.zeros((E3, 2), np.float32)
        for where in (_dev, lambda a: a):
            buf = _buffer(E3, SIZE, H, W, frame_dtype=torch.uint8)
            buf.add_vec(obs=where(vals[0]), next_obs=where(vals[1]), pobs=z, next_pobs=z, act=z, rew=z[:, :1], done=z[:, 0])
            for j, k in enumerate(FRAMES):
                got = buf.store[k][:E3].cpu().numpy()
                assert np.array_equal(got[:, :H * W], R.quantize(vals[j]).reshape(E3, -1)) and not got[:, H * W:].any(), (k, H, W)
            assert not buf.store["obs"][E3:].any()
    assert len(ms) > 100, "the ties are in the frames"


@pytest.mark.parametrize("E, size", [(4, 4), (4, 8), (1, 7)], ids=["size=E", "size=2E", "E=1"])
def test_rings_of_one_and_two_steps_and_a_single_environment(amd, E, size):
    """size == E: every walk has m = 1 (the slot is its own successor, and the newest); E = 1: add_vec is the device-side add"""
    steps = 9
    strs, d = _world(E, steps)
    for dtype in (torch.float32, torch.uint8):
        buf = _buffer(E, size, frame_dtype=dtype)
        want = ring = None
        for t in range(steps):
            want, ring = _feed(buf, d, 1, "device", t, want, ring)
            _, b = _against_truth(buf, strs, d, t, ns=(1, 3, 64), gammas=(0.99, 0.5))
            if size == E:
                assert (b["steps"] == 1).all()


# ------------------------------------------------------------------------------------------------ 2. no synchronisation
class Synchronised(AssertionError):
    pass


def _raiser(name):
    def f(*a, **k):
        raise Synchronised(name)
    return f


def test_all_device_add_vec_never_synchronises(amd, monkeypatch):
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    strs, d = _world(E3, STEPS)
    cases = [(cls, dtype, with_end) for cls in (DeviceReplayBuffer, PrioritizedDeviceReplayBuffer) for dtype in (torch.float32, torch.uint8)
             for with_end in (False, True)]
    bufs = [_buffer(E3, SIZE, cls=cls, frame_dtype=dtype) for cls, dtype, _ in cases]
    calls = []
    for t in range(3):
        kw, _ = _step(d, t, "device", False)
        calls.append((kw, _dev(d["end"][t] | (t == 1))))
    idx = _dev(np.array([1], np.int64))
    # add and add_batch with every field on the device: single-environment rings, episodes tracked so that the marks run too
    singles = [_buffer(1, SIZE, cls=cls, frame_dtype=dtype) for cls, dtype, with_end in cases if with_end]
    for s in singles:
        s.track_episodes()
    three = {k: v for k, v in calls[0][0].items() if k != "episode_end"}
    one = {k: v[0] for k, v in calls[1][0].items() if k != "episode_end"}
    torch.cuda.synchronize()

    def run():
        for buf, (_, _, with_end) in zip(bufs, cases):
            for kw, mask in calls:
                buf.add_vec(**(kw if with_end else {k: v for k, v in kw.items() if k != "episode_end"}))
                if with_end:
                    buf.on_episode_end(envs=mask)
                    buf.on_episode_end(envs=idx)
        for s in singles:
            s.add(**one)
            s.add_batch(**three)

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy"):
            m.setattr(torch.Tensor, name, _raiser(name))
        m.setattr(torch.cuda, "synchronize", _raiser("torch.cuda.synchronize"))
        m.setattr(torch.cuda.Stream, "synchronize", _raiser("Stream.synchronize"))
        m.setattr(torch.cuda.Event, "synchronize", _raiser("Event.synchronize"))
        with pytest.raises(Synchronised):
            torch.ones(1, device="cuda").item()           # the guard does raise
        run()
    # torch's own detector, where this build has one that works: the self-check decides
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            torch.ones(1, device="cuda").item()
            detects = False
        except RuntimeError:
            detects = True
        if detects:
            run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print(f"\nset_sync_debug_mode('error') raises on .item() in this build: {detects}" + (": add_vec ran under it" if detects else ""))
    torch.cuda.synchronize()
    for buf, (_, _, with_end) in zip(bufs, cases):         # and the calls did what they should
        assert buf.stored == (18 if detects else 9)
        assert (buf.episode_flags is not None) == with_end
        if with_end:
            base = buf.next_index - E3
            want = [N.HEAD | N.END if (e == 1 or d["end"][2][e]) else N.HEAD for e in range(E3)]
            assert buf.episode_flags[base:base + E3].cpu().tolist() == want
    for s in singles:                                      # one add and one add_batch of three per run
        n = 8 if detects else 4
        assert (s.stored, s.next_index) == (n, n) and s.episode_flags.cpu().tolist() == [0] * (n - 1) + [N.HEAD] + [0] * (SIZE - n)
        got = s.store["pobs"][n - 4:n, :V.PSTATE].cpu().numpy()
        assert np.array_equal(got, np.concatenate([d["pobs"][1][:1], d["pobs"][0]])), "the add's row, then the batch's three"


# ------------------------------------------------------------------------------------------------ 4. both wrap paths of the strided walk
def test_a_ring_of_more_than_64_steps_wraps_by_one_subtraction(amd):
    """E = 3, 300 slots, 105 steps: steps 100 .. 104 overwrite slots 0 .. 14, so the walks from the ring's last two steps (slots 294 ..
    299, steps 98 and 99) wrap past slot 0 into them; 63 E <= size, the subtraction path (36 slots above: the modulo path)"""
    E, size, steps = 3, 300, 105
    strs, d = _world(E, steps)
    buf = _buffer(E, size)
    for t in range(steps):
        kw, _ = _step(d, t, "device", False)
        buf.add_vec(**kw)
    assert buf.stored == size and buf.next_index == 15
    last = np.concatenate([np.arange(288, 300), np.arange(0, 18)])
    worst, _ = _against_truth(buf, strs, d, steps - 1, idx=last)
    w2, b = _against_truth(buf, strs, d, steps - 1, ns=(64,), gammas=(0.99,))
    assert int(b["steps"].max()) > 7, "long walks are in the batch"
    print(f"\n300 slots: largest |rew - ref64| / tolerance = {max(worst, w2):.3f}")


def test_stride_1_is_the_first_walk_bit_for_bit(amd):
    """dgvit_nstep_walk_strided(stride = 1) against dgvit_nstep_walk on nstep_ref's own scenario (37 slots: both take a modulo) and on a
    ring of 130 slots (both subtract), every output, clamped indices included"""
    from dgvit_amd.replay import DeviceReplayBuffer
    lib = amd.load_library()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream, ops = N.scenario()
    small = DeviceReplayBuffer(N.SIZE, obs_shape=(6, 10), seed=0)
    small.track_episodes()
    z = np.zeros(2, np.float32)
    for op in ops:
        if op[0] == "episode_end":
            small.on_episode_end()
        else:
            for t in ([op[1]] if op[0] == "add" else op[1]):
                small.add(obs=np.zeros((6, 10), np.float32), next_obs=np.zeros((6, 10), np.float32), pobs=z, act=z, next_pobs=z + t,
                          rew=stream[t][0], done=stream[t][1])
    strs, d = _world(1, 150)
    big = _buffer(1, 130)
    for t in range(150):
        kw, _ = _step(d, t, "device", False)
        big.add_vec(**kw)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for buf in (small, big):
        S = buf.size
        idx = _dev(np.concatenate([np.arange(S), [-1, S, 1 << 40]]).astype(np.int64))
        B = idx.numel()
        s = buf.store
        for n in N.NS:
            for gamma in N.GAMMAS:
                outs = []
                for strided in (False, True):
                    o = [torch.full((B,), -7.0, device="cuda") for _ in range(3)] + [torch.full((B, 4), -7.0, device="cuda"),
                                                                                      torch.full((B,), -7, dtype=torch.int32, device="cuda"),
                                                                                      torch.full((B,), -7, dtype=torch.int64, device="cuda")]
                    ring = (p(s["rew"]), 4, p(s["done"]), 4, p(buf.episode_flags), p(s["next_pobs"]), 4, p(idx), B, S)
                    fn = lib.dgvit_nstep_walk_strided if strided else lib.dgvit_nstep_walk
                    rc = fn(*ring, *((1,) if strided else ()), n, gamma, *(p(t) for t in o), st)
                    assert rc == 0, lib.dgvit_last_error()
                    outs.append(o)
                for a, b in zip(*outs):
                    assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
                assert int(outs[0][4].min()) >= 1


# ------------------------------------------------------------------------------------------------ 5. composition
def _filled(dtype=torch.float32, cls=None, steps=STEPS, **kw):
    strs, d = _world(E3, STEPS + 2)
    buf = _buffer(E3, SIZE, cls=cls, frame_dtype=dtype, **kw)
    for t in range(steps):
        buf.add_vec(**_step(d, t, "device", False)[0])
    return buf, strs, d


def test_uint8_ring_with_random_shift_and_n_step(amd):
    buf, strs, d = _filled(torch.uint8)
    idx = np.arange(SIZE)
    pad = 2
    _, b = _against_truth(buf, strs, d, STEPS - 1, ns=(3,), gammas=(0.99,), frames=False, random_shift=pad, return_shifts=True)
    pos = _positions(E3, SIZE, STEPS - 1)
    starts = [(int(pos[s]), s % E3) for s in idx]
    tails = [(V.truth(strs, e, t, STEPS - 1, 3, 0.99)[3], e) for t, e in starts]
    for k, at, stream_id in (("obs", starts, 0), ("next_obs", tails, 1)):
        np.testing.assert_array_equal(b[k + "_shift"].cpu().numpy(), RS.draw_shifts(SIZE, pad, buf.shift_seed, stream_id))
        frames = torch.from_numpy(np.stack([d[k][t, e] for t, e in at]))
        assert torch.equal(b[k].cpu(), RS.ref_shift(frames, b[k + "_shift"].cpu(), pad)), k
    assert int(b["next_obs_shift"].abs().max()) > 0


def test_prioritized_buffer(amd):
    from dgvit_amd.replay import PrioritizedDeviceReplayBuffer
    buf, strs, d = _filled(cls=PrioritizedDeviceReplayBuffer, steps=10, alpha=1.0, eps=0.0)
    assert buf.stored == 30 and np.array_equal(buf.priorities().cpu().numpy(), np.ones(30, np.float32))
    buf.update_priorities(torch.arange(30, device="cuda"), _dev(1.0 + np.arange(30, dtype=np.float32) % 5))
    buf.update_priorities(torch.tensor([4], device="cuda"), torch.tensor([9.0], device="cuda"))
    assert float(buf.max_priority) == 9.0
    for t in (10, 11):
        buf.add_vec(**_step(d, t, "device", False)[0])
    leaves = buf.priorities().cpu().numpy()
    assert buf.stored == 36 and (leaves[30:36] == 9.0).all(), "the new slots' leaves are the max priority"
    assert leaves[4] == 9.0 and np.array_equal(np.delete(leaves[:30], 4), np.delete(1.0 + np.arange(30, dtype=np.float32) % 5, 4))
    buf.add_vec(**_step(d, 12, "device", False)[0])       # wraps: slots 0 .. 2 forget their priorities
    assert (buf.priorities().cpu().numpy()[:3] == 9.0).all()
    B = 67
    u = torch.rand(B, device="cuda", generator=torch.Generator("cuda").manual_seed(6))
    drawn, weights = buf.draw(B, beta=0.7, uniforms=u)
    b = buf.sample(B, beta=0.7, uniforms=u, n_step=3, gamma=0.99)
    assert torch.equal(b["indexes"], drawn) and torch.equal(b["weights"], weights) and float(b["weights"].min()) < 1
    idx = drawn.cpu().numpy()
    _, again = _against_truth(buf, strs, d, 12, idx=idx, ns=(3,), gammas=(0.99,))
    for k in ("rew", "steps", "next_obs", "done"):
        assert torch.equal(again[k], b[k]), k
    buf.update_priorities(b["indexes"], torch.full((B,), 11.0, device="cuda"))
    assert (buf.priorities().cpu().numpy()[idx] == 11.0).all(), "the start slots took the new priority"


def test_a_captured_sample_follows_the_vector_ring(amd):
    buf, strs, d = _filled()
    idx = np.array([21, 22, 23, 24, 25, 26, 0, 35])       # the newest step is slots 21 .. 23; two more steps take it to 27 .. 29
    idx_d = _dev(idx)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            buf.sample(8, n_step=3, gamma=0.99, indices=idx_d)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = buf.sample(8, n_step=3, gamma=0.99, indices=idx_d)
    graph.replay()
    torch.cuda.synchronize()
    _, eager = _against_truth(buf, strs, d, STEPS - 1, idx=idx, ns=(3,), gammas=(0.99,))
    before = {k: v.clone() for k, v in static.items()}
    for k in eager:
        assert torch.equal(static[k], eager[k]), k
    for t in (STEPS, STEPS + 1):
        buf.add_vec(**_step(d, t, "device", False)[0])
    graph.replay()
    torch.cuda.synchronize()
    _, eager = _against_truth(buf, strs, d, STEPS + 1, idx=idx, ns=(3,), gammas=(0.99,))
    for k in eager:
        assert torch.equal(static[k], eager[k]), k
    assert not torch.equal(before["steps"], static["steps"]) or not torch.equal(before["obs"], static["obs"]), "the ring has moved on"


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(amd):
    strs, d = _world(E3, STEPS)
    buf, u8 = _buffer(E3, SIZE), _buffer(E3, SIZE, frame_dtype=torch.uint8)
    good, _ = _step(d, 0, "device", False)
    one = {k: v[0] for k, v in good.items() if k != "episode_end"}
    with pytest.raises(amd.DgvitError, match="add_vec"):
        buf.add(**one)
    with pytest.raises(amd.DgvitError, match="add_vec"):
        buf.add_batch(**{k: v for k, v in good.items() if k != "episode_end"})
    bad = {
        "act": torch.cat([good["act"], good["act"]])[:4],                    # a wrong first axis
        "pobs": good["pobs"].double(),                                       # a device tensor of the wrong dtype
        "next_pobs": good["next_pobs"].half(),
        "obs": (good["obs"] * 255).to(torch.uint8),                          # uint8 frames into an fp32 ring, from the device
        "next_obs": d["codes"]["next_obs"][0],                               # and from the host
        "rew": good["rew"].reshape(1, 3)[:, :2],
        "done": torch.zeros(3, 2, device="cuda"),
    }
    for k, v in bad.items():
        with pytest.raises(ValueError, match=rf"^{k}:"):
            buf.add_vec(**{**good, k: v})
    with pytest.raises(ValueError, match=r"^pobs:"):
        u8.add_vec(**{**good, "pobs": good["pobs"].to(torch.uint8)})         # codes are for the frame fields only
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match=r"^obs:"):
            buf.add_vec(**{**good, "obs": good["obs"].to("cuda:1")})
    else:                                                                    # one device: the other place a tensor can be is "meta"
        with pytest.raises(ValueError, match=r"^obs:"):
            buf.add_vec(**{**good, "obs": good["obs"].to("meta")})
    for end in (torch.zeros(4, device="cuda"), torch.zeros(3, dtype=torch.int64, device="cuda"), [True, False]):
        with pytest.raises(ValueError, match="episode_end"):
            buf.add_vec(**{**good, "episode_end": end})
    assert buf.stored == 0 and buf.next_index == 0 and not any(v.any() for v in buf.store.values()), "a refused call stores nothing"
    with pytest.raises(ValueError, match="envs"):
        buf.on_episode_end()
    buf.add_vec(**good)
    for envs in ([3], [-1], torch.zeros(4, dtype=torch.bool, device="cuda"), np.zeros(3, np.float32)):
        with pytest.raises(ValueError, match="envs"):
            buf.on_episode_end(envs=envs)
    single = _buffer(1, 7)
    with pytest.raises(ValueError, match="envs"):
        single.on_episode_end(envs=[0])


def test_entry_points_refuse_bad_arguments_and_launch_nothing(amd):
    """null pointer, n = 0, stride = 0 and start >= nrows on real device buffers that must stay untouched"""
    from dgvit_amd import _lib as L
    lib = amd.load_library()
    buf = _buffer(E3, SIZE)
    buf.track_episodes()
    src = torch.ones(E3, 60, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    s = buf.store

    def frames(src0=p(src), n=E3, start=0):
        return lib.dgvit_ring_store_frames(src0, 0, 60, p(src), 0, 60, p(s["obs"]), p(s["next_obs"]), 0, 60, n, 60, SIZE, start, None)

    def small(null=False, n=E3, start=0):
        f = L.dgvit_small_fields()
        for j, k in enumerate(("pobs", "act", "rew", "next_pobs", "done")):
            f.src[j], f.ring[j], f.src_ld[j], f.cols[j], f.ring_ld[j] = src.data_ptr(), s[k].data_ptr(), 60, buf.fields[k], 4
        if null:
            f.src[2] = None
        return lib.dgvit_ring_store_small(f, p(buf.episode_flags), None, 0, n, SIZE, start, None)

    out = [torch.zeros(4, device="cuda") for _ in range(3)] + [torch.zeros(4, 4, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"),
                                                               torch.zeros(4, dtype=torch.int64, device="cuda")]
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")

    def walk(rew=p(s["rew"]), stride=E3, n=3, nsel=4):
        return lib.dgvit_nstep_walk_strided(rew, 4, p(s["done"]), 4, p(buf.episode_flags), p(s["next_pobs"]), 4, p(idx), nsel, SIZE, stride, n,
                                            0.99, *(p(t) for t in out), None)

    for rc in (frames(src0=None), frames(n=0), frames(start=SIZE), small(null=True), small(n=0), small(start=SIZE + 3), walk(rew=None),
               walk(stride=0), walk(n=0), walk(nsel=0)):
        assert rc == -1, "DGVIT_ERR_ARG"
    torch.cuda.synchronize()
    assert not any(v.any() for v in s.values()) and not buf.episode_flags.any() and not any(t.any() for t in out), "nothing was launched"
    assert frames() == 0 and small() == 0 and walk() == 0
    torch.cuda.synchronize()
    assert bool((s["obs"][:E3] == 1).all()) and buf.episode_flags[:E3].tolist() == [N.HEAD] * 3 and int(out[4][0]) == 1


# ------------------------------------------------------------------------------------------------ 7. unchanged
def test_a_single_environment_buffer_that_never_uses_the_feature_is_what_it_was(amd):
    """num_envs left alone, add / add_batch / on_episode_end / sample only: the seeded draw and every batch against nstep_ref's ring"""
    from dgvit_amd.replay import DeviceReplayBuffer
    stream, ops = N.scenario()
    strs, d = _world(1, N.TOTAL)
    ring = N.offer(N.Ring(N.SIZE), stream, ops)
    for dtype in (torch.float32, torch.uint8):
        buf = DeviceReplayBuffer(N.SIZE, obs_shape=(6, 10), seed=11, frame_dtype=dtype)
        assert buf.num_envs == 1
        buf.track_episodes()
        for op in ops:
            if op[0] == "episode_end":
                buf.on_episode_end()
            elif op[0] == "add":
                buf.add(**{k: d[k][op[1], 0] for k in FIELDS})
            else:
                buf.add_batch(**{k: d[k][op[1], 0] for k in FIELDS})
        assert np.array_equal(buf.episode_flags.cpu().numpy(), ring.flags) and (buf.next_index, buf.stored) == (ring.next_index, ring.stored)
        gen = torch.Generator(device="cuda").manual_seed(11)
        want_idx = torch.randint(0, N.SIZE, (16,), device="cuda", dtype=torch.int64, generator=gen)
        one = buf.sample(16)
        assert list(one) == ["obs", "pobs", "act", "rew", "next_obs", "next_pobs", "done", "indexes"] and torch.equal(one["indexes"], want_idx)
        at = ring.pos[want_idx.cpu().numpy()]
        for k in FIELDS:
            assert np.array_equal(_bits(one[k].cpu().numpy()), _bits(d[k][at, 0])), k
        idx = np.arange(N.SIZE)
        for n, gamma in ((3, 0.99), (64, 0.5), (5, 1.0)):
            b = {k: v.cpu().numpy() for k, v in buf.sample(0, indices=_dev(idx), n_step=n, gamma=gamma).items()}
            w = ring.walk(idx, n, gamma)
            assert np.array_equal(b["steps"], w["steps"]) and np.array_equal(b["done"][:, 0], w["done"])
            assert (np.abs(b["rew"][:, 0].astype(np.float64) - w["ret64"]) <= w["tol"]).all()
            if N.exact(n, gamma):
                assert np.array_equal(_bits(b["rew"][:, 0]), _bits(w["rew"])) and np.array_equal(_bits(b["discount"][:, 0]), _bits(w["discount"]))
            assert np.array_equal(_bits(b["next_obs"]), _bits(d["next_obs"][ring.pos[w["tail"]], 0]))
            assert np.array_equal(_bits(b["next_pobs"]), _bits(d["next_pobs"][ring.pos[w["tail"]], 0]))
