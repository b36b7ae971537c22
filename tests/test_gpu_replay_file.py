"""GPU: the replay ring as a file -- save_transitions / load_transitions / clear on every ring kind, through
dgvit_ring_export and dgvit_per_set_leaves.

Every comparison is bit for bit: the export copies bits, the load goes through the store path, and the frames are k / 255, which quantise
exactly.  The file is compared with the numpy restatement tests/replay_file_ref.py, built from the streams of vec_replay_ref, nstep_ref
and shared_next_ref and their numpy rings; a loaded ring is compared with the ring that was saved by what both return: ``sample`` of every
stored slot (plain, n-step, shifted), the flags, the tree, a draw and the next indices of the restored generator -- before and after the
same further steps.  Frames are 8 x 16, 6 x 10 and 5 x 7: with one and four bytes per pixel they reach the 16-byte, the 4-byte and the
byte path of the export kernel, and 5 x 7 has a row padding in both rings."""
import functools
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import helpers as H  # noqa: E402
import nstep_ref as N  # noqa: E402
import replay_file_ref as F  # noqa: E402
import shared_next_ref as S  # noqa: E402
import vec_replay_ref as V  # noqa: E402

FIELDS, FRAMES = F.FIELDS, F.FRAMES
EXTRA = 6                                        # further steps after the load
U8, F32 = torch.uint8, torch.float32

# (shape, dtype, E, size, steps, mode, shared, prioritized).  mode: how episode ends reach the ring -- "step": add_vec(episode_end=),
# "after": on_episode_end() after the store, "ops": nstep_ref.scenario's add / add_batch / on_episode_end, "done": by done alone (the
# ring tracks, nothing is passed), "untracked": a ring that never tracked episodes.  steps < size / E: the ring has not wrapped.
CASES = [
    ((8, 16), U8, 3, 36, 20, "step", False, False),
    ((8, 16), F32, 3, 36, 7, "after", True, True),
    ((6, 10), U8, 1, 37, 52, "ops", True, False),
    ((6, 10), F32, 1, 37, 20, "ops", False, True),
    ((5, 7), U8, 3, 36, 20, "done", True, True),
    ((5, 7), F32, 3, 36, 20, "untracked", False, False),
    ((5, 7), U8, 1, 37, 52, "ops", False, True),
    ((5, 7), F32, 1, 37, 52, "ops", True, False),
    ((6, 10), U8, 3, 36, 20, "after", False, True),
    ((6, 10), F32, 3, 36, 20, "step", True, False),
    ((8, 16), F32, 1, 37, 45, "step", False, False),
    ((8, 16), U8, 1, 37, 20, "done", True, True),
    ((5, 7), U8, 3, 36, 7, "untracked", False, True),
    ((5, 7), F32, 3, 36, 20, "step", True, True),
]


def _id(c):
    shape, dtype, E, size, steps, mode, shared, per = c
    return f"{shape[0]}x{shape[1]}-{'u8' if dtype is U8 else 'fp32'}-E{E}-{size}-{steps}-{mode}-{'shared' if shared else 'plain'}-{'per' if per else 'uni'}"


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


def _classes():
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    return {False: DeviceReplayBuffer, True: PrioritizedDeviceReplayBuffer}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _world(E, total, shape, mode):
    """(streams, ops or None, frame ids, data), computed once per key and left unchanged"""
    if mode == "ops":
        stream, ops = N.scenario(total=total)
        strs = [stream]
    else:
        strs, ops = V.streams(E, total), None
        if mode in ("done", "untracked"):
            strs = F.without_ends(strs)
    frs = S.all_frames(strs)
    return strs, ops, frs, F.data(strs, frs, shape)


def _phases(ops, steps):
    """the ops that offer stream positions below `steps` (with the episode_end that follows them), and the rest"""
    k = 0
    for j, op in enumerate(ops):
        if op[0] != "episode_end" and (op[1] if op[0] == "add" else op[1][0]) < steps:
            k = j + 1
    if k < len(ops) and ops[k][0] == "episode_end":
        k += 1
    return ops[:k], ops[k:]


def _make(case, seed=3, size=None, **over):
    shape, dtype, E, size0, steps, mode, shared, per = case
    kw = dict(obs_shape=shape, pstate_dim=V.PSTATE, act_dim=V.ACT, seed=seed, frame_dtype=dtype, num_envs=E)
    size = size0 if size is None else size
    if shared:
        kw.update(shared_next_obs=True, terminal_frames=size)     # a pool that cannot overflow
    kw.update(over)
    return _classes()[per](size, **kw)


def _ref(case, P=None):
    shape, dtype, E, size, steps, mode, shared, per = case
    if shared:
        return S.SharedRing(E, size, size if P is None else P)
    if mode == "ops":
        return N.Ring(size)
    return V.VecRing(E, size, tracked=mode != "untracked")


def _step_kw(d, ts, u8, squeeze, t):
    f = {k: (d[k][ts, 0] if squeeze else d[k][ts]) for k in FIELDS}
    if u8 and t % 2:                                 # the ring's own codes now and then
        for k in FRAMES:
            f[k] = d["codes"][k][ts, 0] if squeeze else d["codes"][k][ts]
    return f


def _feed(case, bufs, ref, lo, hi):
    """steps [lo, hi) of the case's world (the ops that offer those positions) into the device rings and the numpy ring"""
    shape, dtype, E, size, steps, mode, shared, per = case
    strs, ops, frs, d = _world(E, steps + EXTRA, shape, mode)
    u8 = dtype is U8
    if mode == "ops":
        first, rest = _phases(ops, steps)
        for j, op in enumerate(first if lo == 0 else rest):
            for buf in bufs:
                if op[0] == "episode_end":
                    buf.on_episode_end()
                elif op[0] == "add":
                    buf.add(**_step_kw(d, op[1], u8, True, j))
                else:
                    buf.add_batch(**_step_kw(d, op[1], u8, True, j))
            if ref is not None:
                ts = None if op[0] == "episode_end" else ([op[1]] if op[0] == "add" else op[1])
                if ts is None:
                    ref.episode_end(np.array([True])) if shared else ref.episode_end()
                elif shared:
                    ref.store(strs[0], frs[0], ts)
                else:
                    ref.store([strs[0][t][0] for t in ts], [strs[0][t][1] for t in ts], ts)
        return
    for t in range(lo, hi):
        for buf in bufs:
            kw = _step_kw(d, t, u8, False, t)
            if mode == "step":
                buf.add_vec(**kw, episode_end=_dev(d["end"][t]) if t % 2 else d["end"][t])
            else:
                buf.add_vec(**kw)
                if mode == "after":
                    if E > 1:
                        buf.on_episode_end(envs=d["end"][t])
                    elif d["end"][t][0]:
                        buf.on_episode_end()
        if ref is not None:
            if shared:
                ref.add_vec_frames(strs, frs, t)
            else:
                ref.add_vec([s[t][0] for s in strs], [s[t][1] for s in strs], t, None if mode == "untracked" else [s[t][2] for s in strs])


def _built(case, n=1, ref=True, P=None, **over):
    """n device rings of the case after its first `steps` steps (same seed, same calls), and the numpy ring"""
    shape, dtype, E, size, steps, mode, shared, per = case
    bufs = [_make(case, **over) for _ in range(n)]
    ring = _ref(case, P) if ref else None
    if mode != "untracked" and not shared:
        for b in bufs:
            b.track_episodes()
    _feed(case, bufs, ring, 0, steps)
    if per:                                          # leaves that are not all the max leaf, a max leaf above 1, a used header word 1
        g = torch.Generator(device="cuda").manual_seed(7)
        for _ in range(2):
            idx = torch.randint(0, bufs[0].stored, (24,), device="cuda", generator=g)
            prio = torch.rand(24, device="cuda", generator=g) * 3
            for b in bufs:
                b.update_priorities(idx, prio)
    return bufs, ring


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (k, what)
        if x.dtype == torch.float32:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), (k, what)


def _base_sample(buf, idx, **kw):
    torch.manual_seed(11)                            # the shift seed's source
    return _classes()[False].sample(buf, idx.numel(), indices=idx, **kw)


def _equal_rings(a, b, what, tracked=True, draws=True):
    """two rings are the same to their user: counters, flags, every stored slot's sample, the tree, a draw, the generator"""
    assert (a.next_index, a.stored) == (b.next_index, b.stored), what
    assert (a.episode_flags is None) == (b.episode_flags is None), what
    if a.episode_flags is not None:
        assert torch.equal(a.episode_flags, b.episode_flags), what
    idx = torch.arange(a.stored, device="cuda")
    calls = [dict(), dict(random_shift=2, return_shifts=True)] + ([dict(n_step=3, gamma=0.5)] if tracked else [])
    for kw in calls:
        _same(_base_sample(a, idx, **kw), _base_sample(b, idx, **kw), (what, kw))
    if hasattr(a, "tree"):
        assert torch.equal(a.tree.view(torch.int32), b.tree.view(torch.int32)), what
        u = torch.rand(8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
        (ia, wa), (ib, wb) = a.draw(8, 0.7, uniforms=u), b.draw(8, 0.7, uniforms=u)
        assert torch.equal(ia, ib) and torch.equal(wa.view(torch.int32), wb.view(torch.int32)), what
    if draws:
        assert torch.equal(a.sample(8)["indexes"], b.sample(8)["indexes"]), (what, "the generator")


def _files(path):
    out = {k: np.load(os.path.join(path, k + ".npy"), mmap_mode="r") for k in (*FIELDS, "end")}
    if os.path.exists(os.path.join(path, "priority.npy")):
        out["priority"] = np.load(os.path.join(path, "priority.npy"), mmap_mode="r")
    return out


def _meta(path):
    with open(os.path.join(path, "meta.json")) as f:
        return json.load(f)


def _bits(x):
    return int(np.float32(x).view(np.int32))


# ------------------------------------------------------------------------------------------------ 1. the file
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_file_is_the_restatements(amd, case, tmp_path):
    shape, dtype, E, size, steps, mode, shared, per = case
    (buf,), ring = _built(case)
    u8 = dtype is U8
    small, big = str(tmp_path / "chunk5"), str(tmp_path / "chunk4096")
    odd = 5 if buf.stored % 5 else 7                 # a chunk that does not divide the stored count and straddles the wrap
    buf.save_transitions(small, chunk=odd)
    buf.save_transitions(big)
    assert sorted(os.listdir(tmp_path)) == ["chunk4096", "chunk5"], "no temporary directory is left"
    names = sorted(os.listdir(big))
    assert names == sorted([k + ".npy" for k in (*FIELDS, "end", "rng")] + ["meta.json"] + (["priority.npy"] if per else []))
    for name in names:
        with open(os.path.join(small, name), "rb") as f, open(os.path.join(big, name), "rb") as g:
            assert f.read() == g.read(), name
    assert (buf.next_index, buf.stored) == (ring.next_index, ring.stored) and ring.stored % odd
    want, got = F.expected(ring, d=_world(E, steps + EXTRA, shape, mode)[3], shape=shape, u8=u8), _files(big)
    for k in (*FIELDS, "end"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(np.asarray(got[k]).view(np.uint8), want[k].view(np.uint8)), k
    assert got["obs"].dtype == (np.uint8 if u8 else np.float32) and got["obs"].shape == (ring.stored, *shape)
    slots = F.ages(ring)[0]
    assert got["end"].any() == (mode in ("step", "after", "ops")), "the scenario has episode ends, unless they are left to done"
    assert np.asarray(got["done"]).any() or ring.stored < size
    meta = _meta(big)
    assert tuple(meta) == F.META_KEYS
    header = buf.tree[:2].cpu().numpy() if per else None
    assert meta == {
        "format_version": 1, "stored": ring.stored, "size": size, "num_envs": E, "oldest_slot": int(slots[0]), "next_index": ring.next_index,
        "obs_shape": list(shape), "pstate_dim": V.PSTATE, "act_dim": V.ACT, "frame_dtype": "uint8" if u8 else "float32",
        "shared_next_obs": shared, "terminal_frames": size if shared else None, "lost_terminal_frames": 0,
        "episodes_tracked": mode != "untracked", "prioritized": per, "alpha": 0.6 if per else None, "eps": 1e-4 if per else None,
        "max_leaf_bits": _bits(header[0]) if per else None, "update_max_bits": _bits(header[1]) if per else None}
    assert np.array_equal(np.load(os.path.join(big, "rng.npy")), buf.gen.get_state().numpy())
    if per:
        leaves = buf.tree[64:64 + size].cpu().numpy()[slots]
        assert got["priority"].dtype == np.float32 and np.array_equal(np.asarray(got["priority"]).view(np.int32), leaves.view(np.int32))
        assert (leaves > 0).all() and len(np.unique(leaves)) > 4 and header[0] > 1 and header[1] >= 1


# ------------------------------------------------------------------------------------------------ 2., 3. the round trip, and going on
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_a_same_geometry_load_resumes_the_ring(amd, case, tmp_path):
    shape, dtype, E, size, steps, mode, shared, per = case
    (src,), _ = _built(case, ref=False)
    path = str(tmp_path / "ring")
    src.save_transitions(path, chunk=7)
    dst = _make(case, seed=99)                       # another seed: the generator must come from the file
    assert dst.load_transitions(path) == src.stored
    tracked = mode != "untracked"
    assert (dst.episode_flags is None) == (not tracked)
    _equal_rings(src, dst, "loaded", tracked)
    if shared:
        assert dst.lost_terminal_frames() == 0
    _feed(case, [src, dst], None, steps, steps + EXTRA)
    _equal_rings(src, dst, "after the same further steps", tracked)


# ------------------------------------------------------------------------------------------------ 4. too small a pool
@pytest.mark.parametrize("dtype", [F32, U8], ids=["fp32", "u8"])
def test_a_lost_terminal_frame_is_saved_as_the_slots_own_obs(amd, dtype, tmp_path):
    case = ((6, 10), dtype, 3, 36, 20, "step", True, False)      # test_shared_next_host.py's scenario, which overflows a pool of 2
    (src,), ring = _built(case, P=2, terminal_frames=2)
    assert ring.lost > 0 and src.lost_terminal_frames() == ring.lost
    path = str(tmp_path / "ring")
    src.save_transitions(path, chunk=5)
    got, slots = _files(path), F.ages(ring)[0]
    assert _meta(path)["lost_terminal_frames"] == ring.lost and _meta(path)["terminal_frames"] == 2
    out = src.sample(len(slots), indices=_dev(slots))
    for k in FRAMES:
        mine = np.asarray(got[k])
        mine = mine.astype(np.float32) / np.float32(255.0) if dtype is U8 else mine
        assert np.array_equal(mine.view(np.int32), out[k].cpu().numpy().view(np.int32)), k
    want = F.expected(ring, _world(3, 20 + EXTRA, (6, 10), "step")[3], (6, 10), dtype is U8)
    assert np.array_equal(np.asarray(got["next_obs"]), want["next_obs"])
    lost = ring.next_row[slots] == slots
    assert 0 < lost.sum() <= ring.lost and np.array_equal(np.asarray(got["next_obs"])[lost], np.asarray(got["obs"])[lost])


# ------------------------------------------------------------------------------------------------ 5. across formats
OPS_U8 = ((6, 10), U8, 1, 37, 52, "ops", False, False)
OPS_F32 = ((5, 7), F32, 1, 37, 52, "ops", False, False)
VEC_U8 = ((5, 7), U8, 3, 36, 20, "step", False, False)


def _resaved(buf, tmp_path, name):
    path = str(tmp_path / name)
    buf.save_transitions(path, chunk=11)
    return _files(path)


def _same_files(a, b, what, keys=(*FIELDS, "end"), tail=None):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        x = x if tail is None else x[-tail:]
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (k, what)


@pytest.mark.parametrize("case", [OPS_U8, VEC_U8], ids=_id)
@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared"])
def test_a_uint8_file_into_an_fp32_ring_stores_codes_over_255(amd, case, shared, tmp_path):
    (src,), _ = _built(case, ref=False)
    path = str(tmp_path / "ring")
    src.save_transitions(path)
    dst = _make(case[:1] + (F32,) + case[2:6] + (shared, False))
    dst.load_transitions(path)
    got = _files(path)
    idx = torch.arange(dst.stored, device="cuda")
    a, b = _base_sample(src, idx), _base_sample(dst, idx)
    _same(a, b, "the fp32 ring returns what the uint8 ring returns")
    slots = (_meta(path)["oldest_slot"] + np.arange(dst.stored)) % dst.size
    for k in FRAMES:
        want = np.asarray(got[k]).astype(np.float32) / np.float32(255.0)
        assert np.array_equal(b[k].cpu().numpy()[slots].view(np.int32), want.view(np.int32)), k
    assert torch.equal(dst.store["obs"][_dev(slots), :dst.fields["obs"]].cpu(), torch.from_numpy(np.asarray(got["obs"]).astype(np.float32)
                                                                                                 .reshape(len(slots), -1) / np.float32(255.0)))


@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared"])
def test_an_fp32_file_of_k_over_255_into_a_uint8_ring_stores_the_codes(amd, shared, tmp_path):
    case = OPS_F32
    (src,), ring = _built(case)
    path = str(tmp_path / "ring")
    src.save_transitions(path)
    dst = _make(case[:1] + (U8,) + case[2:6] + (shared, False))
    dst.load_transitions(path)
    codes = F.expected(ring, _world(1, 52 + EXTRA, (5, 7), "ops")[3], (5, 7), True)
    slots = F.ages(ring)[0]
    assert torch.equal(dst.store["obs"][_dev(slots), :35].cpu(), torch.from_numpy(codes["obs"].reshape(len(slots), -1)))
    assert (dst.store["obs"][:, 35:] == 0).all()
    idx = torch.arange(dst.stored, device="cuda")
    _same(_base_sample(src, idx), _base_sample(dst, idx), "k / 255 quantises exactly")
    back = _resaved(dst, tmp_path, "back")
    for k in FRAMES:
        assert back[k].dtype == np.uint8 and np.array_equal(np.asarray(back[k]), codes[k]), k


@pytest.mark.parametrize("case", [OPS_U8, OPS_F32, VEC_U8], ids=_id)
def test_plain_to_shared_and_shared_to_plain_agree_by_age(amd, case, tmp_path):
    (src,), _ = _built(case, ref=False)
    first = _resaved(src, tmp_path, "plain")
    shared = _make(case[:6] + (True, False), seed=1)
    shared.load_transitions(str(tmp_path / "plain"))
    assert shared.lost_terminal_frames() == 0
    second = _resaved(shared, tmp_path, "shared")
    _same_files(first, second, "plain -> shared")
    plain = _make(case, seed=2)
    plain.load_transitions(str(tmp_path / "shared"))
    _same_files(first, _resaved(plain, tmp_path, "plain2"), "shared -> plain")
    _equal_rings(src, plain, "shared -> plain", draws=False)


@pytest.mark.parametrize("per", [False, True], ids=["uni", "per"])
@pytest.mark.parametrize("shared", [False, True], ids=["plain", "shared"])
@pytest.mark.parametrize("case", [OPS_U8, OPS_F32], ids=_id)
def test_a_smaller_ring_keeps_the_newest_and_a_larger_one_appends(amd, case, shared, per, tmp_path):
    (src,), _ = _built(case, ref=False)
    first = _resaved(src, tmp_path, "src")
    path = str(tmp_path / "src")
    kind = case[:6] + (shared, per)
    small = _make(kind, size=20)
    assert small.load_transitions(path) == 37 and small.stored == 20
    _same_files(first, _resaved(small, tmp_path, "small"), "the newest 20", tail=20)
    large = _make(kind, size=64, seed=8)
    before = large.gen.get_state()
    assert large.load_transitions(path) == 37 and (large.stored, large.next_index) == (37, 37)
    assert torch.equal(large.gen.get_state(), before), "another geometry: the generator stays"
    _same_files(first, _resaved(large, tmp_path, "large"), "all of them")
    large.load_transitions(path)
    assert (large.stored, large.next_index) == (64, 10)
    twice = {k: np.concatenate([np.asarray(first[k])] * 2) for k in first}
    twice["end"][36] |= 1                            # what was there does not go on into the file: the load ends its episode
    _same_files(twice, _resaved(large, tmp_path, "twice"), "a second load appends", tail=64)
    forced = _make(kind, size=64, seed=8)
    forced.load_transitions(path, restore_rng=True)
    assert torch.equal(forced.gen.get_state(), src.gen.get_state())
    same = _make(case, seed=8)
    same.load_transitions(path, restore_rng=False)
    assert torch.equal(same.gen.get_state(), before)


# ------------------------------------------------------------------------------------------------ 6. priorities
PER = ((5, 7), U8, 3, 36, 20, "step", False, True)
PER_OPS = ((6, 10), F32, 1, 37, 52, "ops", True, True)


@pytest.mark.parametrize("case", [PER, PER_OPS], ids=_id)
def test_priorities_reset_other_parameters_and_rings_without_a_tree(amd, case, tmp_path):
    (src,), _ = _built(case, ref=False)
    path = str(tmp_path / "ring")
    src.save_transitions(path)
    idx = torch.arange(src.stored, device="cuda")
    reset = _make(case, seed=4)
    reset.load_transitions(path, priorities="reset")
    assert (reset.priorities() == 1).all() and float(reset.max_priority) == 1.0, "every leaf at the max leaf of a new ring"
    _same(_base_sample(src, idx), _base_sample(reset, idx), "reset changes the leaves alone")
    for over, word in ((dict(alpha=0.5), "alpha"), (dict(eps=1e-3), "eps")):
        other = _make(case, **over)
        frames = other.store["obs"].clone()
        with pytest.raises(ValueError, match=word):
            other.load_transitions(path)
        assert other.stored == 0 and other.next_index == 0 and torch.equal(other.store["obs"], frames)
        other.load_transitions(path, priorities="reset")     # the leaves are powers; the transitions are not
        assert other.stored == src.stored
    plain = _make(case[:7] + (False,))
    plain.load_transitions(path)
    _same(_base_sample(src, idx), _base_sample(plain, idx), "a prioritized file into a plain ring")
    assert not hasattr(plain, "tree")
    again = str(tmp_path / "plain")
    plain.save_transitions(again)
    assert not os.path.exists(os.path.join(again, "priority.npy")) and _meta(again)["prioritized"] is False
    back = _make(case, seed=4)
    back.load_transitions(again)
    assert (back.priorities() == 1).all(), "a plain file into a prioritized ring: the max leaf everywhere"
    assert torch.equal(back.tree.view(torch.int32), reset.tree.view(torch.int32))
    _same(_base_sample(src, idx), _base_sample(back, idx), "a plain file into a prioritized ring")
    os.remove(os.path.join(path, "priority.npy"))
    bare = _make(case, seed=4)
    bare.load_transitions(path)
    assert torch.equal(bare.tree.view(torch.int32), reset.tree.view(torch.int32)), "no priority.npy: like reset"


def test_leaves_loaded_across_the_ring_end_and_into_a_deep_tree(amd, tmp_path):
    """a ring of 4100 slots has a three-level tree; loaded into one of 5000 at next_index 4000 the leaves wrap: two
    dgvit_per_set_leaves calls per chunk, and the rebuilt tree is that of the same leaves written by update_priorities"""
    from dgvit_amd.replay import PrioritizedDeviceReplayBuffer as P
    n, shape = 4100, (5, 7)
    g = np.random.default_rng(3)
    kw = dict(obs=g.integers(0, 256, (n, 5, 7)).astype(np.uint8), next_obs=g.integers(0, 256, (n, 5, 7)).astype(np.uint8),
              pobs=g.standard_normal((n, 2)).astype(np.float32), act=g.standard_normal((n, 2)).astype(np.float32),
              rew=g.standard_normal((n, 1)).astype(np.float32), next_pobs=g.standard_normal((n, 2)).astype(np.float32),
              done=(g.random((n, 1)) < 0.05).astype(np.float32))
    src = P(n, obs_shape=shape, frame_dtype=U8, seed=1)
    src.add_batch(**kw)
    prio = torch.rand(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 5
    src.update_priorities(torch.arange(n, device="cuda"), prio)
    path = str(tmp_path / "ring")
    src.save_transitions(path, chunk=1000)
    same = P(n, obs_shape=shape, frame_dtype=U8, seed=2)
    same.load_transitions(path)
    assert torch.equal(same.tree.view(torch.int32), src.tree.view(torch.int32))
    dst, ref = (P(5000, obs_shape=shape, frame_dtype=U8, seed=2) for _ in range(2))
    filler = {k: v[:4000] for k, v in kw.items()}
    for b in (dst, ref):
        b.add_batch(**filler)
    dst.load_transitions(path)
    ref.add_batch(**kw)
    slots = (4000 + torch.arange(n, device="cuda")) % 5000
    ref.update_priorities(slots, prio)
    assert (dst.next_index, dst.stored) == (ref.next_index, ref.stored) == (3100, 5000)
    assert torch.equal(dst.tree[2:].view(torch.int32), ref.tree[2:].view(torch.int32)), "leaves and every ancestor"
    assert float(dst.max_priority) == float(src.max_priority) == float(ref.max_priority)
    idx = torch.arange(5000, device="cuda")
    _same(_base_sample(dst, idx), _base_sample(ref, idx), "the transitions across the ring's end")


# ------------------------------------------------------------------------------------------------ 7. refusals
def _untouched(buf, frames):
    assert buf.stored == 0 and buf.next_index == 0 and torch.equal(buf.store["obs"], frames["obs"])
    assert buf.shared_next_obs or torch.equal(buf.store["next_obs"], frames["next_obs"])


def test_a_file_that_does_not_fit_is_refused_before_anything_is_stored(amd, tmp_path):
    case = ((6, 10), U8, 3, 36, 20, "step", False, False)
    (src,), _ = _built(case, ref=False)
    path = str(tmp_path / "ring")
    src.save_transitions(path)
    from dgvit_amd.replay import DeviceReplayBuffer as B
    base = dict(obs_shape=(6, 10), pstate_dim=2, act_dim=2, frame_dtype=U8, num_envs=3)
    for over, word in ((dict(num_envs=1), "num_envs"), (dict(num_envs=4), "num_envs"), (dict(obs_shape=(5, 12)), "obs_shape"),
                       (dict(obs_shape=(10, 6)), "obs_shape"), (dict(pstate_dim=3), "pstate_dim"), (dict(act_dim=1), "act_dim")):
        for shared in (False, True):
            buf = B(36, **{**base, **over}, shared_next_obs=shared)
            frames = {k: v.clone() for k, v in buf.store.items()}
            with pytest.raises(ValueError, match=word):
                buf.load_transitions(path)
            _untouched(buf, frames)
    buf = B(36, **base)
    frames = {k: v.clone() for k, v in buf.store.items()}
    for name in ("act.npy", "next_obs.npy", "end.npy", "meta.json"):
        broken = str(tmp_path / ("without_" + name))
        shutil.copytree(path, broken)
        os.remove(os.path.join(broken, name))
        with pytest.raises(FileNotFoundError, match=name):
            buf.load_transitions(broken)
        _untouched(buf, frames)
    for version in (0, 2, "1", None):
        other = str(tmp_path / f"version_{version}")
        shutil.copytree(path, other)
        meta = _meta(path)
        meta["format_version"] = version
        with open(os.path.join(other, "meta.json"), "w") as f:
            json.dump(meta, f)
        with pytest.raises(ValueError, match="format_version"):
            buf.load_transitions(other)
        _untouched(buf, frames)
    short = str(tmp_path / "short")
    shutil.copytree(path, short)
    np.save(os.path.join(short, "rew.npy"), np.zeros((35, 1), np.float32))
    with pytest.raises(ValueError, match="rew.npy"):
        buf.load_transitions(short)
    _untouched(buf, frames)
    assert buf.load_transitions(path) == 36, "and the file itself loads"


def test_save_refuses_an_existing_path_an_empty_ring_and_a_capture(amd, tmp_path):
    case = ((6, 10), U8, 3, 36, 20, "step", False, False)
    (src,), _ = _built(case, ref=False)
    path = str(tmp_path / "ring")
    src.save_transitions(path)
    before = {n: open(os.path.join(path, n), "rb").read() for n in os.listdir(path)}
    _feed(case, [src], None, 20, 22)
    with pytest.raises(FileExistsError, match="overwrite"):
        src.save_transitions(path)
    assert {n: open(os.path.join(path, n), "rb").read() for n in os.listdir(path)} == before and os.listdir(tmp_path) == ["ring"]
    src.save_transitions(path, overwrite=True)
    assert open(os.path.join(path, "obs.npy"), "rb").read() != before["obs.npy"] and os.listdir(tmp_path) == ["ring"]
    empty = _make(case)
    with pytest.raises(RuntimeError, match="empty"):
        empty.save_transitions(str(tmp_path / "empty"))
    with pytest.raises(RuntimeError, match="empty"):
        empty.save_transitions(path, overwrite=True)
    assert os.listdir(tmp_path) == ["ring"] and _meta(path)["stored"] == 36
    idx = torch.arange(36, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            src.sample(36, indices=idx)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        src.sample(36, indices=idx)
        with pytest.raises(amd.DgvitError, match="capture"):
            src.save_transitions(str(tmp_path / "captured"))
        with pytest.raises(amd.DgvitError, match="capture"):
            empty.load_transitions(path)
    assert os.listdir(tmp_path) == ["ring"] and empty.stored == 0


# ------------------------------------------------------------------------------------------------ 8. clear()
@pytest.mark.parametrize("case", [CASES[4], CASES[2], CASES[8], CASES[5]], ids=_id)
def test_a_cleared_ring_is_a_new_ring(amd, case, tmp_path):
    shape, dtype, E, size, steps, mode, shared, per = case
    (buf, twin), _ = _built(case, n=2, ref=False)
    path = str(tmp_path / "ring")
    buf.save_transitions(path)
    frames = buf.store["obs"].clone()
    pointers = {k: v.data_ptr() for k, v in buf.store.items()}
    buf.clear()
    assert buf.stored == 0 and buf.next_index == 0 and {k: v.data_ptr() for k, v in buf.store.items()} == pointers
    assert torch.equal(buf.store["obs"], frames), "the frame matrices are not touched"
    with pytest.raises(RuntimeError, match="empty"):
        buf.sample(4)
    with pytest.raises(RuntimeError, match="empty"):
        buf.save_transitions(str(tmp_path / "none"))
    fresh = _make(case)
    if mode != "untracked":
        assert buf.episode_flags is not None and not buf.episode_flags.any()
    if shared:
        assert (buf.next_row == -1).all() and buf._pool_state.tolist() == [0, 0, 0]
    if per:
        assert torch.equal(buf.tree.view(torch.int32), fresh.tree.view(torch.int32))
    buf.load_transitions(path)
    _equal_rings(twin, buf, "cleared and loaded", mode != "untracked")
    _feed(case, [twin, buf], None, steps, steps + EXTRA)
    _equal_rings(twin, buf, "and fed the same further steps", mode != "untracked")


# ------------------------------------------------------------------------------------------------ 9. past 4 GiB
def test_export_reads_a_frame_matrix_past_4_gib(amd):
    """a uint8 ring of 128 x 160 frames whose matrices are 4.0014 GiB each: known rows at slot 0, on either side of byte 2^31 and of byte
    2^32 and at the last slot, exported chunk by chunk (nothing goes to disk)"""
    from dgvit_amd import replay
    shape, row = (128, 160), 128 * 160
    size = (1 << 32) // row + 70
    assert size * row > (1 << 32) + 64 * row
    H.need_device_memory(2 * size * row + (1 << 28))
    buf = replay.DeviceReplayBuffer(size, obs_shape=shape, frame_dtype=U8)
    marks = [0, size - 1]
    for b in (1 << 31, 1 << 32):
        marks += [b // row - 1, b // row, b // row + 1]          # the row that holds byte b and its neighbours
    g = torch.Generator(device="cuda").manual_seed(9)
    at = torch.tensor(marks, device="cuda")
    known = {k: torch.randint(0, 256, (len(marks), row), dtype=U8, device="cuda", generator=g) for k in FRAMES}
    for k in FRAMES:
        buf.store[k][at] = known[k]
    buf.store["rew"][at, 0] = at.float()
    buf.stored, buf.next_index = size, 0
    chunks = [(0, 1), (size - 1, 1)] + [(b // row - 1, 3) for b in (1 << 31, 1 << 32)]
    for a0, n in chunks:
        out = buf._export_chunk(a0, n)
        blocks, total = replay.export_layout(n, shape, 2, 2, U8)
        assert out.numel() == total and out.dtype == U8
        rows = [marks.index(a0 + j) for j in range(n)]
        for k in FRAMES:
            off, nb = blocks[k]
            assert torch.equal(out[off:off + nb].view(n, row), known[k][rows]), (k, a0)
        off, nb = blocks["rew"]
        assert out[off:off + nb].view(torch.float32).tolist() == [float(a0 + j) for j in range(n)]
    buf.next_index = 5                               # a full ring whose oldest slot is 5: age a0 lies in slot a0 + 5, and wraps
    out = buf._export_chunk(size - 6, 2)
    blocks = replay.export_layout(2, shape, 2, 2, U8)[0]
    for k in FRAMES:
        off, nb = blocks[k]
        assert torch.equal(out[off:off + nb].view(2, row), known[k][[1, 0]]), k
