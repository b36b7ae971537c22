"""GPU: prioritized replay on the device -- the radix-64 sum / min tree (dgvit_per_*) and replay.PrioritizedDeviceReplayBuffer.

The reference is never the code under test: tests/prioritized_replay_ref.py restates leaves, selection and weights in numpy fp64.  The
exact tests use alpha = 1, eps = 0 and integer priorities in [1, 16] whose total is a power of two, with uniforms (m + 0.5) / total: every
sum, product and difference the kernel forms is then exact in fp32 in any order, so its indices must EQUAL the restatement's.  Frames are
4 x 4: only the tree is under test."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import prioritized_replay_ref as R  # noqa: E402
import replay_shift_ref as S  # noqa: E402

H, W = 4, 4
EDGE_U = [0.0, 1.0 - 2.0 ** -24, 1.0]


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def _buffer(size, stored, alpha=1.0, eps=0.0, seed=0, frames=False):
    """a buffer of `size` slots with `stored` transitions added in one add_batch (every leaf 1 = the initial max priority)"""
    from dgvit_amd.replay import PrioritizedDeviceReplayBuffer
    buf = PrioritizedDeviceReplayBuffer(size, obs_shape=(H, W), seed=seed, alpha=alpha, eps=eps)
    if stored:
        _add(buf, stored, 0, frames)
    return buf


def _add(buf, n, base=0, frames=False):
    obs = torch.zeros(n, H, W)
    if frames:
        obs = (base + torch.arange(n * H * W, dtype=torch.float32)).reshape(n, H, W)
    col = (base + torch.arange(n, dtype=torch.float32))[:, None]
    buf.add_batch(obs=obs, next_obs=-obs - 1, pobs=col.repeat(1, 2), next_pobs=col.repeat(1, 2) + 0.5, act=-col.repeat(1, 2), rew=col,
                  done=torch.zeros(n, 1))


def _set(buf, idx, prio):
    buf.update_priorities(_dev(np.asarray(idx), torch.int64), _dev(np.asarray(prio, dtype=np.float32), torch.float32))


def _leaves(buf):
    return buf.priorities().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. exact selection
def _exact_uniforms(total, limit=40000):
    """(m + 0.5) / total for every integer m (a stride of them, and the last, above `limit`), then u = 0, 1 - 2^-24 and 1"""
    m = np.arange(total, dtype=np.float64)
    if total > limit:
        m = np.unique(np.concatenate([m[::total // limit + 1], m[-3:]]))
    u = np.concatenate([(m + 0.5) / total, EDGE_U]).astype(np.float32)
    assert ((u[:-3].astype(np.float64) * total) == m + 0.5).all(), "the masses must be exact in fp32"
    return u


def _raw_tree(capacity, slots, prio):
    """a tree built through the C entry points alone: only `slots` are ever written, so every other leaf is 0 (never stored)"""
    from dgvit_amd import _lib as L
    lib = L.load()
    tree = torch.full((lib.dgvit_per_tree_floats(capacity),), float("nan"), device="cuda")
    L.check(lib.dgvit_per_init(_p(tree), capacity, _st()), "dgvit_per_init")
    idx, pr = _dev(np.asarray(slots), torch.int64), _dev(np.asarray(prio, dtype=np.float32), torch.float32)
    L.check(lib.dgvit_per_update(_p(tree), capacity, capacity, _p(idx), _p(pr), idx.numel(), 1.0, 0.0, _st()), "dgvit_per_update")
    return tree


def _raw_sample(tree, capacity, u, beta=1.0, stratified=0):
    from dgvit_amd import _lib as L
    ud = _dev(u, torch.float32)
    idx = torch.full((ud.numel(),), -7, dtype=torch.int64, device="cuda")
    w = torch.full((ud.numel(),), float("nan"), device="cuda")
    L.check(L.load().dgvit_per_sample(_p(tree), capacity, _p(ud), ud.numel(), stratified, beta, _p(idx), _p(w), _st()), "dgvit_per_sample")
    return idx.cpu().numpy(), w.cpu().numpy().astype(np.float64)


BOUNDARY_SLOTS = [0, 1, 62, 63, 64, 65, 127, 128, 4095, 4096, 4097, 4159, 4160, 4999, 262143, 262144]


@pytest.mark.parametrize("capacity", [1, 63, 64, 65, 4096, 4097, 5000, 262145])
def test_exact_selection_on_sparse_trees(amd, capacity):
    """Only the slots around the block and level boundaries are written; slot 0 and the last slot are left at 0 whenever the tree has
    more than two slots, so zero leaves lead and trail.  For 262145 (four levels) the slots are 0, 63, 64, 4095, 4096, 262143, 262144."""
    if capacity == 262145:
        slots = [0, 63, 64, 4095, 4096, 262143, 262144]
    else:
        slots = sorted({s for s in BOUNDARY_SLOTS + [capacity // 2, capacity - 2] if 0 < s < capacity - 1}) or [0]
    prio = R.power_of_two_priorities(len(slots), capacity)
    leaf = np.zeros(capacity)
    leaf[slots] = prio
    total = leaf.sum()
    tree = _raw_tree(capacity, slots, prio)
    u = _exact_uniforms(int(total))
    idx, w = _raw_sample(tree, capacity, u)
    want = R.select(leaf, R.masses(u.astype(np.float64), total))
    np.testing.assert_array_equal(idx, want)
    assert set(idx.tolist()) == set(slots), "every written slot is reached, nothing else"
    assert (leaf[idx[-3:]] > 0).all() and idx[-3] == slots[0] and idx[-2] == slots[-1] and idx[-1] == slots[-1]
    np.testing.assert_allclose(w, R.weights(leaf, want, 1.0), rtol=1e-5)
    # the header's max leaf and the top block agree with the leaves
    assert float(tree[0]) == max(1.0, prio.max())


@pytest.mark.parametrize("capacity", [1, 63, 64, 65, 4096, 4097, 5000])
def test_exact_selection_on_full_rings(amd, capacity):
    """every slot stored through add_batch and then given an integer priority: all m, so no leaf is left out"""
    buf = _buffer(capacity, capacity)
    leaf = R.power_of_two_priorities(capacity, 1000 + capacity)
    _set(buf, np.arange(capacity), leaf)
    np.testing.assert_array_equal(_leaves(buf), leaf)
    total = leaf.sum()
    assert float(buf.total_priority) == total and float(buf.min_priority) == leaf.min()
    u = _exact_uniforms(int(total))
    idx, _ = buf.draw(u.size, beta=0.4, uniforms=_dev(u, torch.float32))
    np.testing.assert_array_equal(idx.cpu().numpy(), R.select(leaf, R.masses(u.astype(np.float64), total)))
    # stratified: sample j draws from the j-th of n equal slices; with n = total and u = 0.5 slice j is the unit [j, j + 1)
    n = int(total)
    if n <= (1 << 15):
        half = np.full(n, 0.5, dtype=np.float32)
        idx, _ = buf.draw(n, stratified=True, uniforms=_dev(half, torch.float32))
        np.testing.assert_array_equal(idx.cpu().numpy(), R.select(leaf, R.masses(half.astype(np.float64), total, stratified=True)))


def test_an_all_zero_tree_gives_index_zero_and_weight_one(amd):
    from dgvit_amd import _lib as L
    for capacity in (1, 65, 4097):
        tree = torch.empty(L.load().dgvit_per_tree_floats(capacity), device="cuda")
        L.check(L.load().dgvit_per_init(_p(tree), capacity, _st()), "dgvit_per_init")
        levels = R.level_sizes(capacity)
        host = tree.cpu().numpy()
        assert host[0] == 1.0 and not host[1:64].any()
        off = 64
        for n in levels:
            pad = -(-n // 64) * 64
            assert not host[off:off + pad].any() and np.isposinf(host[off + pad:off + 2 * pad]).all()
            off += 2 * pad
        assert off == host.size
        idx, w = _raw_sample(tree, capacity, np.array(EDGE_U + [0.3], dtype=np.float32), beta=1.0)
        assert not idx.any() and (w == 1.0).all()


# ------------------------------------------------------------------------------------------------ 2. general floats
@pytest.fixture(scope="module")
def general(amd):
    """size 300, priorities 1 + 9 rng.random(300), alpha 0.6, and 65536 uploaded uniforms of the same generator"""
    rng = np.random.default_rng(1)
    prio = 1 + 9 * rng.random(300)
    u = rng.random(65536).astype(np.float32)
    buf = _buffer(300, 300, alpha=0.6, eps=1e-4)
    _set(buf, np.arange(300), prio)
    leaf = _leaves(buf)
    return dict(buf=buf, prio=prio, u=u, ud=_dev(u, torch.float32), leaf=leaf, C=np.cumsum(leaf), total=leaf.sum())


def test_general_selection_lands_in_the_right_interval(general):
    g = general
    idx, _ = g["buf"].draw(g["u"].size, uniforms=g["ud"])
    i = idx.cpu().numpy()
    assert i.min() >= 0 and i.max() < 300
    tol = 4 * 64 * 2.0 ** -24 * g["total"]          # four levels of at most 63 fp32 additions each
    mass = g["u"].astype(np.float64) * g["total"]
    lower = np.where(i > 0, g["C"][np.maximum(i - 1, 0)], 0.0)
    assert (lower - tol <= mass).all() and (mass <= g["C"][i] + tol).all()


def test_general_counts_follow_the_priorities(general):
    """every slot's count within 5 binomial sigma of B leaf / total (the fp64 restatement's own worst slot on these uniforms, with the
    leaves at alpha 0.6: 3.90 sigma; smallest expected count 84)"""
    g = general
    B = g["u"].size
    idx, _ = g["buf"].draw(B, uniforms=g["ud"])
    counts = np.bincount(idx.cpu().numpy(), minlength=300)
    p = g["leaf"] / g["total"]
    sigma = np.sqrt(B * p * (1 - p))
    z = np.abs(counts - B * p) / sigma
    print("worst slot:", z.max(), "sigma; smallest expected count:", (B * p).min())
    assert z.max() <= 5.0


def test_stratified_counts_are_within_four_of_their_expectation(general):
    """exact arithmetic bounds |count - B leaf / total| by 2 (the restatement stays within 1.6); each of a slot's two boundaries may move
    one sample under fp32 rounding"""
    g = general
    B = g["u"].size
    idx, _ = g["buf"].draw(B, stratified=True, uniforms=g["ud"])
    counts = np.bincount(idx.cpu().numpy(), minlength=300)
    dev = np.abs(counts - B * g["leaf"] / g["total"])
    print("largest deviation:", dev.max())
    assert dev.max() <= 4.0


# ------------------------------------------------------------------------------------------------ 3. weights and leaves
@pytest.mark.parametrize("beta", [0.0, 0.4, 1.0])
def test_weights_equal_the_restatement(general, beta):
    """rtol 1e-5: fp32 division and an accurate powf are within a few 6e-8 ulps, a wrong formula errs by percents"""
    g = general
    idx, w = g["buf"].draw(g["u"].size, beta=beta, uniforms=g["ud"])
    assert w.shape == (g["u"].size, 1) and w.dtype == torch.float32
    got = w[:, 0].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(got, R.weights(g["leaf"], idx.cpu().numpy(), beta), rtol=1e-5, atol=0)
    assert got.max() == 1.0, "the slot with the smallest leaf is drawn (expected 84 times) and has weight exactly 1"
    if beta == 0.0:
        assert (got == 1.0).all()


def test_leaves_after_an_update(general):
    g = general
    np.testing.assert_allclose(g["leaf"], R.leaves(g["prio"].astype(np.float32), 0.6, np.float64(np.float32(1e-4))), rtol=1e-5, atol=0)
    # alpha = 1: |p| + eps exactly as fp32 forms it; the sign is ignored; 0 gives eps; the clamp holds
    buf = _buffer(300, 300, alpha=1.0, eps=1e-4)
    rng = np.random.default_rng(2)
    p = (rng.standard_normal(300) * 10).astype(np.float32)
    p[:4] = [0.0, -0.0, 3e38, -3e38]
    _set(buf, np.arange(300), p)
    want = np.minimum(np.abs(p) + np.float32(1e-4), np.float32(2.0 ** 64)).astype(np.float32)
    np.testing.assert_array_equal(buf.priorities().cpu().numpy(), want)
    zero = _buffer(70, 70, alpha=0.5, eps=0.0)
    _set(zero, [3, 69], [0.0, 4.0])
    got = _leaves(zero)
    assert got[3] == 2.0 ** -64 and abs(got[69] - 2.0) <= 2e-5 and float(zero.min_priority) == 2.0 ** -64


# ------------------------------------------------------------------------------------------------ 4. update semantics
def _check_consistent(buf):
    """total = the fp64 sum of the leaves to 4 levels x 64 roundings; the min the weights use = the smallest leaf, exactly"""
    leaf = _leaves(buf)
    assert abs(float(buf.total_priority) - leaf.sum()) <= 64 * 4 * 2.0 ** -24 * leaf.sum()
    assert float(buf.min_priority) == leaf.min()
    return leaf


def test_duplicate_indices_keep_the_largest_new_value(amd):
    """also when the old value was larger than every new one; the same bits over 3 repeats (4096 updates on 50 slots, and 3 on one)"""
    rng = np.random.default_rng(5)
    idx = np.concatenate([[4999, 4999, 4999], rng.integers(0, 50, 4096), [4096, 64, 4096]])
    prio = np.concatenate([[0.5, 2.0, 1.0], rng.random(4096) * 3 + 0.25, [1.5, 0.75, 1.25]]).astype(np.float32)
    want = np.full(5000, 100.0)
    for i in np.unique(idx):
        want[i] = prio[idx == i].max()
    trees = []
    for _ in range(3):
        buf = _buffer(5000, 5000)
        _set(buf, np.arange(5000), np.full(5000, 100.0))     # the old value: larger than every new one
        _set(buf, idx, prio)
        np.testing.assert_array_equal(_leaves(buf), want)
        _check_consistent(buf)
        trees.append(buf.tree.clone())
    assert torch.equal(trees[0].view(torch.int32), trees[1].view(torch.int32))
    assert torch.equal(trees[0].view(torch.int32), trees[2].view(torch.int32))
    assert float(buf.max_priority) == 100.0


def test_indices_outside_the_stored_range_change_nothing(amd):
    buf = _buffer(5000, 4500)
    _set(buf, np.arange(4500), np.random.default_rng(6).random(4500) * 0.9 + 0.01)     # (below the max leaf 1: header word 1 is settled too)
    before = buf.tree.clone()
    bad = np.array([-1, 4500, 4999, 5000, 5001, 1 << 40, -(1 << 40), np.iinfo(np.int64).min, np.iinfo(np.int64).max])
    _set(buf, bad, np.full(bad.size, 50.0))
    assert torch.equal(buf.tree.view(torch.int32), before.view(torch.int32))
    # mixed with good ones: only the good ones land, and the max leaf rises by them alone
    _set(buf, np.array([-1, 7, 4500, 4499]), np.array([90.0, 3.0, 80.0, 2.0]))
    after = buf.tree.clone()
    leaf = _check_consistent(buf)
    assert leaf[7] == 3.0 and leaf[4499] == 2.0 and float(buf.max_priority) == 3.0
    changed = (after.view(torch.int32) != before.view(torch.int32)).nonzero().flatten().tolist()
    off = [o for o, _ in buf._levels]
    pad = [p for _, p in buf._levels]
    allowed = {0, 1}
    for leaf_i in (7, 4499):
        for l in range(3):
            allowed |= {off[l] + (leaf_i >> 6 * l), off[l] + pad[l] + (leaf_i >> 6 * l)}
    assert set(changed) <= allowed, "only the two leaves, their ancestors and the header changed"


def test_non_finite_priorities_sign_and_the_running_max(amd):
    buf = _buffer(5000, 4500)
    assert float(buf.max_priority) == 1.0
    _set(buf, [10, 11], [-7.0, 2.0])
    leaf = _check_consistent(buf)
    assert leaf[10] == 7.0 and leaf[11] == 2.0 and float(buf.max_priority) == 7.0
    _set(buf, [10, 12], [0.5, 3.0])                       # the max never falls, even when its slot does
    assert float(buf.max_priority) == 7.0
    _set(buf, [100, 101, 102, 103], [float("nan"), float("inf"), float("-inf"), 9.0])
    leaf = _check_consistent(buf)
    assert (leaf[100:103] == 7.0).all(), "a non-finite priority takes the max leaf as it stood when the call began"
    assert leaf[103] == 9.0 and float(buf.max_priority) == 9.0
    assert np.isfinite(float(buf.total_priority))
    _add(buf, 1)                                           # a new transition gets the max priority
    assert _leaves(buf)[4500] == 9.0


# ------------------------------------------------------------------------------------------------ 5. ring
def test_the_ring_hands_out_the_max_priority(amd):
    buf = _buffer(100, 70)
    assert (_leaves(buf) == 1.0).all() and buf.get_stored_size() == 70
    mine = 2.0 + np.arange(70) / 10.0
    _set(buf, np.arange(70), mine)
    top = float(buf.max_priority)
    assert top == float(np.float32(8.9))
    _add(buf, 50, base=70)                                  # add_batch straddling the end: slots 70 .. 99 and 0 .. 19
    leaf = _check_consistent(buf)
    assert buf.get_stored_size() == 100 and buf.next_index == 20
    assert (leaf[70:] == top).all() and (leaf[:20] == top).all(), "overwritten and new slots carry the max priority"
    np.testing.assert_array_equal(leaf[20:70], mine[20:70].astype(np.float32))
    _set(buf, [20, 21], [1.0, 20.0])
    for k in range(3):                                      # single adds at slots 20, 21, 22
        buf.add(obs=np.zeros((H, W)), next_obs=np.zeros((H, W)), pobs=[0, 0], next_pobs=[0, 0], act=[0, 0], rew=0.0, done=0.0)
    leaf = _check_consistent(buf)
    assert (leaf[20:23] == 20.0).all() and leaf[23] == np.float32(mine[23])
    _add(buf, 250)                                          # more rows than the ring: every slot is new
    assert (_check_consistent(buf) == 20.0).all() and buf.get_stored_size() == 100


def test_the_ring_wraps_across_a_level_boundary(amd):
    """size 4097 (three levels): a batch over slots 4090 .. 4096 and 0 .. 9 rebuilds both ends of every level"""
    buf = _buffer(4097, 4090)
    _set(buf, np.arange(4090), np.full(4090, 0.5))
    _set(buf, [5], [6.0])
    _add(buf, 17)
    leaf = _check_consistent(buf)
    want = np.full(4097, 0.5)
    want[4090:], want[:10] = 6.0, 6.0
    np.testing.assert_array_equal(leaf, want)


# ------------------------------------------------------------------------------------------------ 6. composition
def test_sample_is_the_draw_plus_the_base_gathers(amd):
    from dgvit_amd.replay import DeviceReplayBuffer
    buf = _buffer(100, 80, alpha=0.6, eps=1e-4, seed=3, frames=True)
    _set(buf, np.arange(80), np.random.default_rng(7).random(80) * 5)
    b = buf.sample(32, beta=0.4)
    assert b["weights"].shape == (32, 1) and b["indexes"].dtype == torch.int64 and int(b["indexes"].max()) < 80
    base = DeviceReplayBuffer.sample(buf, 32, indices=b["indexes"])
    assert set(b) == set(base) | {"weights"}
    for k in base:
        assert torch.equal(b[k], base[k]), k
    assert not torch.equal(buf.sample(32)["indexes"], b["indexes"]), "self.gen advances"
    # the same uniforms give the same draw, and the weights are the restatement's
    u = torch.rand(32, device="cuda")
    b1, b2 = buf.sample(32, uniforms=u), buf.sample(32, uniforms=u, stratified=False)
    assert torch.equal(b1["indexes"], b2["indexes"]) and torch.equal(b1["weights"], b2["weights"])
    np.testing.assert_allclose(b1["weights"][:, 0].cpu().numpy(), R.weights(_leaves(buf), b1["indexes"].cpu().numpy(), 0.4), rtol=1e-5)
    # DrQ shift composes unchanged
    s = buf.sample(32, uniforms=u, random_shift=2, return_shifts=True)
    assert torch.equal(s["indexes"], b1["indexes"]) and torch.equal(s["weights"], b1["weights"])
    for k in ("obs", "next_obs"):
        stored = buf.store[k][s["indexes"], :H * W].reshape(32, H, W)
        assert torch.equal(s[k], S.ref_shift(stored, s[k + "_shift"].cpu(), 2))
    assert int(s["obs_shift"].abs().max()) > 0
    for k in ("act", "rew", "pobs", "next_pobs", "done"):
        assert torch.equal(s[k], b1[k])


def test_an_empty_buffer_and_bad_tensors_are_refused(amd):
    buf = _buffer(10, 0)
    with pytest.raises(RuntimeError, match="empty"):
        buf.sample(4)
    _add(buf, 5)
    with pytest.raises(ValueError, match="uniforms"):
        buf.sample(4, uniforms=torch.rand(5, device="cuda"))
    with pytest.raises(ValueError, match="uniforms"):
        buf.sample(4, uniforms=torch.rand(4))
    with pytest.raises(ValueError, match="indexes"):
        buf.update_priorities(torch.zeros(4, device="cuda"), torch.ones(4, device="cuda"))
    with pytest.raises(ValueError, match="priorities"):
        buf.update_priorities(torch.zeros(4, dtype=torch.int64, device="cuda"), torch.ones(3, device="cuda"))
    buf.update_priorities(torch.tensor([0, 1], dtype=torch.int32), torch.tensor([[2.0], [3.0]], device="cuda"))     # int32 on the host, (B, 1)
    assert _leaves(buf).tolist() == [2.0, 3.0, 1.0, 1.0, 1.0]


# ------------------------------------------------------------------------------------------------ 7. capture
def test_sample_and_update_in_one_captured_graph(amd):
    """sample(uniforms=persistent) then update_priorities in one torch.cuda.graph (a linear chain, no side stream inside): replayed twice
    with the uniforms and the priorities refilled in between; each replay draws from the buffer's contents at replay time.  Integer leaves
    (alpha 1, eps 0) and masses (m + 0.5) T / 256 with T < 2^12 keep the comparison exact."""
    B, n = 64, 130
    buf = _buffer(n, n)
    rng = np.random.default_rng(11)
    _set(buf, np.arange(n), R.power_of_two_priorities(n, 12))
    u = torch.zeros(B, device="cuda")
    pr = torch.ones(B, device="cuda")

    def fill():
        u.copy_(_dev((rng.choice(256, B, replace=False) + 0.5) / 256.0, torch.float32))
        pr.copy_(_dev(rng.integers(1, 17, B).astype(np.float32), torch.float32))

    def step():
        b = buf.sample(B, beta=1.0, uniforms=u)
        buf.update_priorities(b["indexes"], pr)
        return b
    fill()
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
        with pytest.raises(amd.DgvitError, match="uniforms"):
            buf.sample(B)
    drawn = []
    for _ in range(2):
        fill()
        torch.cuda.synchronize()
        leaf = _leaves(buf)
        assert (leaf == np.round(leaf)).all() and leaf.sum() < 4096
        graph.replay()
        torch.cuda.synchronize()
        uh = u.cpu().numpy().astype(np.float64)
        want = R.select(leaf, R.masses(uh, leaf.sum()))
        got = static["indexes"].cpu().numpy()
        np.testing.assert_array_equal(got, want)
        np.testing.assert_allclose(static["weights"][:, 0].cpu().numpy(), R.weights(leaf, want, 1.0), rtol=1e-5)
        assert torch.equal(static["rew"][:, 0], static["indexes"].float()), "the gathers follow the drawn indices"
        after, prh = leaf.copy(), pr.cpu().numpy()
        for i in np.unique(want):
            after[i] = prh[want == i].max()
        np.testing.assert_array_equal(_leaves(buf), after)
        _check_consistent(buf)
        drawn.append(got.copy())
    assert not np.array_equal(drawn[0], drawn[1])
