"""Host restatement (numpy, fp64) of prioritized replay as include/dgvit_hip.h states it, independent of the kernels (shared by
test_prioritized_replay_host.py and test_gpu_prioritized_replay.py).

* ``leaves``: clamp((|priority| + eps)^alpha, 2^-64, 2^64); a non-finite priority takes ``max_leaf``.
* ``select``: the slot a mass falls in is ``searchsorted(cumsum(leaves), mass, side="right")`` -- the first slot whose inclusive prefix
  exceeds the mass, which a zero leaf never is -- clipped to the last nonzero leaf (mass == total); an all-zero tree gives slot 0.
* ``masses``: u * total, or (j + u) / n * total for the stratified draw.
* ``weights``: (p_min / leaf)^beta with p_min the smallest nonzero leaf.
* ``tree_floats``: 64 + 2 * sum_l pad64(n_l), n_0 = capacity, n_l = ceil(n_{l-1} / 64), the last level the first with n_l <= 64.
"""
import numpy as np

LEAF_MIN, LEAF_MAX = 2.0 ** -64, 2.0 ** 64
MAX_CAPACITY = 1 << 24


def leaves(priorities, alpha, eps, max_leaf=1.0):
    p = np.asarray(priorities, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.clip((np.abs(p) + eps) ** alpha, LEAF_MIN, LEAF_MAX)
    return np.where(np.isfinite(p), v, max_leaf)


def select(leaf, mass):
    leaf = np.asarray(leaf, dtype=np.float64)
    mass = np.atleast_1d(np.asarray(mass, dtype=np.float64))
    nz = np.flatnonzero(leaf > 0)
    if nz.size == 0:
        return np.zeros(mass.shape, dtype=np.int64)
    i = np.searchsorted(np.cumsum(leaf), mass, side="right")
    return np.clip(i, 0, nz[-1]).astype(np.int64)


def select_loop(leaf, mass):
    """``select`` written out: walk the slots, keep the first nonzero one whose running sum exceeds the mass"""
    out = []
    for m in np.atleast_1d(mass):
        run, pick, last = 0.0, None, 0
        for i, v in enumerate(leaf):
            run += float(v)
            if v > 0:
                last = i
                if pick is None and run > m:
                    pick = i
        out.append(last if pick is None else pick)
    return np.asarray(out, dtype=np.int64)


def masses(u, total, stratified=False):
    u = np.asarray(u, dtype=np.float64)
    if stratified:
        return (np.arange(u.size) + u) / u.size * total
    return u * total


def weights(leaf, idx, beta):
    leaf = np.asarray(leaf, dtype=np.float64)
    return (leaf[leaf > 0].min() / leaf[idx]) ** beta


def level_sizes(capacity):
    n, out = int(capacity), []
    while True:
        out.append(n)
        if n <= 64:
            return out
        n = -(-n // 64)


def tree_floats(capacity):
    return 64 + 2 * sum(-(-n // 64) * 64 for n in level_sizes(capacity))


def power_of_two_priorities(k, seed):
    """k integers in [1, 16] whose sum is a power of two (the one in (4k, 8k]; 16 for k == 2, any for k == 1): with them every partial
    sum of the tree, in any order, is exact in fp32"""
    rng = np.random.default_rng(seed)
    p = rng.integers(1, 17, size=k)
    target = 1 << int(np.floor(np.log2(8 * k)))
    if k <= 2:
        target = 16 if k == 2 else 1 << int(rng.integers(0, 5))
    while p.sum() != target:
        up = p.sum() < target
        c = np.flatnonzero(p < 16) if up else np.flatnonzero(p > 1)
        p[c[rng.integers(c.size)]] += 1 if up else -1
    return p.astype(np.float64)
