"""CPU (no GPU): the prioritized-replay entry points (dgvit_per_*), their argument checks, the Python checks in front of them and the
host restatement tests/prioritized_replay_ref.py.  Every library call here fails its argument check before any launch: the pointers are
never dereferenced."""
import ctypes
import os

import numpy as np
import pytest
import torch

import prioritized_replay_ref as R

FAKE = ctypes.c_void_p(0x1000)   # non-null, 16-byte aligned, never read: only argument checks run
NAMES = ["dgvit_per_tree_floats", "dgvit_per_init", "dgvit_per_set_range", "dgvit_per_update", "dgvit_per_sample"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


def test_symbols_are_exported_bound_and_documented(lib):
    from dgvit_amd import _lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    with open(os.path.join(os.path.dirname(L.LIB_PATH), os.pardir, "include", "dgvit_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert hasattr(raw, name), name
        assert name in L.SIGNATURES, name
        assert name + "(" in header, name
    assert L.SIGNATURES["dgvit_per_tree_floats"] == (ctypes.c_longlong, [ctypes.c_longlong])
    res, args = L.SIGNATURES["dgvit_per_update"]
    assert res is ctypes.c_int and len(args) == 9 and args[6] is ctypes.c_float and args[7] is ctypes.c_float
    res, args = L.SIGNATURES["dgvit_per_sample"]
    assert res is ctypes.c_int and len(args) == 9 and args[4] is ctypes.c_int and args[5] is ctypes.c_float


def test_abi_version_is_unchanged(lib):
    assert lib.dgvit_abi_version() == 7


def test_class_is_exported_beside_the_base():
    from dgvit_amd import replay
    assert issubclass(replay.PrioritizedDeviceReplayBuffer, replay.DeviceReplayBuffer)
    assert "update_priorities" in replay.PrioritizedDeviceReplayBuffer.__doc__


# ------------------------------------------------------------------------------------------------ the size formula
@pytest.mark.parametrize("capacity, floats", [(1, 192), (64, 192), (65, 448), (4096, 8384), (4097, 8768), (1 << 24, 34087104)])
def test_tree_floats_table(lib, capacity, floats):
    assert lib.dgvit_per_tree_floats(capacity) == floats
    assert R.tree_floats(capacity) == floats


def test_tree_floats_equals_the_restatement_on_a_sweep(lib):
    from dgvit_amd.replay import per_tree_layout
    caps = sorted(set(list(range(1, 200)) + [4095, 4096, 4097, 4160, 4161, 100000, 262143, 262144, 262145, 266240, 266241, (1 << 24) - 1, 1 << 24]
                      + [int(c) for c in np.random.default_rng(0).integers(1, (1 << 24) + 1, 300)]))
    for c in caps:
        assert lib.dgvit_per_tree_floats(c) == R.tree_floats(c), c
        levels, floats = per_tree_layout(c)
        assert floats == R.tree_floats(c) and len(levels) == len(R.level_sizes(c)), c
    assert [len(R.level_sizes(c)) for c in (1, 64, 65, 4096, 4097, 262144, 262145, 1 << 24)] == [1, 1, 2, 2, 3, 3, 4, 4]


@pytest.mark.parametrize("capacity", [0, -1, (1 << 24) + 1])
def test_tree_floats_refuses_a_bad_capacity(lib, capacity):
    assert lib.dgvit_per_tree_floats(capacity) == -1


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _init(lib, tree=FAKE, capacity=100):
    return lib.dgvit_per_init(tree, capacity, None)


def _set_range(lib, tree=FAKE, capacity=100, first=0, count=10):
    return lib.dgvit_per_set_range(tree, capacity, first, count, None)


def _update(lib, tree=FAKE, capacity=100, stored=50, idx=FAKE, prio=FAKE, n=8, alpha=0.6, eps=1e-4):
    return lib.dgvit_per_update(tree, capacity, stored, idx, prio, n, alpha, eps, None)


def _sample(lib, tree=FAKE, capacity=100, uniforms=FAKE, n=8, stratified=0, beta=0.4, idx_out=FAKE, weights_out=FAKE):
    return lib.dgvit_per_sample(tree, capacity, uniforms, n, stratified, beta, idx_out, weights_out, None)


BAD = [
    (_init, "per_init", dict(tree=None), b"null"),
    (_init, "per_init", dict(capacity=0), b"capacity=0"),
    (_init, "per_init", dict(capacity=(1 << 24) + 1), b"capacity=16777217"),
    (_init, "per_init", dict(tree=ctypes.c_void_p(0x1004)), b"aligned"),
    (_set_range, "per_set_range", dict(tree=None), b"null"),
    (_set_range, "per_set_range", dict(capacity=0), b"capacity=0"),
    (_set_range, "per_set_range", dict(capacity=(1 << 24) + 1), b"capacity=16777217"),
    (_set_range, "per_set_range", dict(first=-1), b"first=-1"),
    (_set_range, "per_set_range", dict(first=100, count=1), b"first=100"),
    (_set_range, "per_set_range", dict(count=0), b"count=0"),
    (_set_range, "per_set_range", dict(count=-4), b"count=-4"),
    (_set_range, "per_set_range", dict(first=95, count=6), b"count=6"),
    (_set_range, "per_set_range", dict(first=1, count=1 << 62), b"first=1"),
    (_update, "per_update", dict(tree=None), b"null"),
    (_update, "per_update", dict(idx=None), b"null"),
    (_update, "per_update", dict(prio=None), b"null"),
    (_update, "per_update", dict(capacity=0), b"capacity=0"),
    (_update, "per_update", dict(capacity=(1 << 24) + 1), b"capacity=16777217"),
    (_update, "per_update", dict(stored=-1), b"stored=-1"),
    (_update, "per_update", dict(stored=101), b"stored=101"),
    (_update, "per_update", dict(n=0), b"n=0"),
    (_update, "per_update", dict(n=-2), b"n=-2"),
    (_update, "per_update", dict(n=1 << 24), b"n=16777216"),
    (_update, "per_update", dict(alpha=-0.1), b"alpha=-0.1"),
    (_update, "per_update", dict(alpha=1.5), b"alpha=1.5"),
    (_update, "per_update", dict(alpha=float("nan")), b"alpha="),
    (_update, "per_update", dict(eps=-1.0), b"eps=-1"),
    (_update, "per_update", dict(eps=float("inf")), b"eps=inf"),
    (_sample, "per_sample", dict(tree=None), b"null"),
    (_sample, "per_sample", dict(uniforms=None), b"null"),
    (_sample, "per_sample", dict(idx_out=None), b"null"),
    (_sample, "per_sample", dict(weights_out=None), b"null"),
    (_sample, "per_sample", dict(capacity=0), b"capacity=0"),
    (_sample, "per_sample", dict(capacity=(1 << 24) + 1), b"capacity=16777217"),
    (_sample, "per_sample", dict(n=0), b"n=0"),
    (_sample, "per_sample", dict(n=-1), b"n=-1"),
    (_sample, "per_sample", dict(n=1 << 24), b"n=16777216"),
    (_sample, "per_sample", dict(stratified=2), b"stratified=2"),
    (_sample, "per_sample", dict(beta=-0.5), b"beta=-0.5"),
    (_sample, "per_sample", dict(beta=1.25), b"beta=1.25"),
    (_sample, "per_sample", dict(beta=float("nan")), b"beta="),
]


@pytest.mark.parametrize("call, name, kw, word", BAD, ids=[f"{b[1]}-" + "-".join(f"{k}={v if not isinstance(v, ctypes.c_void_p) else v.value}"
                                                                                  for k, v in b[2].items()) for b in BAD])
def test_bad_arguments_are_refused_before_any_launch(lib, call, name, kw, word):
    assert call(lib, **kw) == -1          # DGVIT_ERR_ARG
    msg = lib.dgvit_last_error()
    assert name.encode() in msg and word in msg, msg


# ------------------------------------------------------------------------------------------------ the Python checks
@pytest.mark.parametrize("kw", [dict(alpha=-0.1), dict(alpha=1.01), dict(alpha=True), dict(alpha="0.6"), dict(alpha=None),
                                dict(alpha=float("nan")), dict(eps=-1e-6), dict(eps=False), dict(eps=float("inf")), dict(eps=float("nan")),
                                dict(eps="1e-4"), dict(size=(1 << 24) + 1), dict(size=0)],
                         ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_constructor_refuses_bad_arguments_before_the_device_is_touched(kw):
    """device="cpu" would be refused next (DgvitError), so a ValueError shows the check ran first, without storage or library"""
    from dgvit_amd.replay import PrioritizedDeviceReplayBuffer
    args = dict(size=8, obs_shape=(4, 4), device="cpu")
    args.update(kw)
    with pytest.raises(ValueError, match=next(iter(kw))):
        PrioritizedDeviceReplayBuffer(**args)


def test_constructor_refuses_a_cpu_device():
    import dgvit_amd
    from dgvit_amd.replay import PrioritizedDeviceReplayBuffer
    with pytest.raises(dgvit_amd.DgvitError, match="ROCm device"):
        PrioritizedDeviceReplayBuffer(8, obs_shape=(4, 4), device="cpu")


@pytest.mark.parametrize("bad", [-0.1, 1.5, True, None, "0.4", float("nan")])
def test_sample_refuses_bad_beta(bad):
    """the check runs before the library is loaded or anything is drawn: a buffer without storage is enough to reach it"""
    from dgvit_amd.replay import PrioritizedDeviceReplayBuffer
    buf = object.__new__(PrioritizedDeviceReplayBuffer)
    with pytest.raises(ValueError, match="beta"):
        buf.sample(4, beta=bad)
    with pytest.raises(ValueError, match="beta"):
        buf.draw(4, beta=bad)


def test_sample_takes_no_explicit_indices():
    from dgvit_amd.replay import PrioritizedDeviceReplayBuffer
    buf = object.__new__(PrioritizedDeviceReplayBuffer)
    with pytest.raises(TypeError):
        buf.sample(4, indices=torch.zeros(4, dtype=torch.int64))


def test_python_layout_is_the_restated_one():
    from dgvit_amd.replay import per_tree_layout
    levels, floats = per_tree_layout(4097)
    assert levels == [(64, 4160), (64 + 2 * 4160, 128), (64 + 2 * 4160 + 2 * 128, 64)] and floats == 8768


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restated_select_equals_the_written_out_loop():
    rng = np.random.default_rng(3)
    for trial in range(20):
        n = int(rng.integers(1, 40))
        leaf = rng.random(n) * (rng.random(n) > 0.4)          # zeros in front, inside and behind
        if trial == 0:
            leaf[:] = 0
        total = leaf.sum()
        mass = np.concatenate([[0.0, total, total * (1 - 2.0 ** -24)], rng.random(50) * total, np.cumsum(leaf)])
        got = R.select(leaf, mass)
        np.testing.assert_array_equal(got, R.select_loop(leaf, mass))
        if total > 0:
            assert (leaf[got] > 0).all()
        else:
            assert not got.any()


def test_restated_leaves_clamp_and_take_the_max_for_non_finite():
    got = R.leaves([0.0, -3.0, 1e30, np.nan, np.inf, -np.inf], 1.0, 0.0, max_leaf=7.0)
    np.testing.assert_array_equal(got, [2.0 ** -64, 3.0, 2.0 ** 64, 7.0, 7.0, 7.0])
    np.testing.assert_allclose(R.leaves([2.0, -2.0], 0.5, 2.0), [2.0, 2.0])
    np.testing.assert_array_equal(R.leaves([0.0, 5.0], 0.0, 0.0), [1.0, 1.0])


def test_restated_masses_and_weights():
    u = np.array([0.5, 0.5, 0.5, 0.5])
    np.testing.assert_array_equal(R.masses(u, 8.0), [4.0] * 4)
    np.testing.assert_array_equal(R.masses(u, 8.0, stratified=True), [1.0, 3.0, 5.0, 7.0])
    leaf = np.array([0.0, 4.0, 1.0, 2.0])
    np.testing.assert_array_equal(R.weights(leaf, np.array([1, 2, 3]), 1.0), [0.25, 1.0, 0.5])
    np.testing.assert_array_equal(R.weights(leaf, np.array([1, 2, 3]), 0.0), [1.0, 1.0, 1.0])


@pytest.mark.parametrize("k", [1, 2, 3, 7, 64, 300, 5000])
def test_power_of_two_priorities(k):
    p = R.power_of_two_priorities(k, k)
    s = int(p.sum())
    assert p.min() >= 1 and p.max() <= 16 and (p == np.round(p)).all() and s & (s - 1) == 0
