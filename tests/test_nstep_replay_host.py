"""CPU (no GPU): n-step replay sampling -- the entry points dgvit_ring_mark, dgvit_nstep_walk and dgvit_sac_critic_loss_v2 with their
argument checks, the Python checks in front of them, and the numpy restatement tests/nstep_ref.py against a truth computed from the
transition stream alone.  Every library call here fails its argument check before any launch: the pointers are never dereferenced."""
import ctypes
import os

import numpy as np
import pytest
import torch

import nstep_ref as N

FAKE = ctypes.c_void_p(0x1000)   # non-null, 16-byte aligned, never read: only argument checks run
OFF8 = ctypes.c_void_p(0x1008)   # 8-byte but not 16-byte aligned
OFF4 = ctypes.c_void_p(0x1004)   # 4-byte but not 8-byte aligned
OFF2 = ctypes.c_void_p(0x1002)

NAMES = ("dgvit_ring_mark", "dgvit_nstep_walk", "dgvit_sac_critic_loss_v2")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


def test_symbols_are_exported_bound_and_declared(lib):
    from dgvit_amd import _lib as L
    raw = ctypes.CDLL(L.LIB_PATH)
    with open(os.path.join(os.path.dirname(L.LIB_PATH), os.pardir, "include", "dgvit_hip.h")) as f:
        header = f.read()
    P, I, LL, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double
    for name in NAMES:
        assert hasattr(raw, name)
        assert "int " + name + "(" in header
    assert L.SIGNATURES["dgvit_ring_mark"] == (I, [P, LL, LL, LL, P])
    assert L.SIGNATURES["dgvit_nstep_walk"] == (I, [P, LL, P, LL, P, P, LL, P, LL, LL, I, D] + [P] * 7)
    assert L.SIGNATURES["dgvit_sac_critic_loss_v2"] == (I, [P] * 10 + [F, F] + [P] * 4 + [I, I, P])
    assert L.SIGNATURES["dgvit_sac_critic_loss"] == (I, [P] * 9 + [F, F] + [P] * 4 + [I, I, P]), "the first entry point keeps its signature"
    assert "#define DGVIT_RING_END 1" in header and "#define DGVIT_RING_HEAD 2" in header
    from dgvit_amd import replay
    assert (replay.FLAG_END, replay.FLAG_HEAD, replay.NSTEP_MAX) == (N.END, N.HEAD, 64)


def test_abi_version_is_unchanged(lib):
    assert lib.dgvit_abi_version() == 7


def _ids(v):
    return None if isinstance(v, bytes) else "-".join(f"{k}={x if not isinstance(x, ctypes.c_void_p) else x.value}" for k, x in v.items())


def _msg(lib, rc, name, word):
    assert rc == -1, "DGVIT_ERR_ARG"
    msg = lib.dgvit_last_error()
    assert name in msg and word in msg, msg


def _mark(lib, flags=FAKE, nrows=37, start=0, n=1):
    return lib.dgvit_ring_mark(flags, nrows, start, n, None)


@pytest.mark.parametrize("kw, word", [
    (dict(flags=None), b"null"),
    (dict(nrows=0), b"nrows=0"),
    (dict(nrows=-1), b"nrows=-1"),
    (dict(n=0), b"n=0"),
    (dict(n=-2), b"n=-2"),
    (dict(n=38), b"n=38"),                  # n > nrows
    (dict(start=-1), b"start=-1"),
    (dict(start=37), b"start=37"),
    (dict(start=1 << 40), b"start=1099511627776"),
], ids=_ids)
def test_ring_mark_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _mark(lib, **kw), b"ring_mark", word)


def _walk(lib, rew=FAKE, rew_ld=4, done=FAKE, done_ld=4, flags=FAKE, next_small=FAKE, small_ld=4, idx=FAKE, nsel=8, nrows=37, n=3,
          gamma=0.99, ret_out=FAKE, done_out=FAKE, discount_out=FAKE, next_small_out=FAKE, steps_out=FAKE, tail_out=FAKE):
    return lib.dgvit_nstep_walk(rew, rew_ld, done, done_ld, flags, next_small, small_ld, idx, nsel, nrows, n, gamma, ret_out, done_out,
                                discount_out, next_small_out, steps_out, tail_out, None)


WALK_POINTERS = ("rew", "done", "flags", "next_small", "idx", "ret_out", "done_out", "discount_out", "next_small_out", "steps_out", "tail_out")


@pytest.mark.parametrize("kw, word", [({k: None}, b"null") for k in WALK_POINTERS] + [
    (dict(nsel=0), b"nsel=0"),
    (dict(nsel=-5), b"nsel=-5"),
    (dict(nsel=1 << 31), b"nsel=2147483648"),
    (dict(nrows=0), b"nrows=0"),
    (dict(nrows=-37), b"nrows=-37"),
    (dict(n=0), b"n=0"),
    (dict(n=-1), b"n=-1"),
    (dict(n=65), b"n=65"),
    (dict(gamma=float("nan")), b"gamma="),
    (dict(gamma=-0.1), b"gamma=-0.1"),
    (dict(gamma=1.5), b"gamma=1.5"),
    (dict(gamma=float("inf")), b"gamma=inf"),
    (dict(rew_ld=0), b"rew_ld=0"),
    (dict(done_ld=-4), b"done_ld=-4"),
    (dict(small_ld=0), b"small_ld=0"),
    (dict(small_ld=2), b"small_ld=2"),
    (dict(small_ld=6), b"small_ld=6"),
    (dict(next_small=OFF8), b"16-byte aligned"),
    (dict(next_small_out=OFF8), b"16-byte aligned"),
    (dict(next_small_out=OFF4), b"16-byte aligned"),
    (dict(rew=OFF2), b"aligned"),
    (dict(done=OFF2), b"aligned"),
    (dict(ret_out=OFF2), b"aligned"),
    (dict(done_out=OFF2), b"aligned"),
    (dict(discount_out=OFF2), b"aligned"),
    (dict(steps_out=OFF2), b"aligned"),
    (dict(idx=OFF4), b"aligned"),
    (dict(tail_out=OFF4), b"aligned"),
], ids=_ids)
def test_nstep_walk_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _walk(lib, **kw), b"nstep_walk", word)


def _critic(lib, q1=FAKE, q2=FAKE, reward=FAKE, done=None, weights=None, discount=FAKE, next_q1=FAKE, next_q2=FAKE, next_log_pi=FAKE,
            log_alpha=None, alpha=0.2, gamma=0.99, target=FAKE, td=None, loss=FAKE, grads=None, B=32, A=2):
    return lib.dgvit_sac_critic_loss_v2(q1, q2, reward, done, weights, discount, next_q1, next_q2, next_log_pi, log_alpha, alpha, gamma, target,
                                        td, loss, grads, B, A, None)


CRITIC_BAD = [({k: None}, b"null") for k in ("q1", "q2", "reward", "next_q1", "next_q2", "next_log_pi", "target", "loss")]
CRITIC_BAD += [({k: OFF2}, b"aligned") for k in ("q1", "q2", "reward", "done", "weights", "discount", "next_q1", "next_q2", "next_log_pi", "log_alpha",
                                                 "target", "td", "loss", "grads")]
CRITIC_BAD += [
    (dict(B=0), b"B=0"),
    (dict(B=-3), b"B=-3"),
    (dict(A=0), b"A=0"),
    (dict(A=17), b"A=17"),
    (dict(B=(1 << 19) + 1, A=2), b"B*A=1048578"),
    (dict(alpha=float("nan")), b"alpha="),
    (dict(alpha=float("inf")), b"alpha=inf"),
    (dict(discount=None, gamma=float("nan")), b"gamma="),            # without a discount the call is the first entry point: gamma is read
    (dict(discount=None, gamma=float("-inf")), b"gamma=-inf"),
    (dict(gamma=float("nan"), B=0), b"B=0"),                         # with one it is not: a NaN gamma is not what is refused
]


@pytest.mark.parametrize("kw, word", CRITIC_BAD, ids=_ids)
def test_critic_loss_v2_refuses_bad_arguments_before_any_launch(lib, kw, word):
    _msg(lib, _critic(lib, **kw), b"sac_critic_loss", word)


# ------------------------------------------------------------------------------------------------ the Python checks
@pytest.mark.parametrize("bad", [True, False, 3.0, 0, 65, -1, "3", np.float32(2), [3]])
def test_bad_n_step_raises_without_a_device(bad):
    from dgvit_amd import replay
    with pytest.raises(ValueError, match="n_step"):
        replay._n_step(bad)
    for cls in (replay.DeviceReplayBuffer, replay.PrioritizedDeviceReplayBuffer):
        buf = object.__new__(cls)         # no device behind it: the check runs before anything is touched
        with pytest.raises(ValueError, match="n_step"):
            buf.sample(4, n_step=bad)


@pytest.mark.parametrize("bad", [True, -0.1, 1.5, float("nan"), float("inf"), "0.9", None, torch.tensor(0.9)])
def test_bad_gamma_raises_without_a_device(bad):
    from dgvit_amd import replay
    for cls in (replay.DeviceReplayBuffer, replay.PrioritizedDeviceReplayBuffer):
        buf = object.__new__(cls)
        with pytest.raises(ValueError, match="gamma"):
            buf.sample(4, n_step=3, gamma=bad)


def test_good_n_step_and_gamma_pass_the_helpers():
    from dgvit_amd import replay
    assert replay._n_step(None) is None
    assert [replay._n_step(v) for v in (1, 64, np.int64(5))] == [1, 64, 5]
    assert [replay._unit("gamma", v) for v in (0, 1, 0.99, np.float32(0.5))] == [0.0, 1.0, 0.99, 0.5]


def _critic_args(Bn=4, A=2):
    return [torch.zeros(Bn, A), torch.zeros(Bn, A), torch.zeros(Bn, 1), torch.zeros(Bn, A), torch.zeros(Bn, A), torch.zeros(Bn, 1)]


@pytest.mark.parametrize("bad", [torch.zeros(3), torch.zeros(4, 2), torch.zeros(1, 4), torch.zeros(()), 0.99, [0.99] * 4, np.zeros(4, np.float32)])
def test_bad_discount_shape_raises_before_the_device_check(bad):
    from dgvit_amd import sac_losses
    with pytest.raises(ValueError, match="discount"):
        sac_losses.critic_loss(*_critic_args(), alpha=0.2, discount=bad)


def test_discount_on_the_cpu_reaches_the_device_check_and_gamma_is_not_read():
    """shapes right, tensors on the CPU: the shape checks pass and the device check refuses; gamma=None is not looked at"""
    import dgvit_amd
    from dgvit_amd import sac_losses
    for disc in (torch.ones(4), torch.ones(4, 1)):
        with pytest.raises(dgvit_amd.DgvitError):
            sac_losses.critic_loss(*_critic_args(), alpha=0.2, discount=disc, gamma=None)
    with pytest.raises(ValueError, match="gamma"):
        sac_losses.critic_loss(*_critic_args(), alpha=0.2, gamma=None)


# ------------------------------------------------------------------------------------------------ the restatement against the stream
def _compare(ring, stream, n, gamma):
    """every written slot of ``ring``: the walk against the truth at the slot's stream position -> the stop reasons seen"""
    slots = np.flatnonzero(ring.pos >= 0)
    w = ring.walk(slots, n, gamma)
    for j, s in enumerate(slots):
        ret, disc, m, tail, done, why = N.truth(stream, int(ring.pos[s]), n, gamma)
        assert w["ret64"][j] == ret and w["disc64"][j] == disc, (s, n, gamma)
        assert w["steps"][j] == m and ring.pos[w["tail"][j]] == tail and w["done"][j] == done, (s, n, gamma)
        assert w["why"][j] == why, (s, n, gamma)
    return set(w["why"])


@pytest.mark.parametrize("size, total", [(37, 52), (37, 20), (5, 52), (5, 3), (1, 9), (64, 52), (64, 64), (64, 200)])
def test_ring_and_flags_walk_equals_the_stream(size, total):
    stream, ops = N.scenario(total=total, max_call=max(5, size + 3) if size <= 5 else 5)
    ring, seen = N.Ring(size), set()
    done = 0
    for j, op in enumerate(ops):                     # after every call, not only at the end: every head position occurs
        N.offer(ring, stream, [op])
        done += 0 if op[0] == "episode_end" else (1 if op[0] == "add" else len(op[1]))
        if j + 1 < len(ops) and ops[j + 1][0] == "episode_end":
            continue                                 # (the stream says `end` of a transition whose on_episode_end() is the next call)
        assert int((ring.flags & N.HEAD != 0).sum()) == 1, "exactly one slot carries HEAD"
        assert ring.flags[(ring.next_index - 1) % size] & N.HEAD
        assert ring.stored == min(done, size)
        for n in (1, 3, 64):
            seen |= _compare(ring, stream[:done], n, 0.99)
    for n in N.NS:
        for gamma in N.GAMMAS:
            seen |= _compare(ring, stream, n, gamma)
    if (size, total) == (37, 52):
        assert ring.next_index == 15 and ring.stored == 37, "the ring wrapped: 15 slots were overwritten"
        want = {frozenset(w) for w in (("done",), ("end",), ("done", "end"), ("head",), ("n",), ("done", "n"), ("end", "n"), ("done", "end", "n"),
                                       ("head", "n"))}
        assert want <= seen, want - seen


def test_add_batch_of_more_than_size_and_a_store_that_ends_at_the_last_slot():
    ring = N.Ring(8)
    ring.store(np.zeros(5), np.zeros(5), np.arange(5))
    ring.episode_end()
    assert ring.flags.tolist() == [0, 0, 0, 0, N.HEAD | N.END, 0, 0, 0]
    ring.store(np.zeros(3), np.zeros(3), 5 + np.arange(3))           # ends exactly at the last slot
    assert ring.flags.tolist() == [0, 0, 0, 0, N.END, 0, 0, N.HEAD] and ring.next_index == 0
    ring.store(np.zeros(11), np.zeros(11), 8 + np.arange(11))        # n > size: the last 8 stay, every old mark is forgotten
    assert ring.flags.tolist() == [0, 0, 0, 0, 0, 0, 0, N.HEAD] and ring.pos.tolist() == list(range(11, 19))
    ring.episode_end()
    ring.store(0.0, 0.0, 19)
    assert ring.flags.tolist() == [N.HEAD, 0, 0, 0, 0, 0, 0, N.END]


def test_tracking_that_starts_late_knows_only_the_head():
    ring = N.Ring(8, tracked=False)
    ring.store(np.zeros(3), np.array([0, 1, 0], np.float32), np.arange(3))
    assert ring.flags is None
    ring.track()
    assert ring.flags.tolist() == [0, 0, N.HEAD, 0, 0, 0, 0, 0]
    w = ring.walk([0, 1, 2], 5, 0.5)
    assert w["steps"].tolist() == [2, 1, 1], "done still stops a walk; the head stops the last one"


# ------------------------------------------------------------------------------------------------ the tolerance
@pytest.fixture(scope="module")
def full_ring():
    stream, ops = N.scenario()
    return N.offer(N.Ring(N.SIZE), stream, ops)


def test_the_yardstick_meets_the_tolerance_in_the_other_summation_order(full_ring):
    worst = 0.0
    for n in N.NS:
        for gamma in N.GAMMAS:
            a, b = full_ring.walk(np.arange(N.SIZE), n, gamma), full_ring.walk(np.arange(N.SIZE), n, gamma, descending=True)
            err = np.abs(a["ret64"] - b["ret64"])
            assert (err <= a["tol"]).all(), (n, gamma)
            assert (np.abs(b["ret64"].astype(np.float32).astype(np.float64) - a["ret64"]) <= a["tol"]).all(), "and rounded to fp32 once"
            worst = max(worst, float((err / a["tol"])[a["tol"] > 0].max(initial=0.0)))
            if N.exact(n, gamma):
                assert np.array_equal(a["ret64"], b["ret64"]), "exact arithmetic: any order gives the same bits"
                assert np.array_equal(a["ret64"], a["rew"].astype(np.float64)) and np.array_equal(a["disc64"], a["discount"].astype(np.float64))
    assert worst < 1.0


def test_the_tolerance_refuses_a_sum_accumulated_in_fp32(full_ring):
    """the bound does demand the double accumulation: at gamma = 0.99 an fp32 accumulator misses it"""
    worst = 0.0
    for n in (5, 64):
        a, b = full_ring.walk(np.arange(N.SIZE), n, 0.99), full_ring.walk(np.arange(N.SIZE), n, 0.99, fp32_sum=True)
        ok = a["tol"] > 0
        worst = max(worst, float((np.abs(b["ret64"] - a["ret64"])[ok] / a["tol"][ok]).max()))
    assert worst > 2.0, worst


def test_scenario_is_what_the_tests_say_it_is():
    stream, ops = N.scenario()
    assert len(stream) == N.TOTAL == 52
    assert {op[0] for op in ops} == {"add", "add_batch", "episode_end"}
    assert all(abs(r) <= 1 and float(r) * 256 == int(float(r) * 256) for r, _, _ in stream)
    ends = {(bool(d), e) for _, d, e in stream if d or e}
    assert ends == {(True, False), (False, True), (True, True)}, "episodes end by done, by on_episode_end() and by both"
    offered = [t for op in ops if op[0] != "episode_end" for t in ([op[1]] if op[0] == "add" else op[1])]
    assert offered == list(range(52))
    for j, op in enumerate(ops):
        if op[0] == "episode_end":
            prev = ops[j - 1]
            assert stream[prev[1] if prev[0] == "add" else prev[1][-1]][2]
