"""n-step replay sampling (dgvit_amd.replay: sample(..., n_step=, gamma=)) restated in numpy: the ring's store path with its
episode flags (``Ring.store`` / ``mark``), the walk (``Ring.walk``), and, with no ring at all, the truth computed from the transition
stream itself (``truth``) that the restatement is checked against.

A transition of the stream is (rew, done, end): ``end`` says that on_episode_end() followed it.  Stream position t is the number of
transitions offered before it.  The n-step transition that starts at t visits t, t + 1, ... and stops behind the first position with
done != 0 or end, at the last position of the stream (nothing newer exists), or after n positions:

    m = positions visited,  ret = sum_{k<m} gamma^k rew_{t+k},  discount = gamma^m,  tail = t + m - 1

The yardstick is float64: products gamma^k built left to right, the sum in ascending k.  ``tolerance`` is derived, not measured:

    2^-23 |ref| + m 2^-52 sum_k gamma^k |r_k|

the one rounding to fp32, and the double sum of m terms with or without fma contraction.

``scenario`` is the stream the tests push through the buffers: episodes of lengths drawn from {1, 2, 3, 7, 11} that end by done = 1, by
on_episode_end() or by both, rewards that are multiples of 1/256 in [-1, 1], cut into add / add_batch calls (a call ends wherever
on_episode_end() must follow, because only the newest slot can take END).
"""
import numpy as np

END, HEAD = 1, 2
NS = (1, 2, 3, 5, 64)
GAMMAS = (0.99, 0.5, 1.0, 0.0)
SIZE, TOTAL, FRAME, PSTATE, ACT = 37, 52, (6, 10), 2, 2
LENGTHS = (1, 2, 3, 7, 11)


def exact(n, gamma):
    """the cases whose arithmetic on multiples of 1/256 in [-1, 1] is exact in fp32 and in double: rew and discount must be bit-equal"""
    return gamma == 1.0 or gamma == 0.0 or (gamma == 0.5 and n <= 5)


class Ring:
    """rew, done, the episode flags and, per slot, the stream position of the transition it holds (-1: never written)"""

    def __init__(self, size, tracked=True):
        self.size = int(size)
        self.rew, self.done = np.zeros(size, np.float32), np.zeros(size, np.float32)
        self.pos = np.full(size, -1, np.int64)
        self.flags = np.zeros(size, np.uint8) if tracked else None
        self.next_index = self.stored = 0

    def track(self):
        if self.flags is None:
            self.flags = np.zeros(self.size, np.uint8)
            if self.stored:
                self.flags[(self.next_index - 1) % self.size] = HEAD

    def mark(self, start, n):
        """dgvit_ring_mark"""
        assert 1 <= n <= self.size and 0 <= start < self.size
        self.flags[(start + np.arange(n)) % self.size] = 0
        self.flags[(start + n - 1) % self.size] = HEAD
        if n < self.size:
            self.flags[(start - 1) % self.size] &= END

    def store(self, rew, done, pos):
        """add (one transition) / add_batch (arrays): of more than `size` transitions the last `size` stay"""
        rew, done, pos = (np.atleast_1d(np.asarray(v)) for v in (rew, done, pos))
        n = min(len(rew), self.size)
        slots = (self.next_index + np.arange(n)) % self.size
        self.rew[slots], self.done[slots], self.pos[slots] = rew[-n:], done[-n:], pos[-n:]
        if self.flags is not None:
            self.mark(self.next_index, n)
        self.next_index = (self.next_index + n) % self.size
        self.stored = min(self.stored + n, self.size)

    def episode_end(self):
        assert self.stored
        self.track()
        self.flags[(self.next_index - 1) % self.size] |= END

    def walk(self, idx, n, gamma, descending=False, fp32_sum=False):
        """dgvit_nstep_walk on the slots idx -> dict of arrays: ret64, rew (ret64 rounded to fp32 once), disc64, discount, steps, tail,
        done, tol (``tolerance``), why (the stop reasons).  ``descending``: the same sum evaluated last term first with gamma ** k, a second
        float64 evaluation.  ``fp32_sum``: what a kernel accumulating in fp32 would return, to show that the tolerance refuses it."""
        self.track()
        gamma = float(gamma)
        idx = np.clip(np.asarray(idx, np.int64).reshape(-1), 0, self.size - 1)
        out = {k: [] for k in ("ret64", "disc64", "steps", "tail", "done", "tol", "why")}
        for i in idx:
            slots, why = [], set()
            for k in range(n):
                s = (int(i) + k) % self.size
                slots.append(s)
                if self.done[s] != 0:
                    why.add("done")
                if self.flags[s] & END:
                    why.add("end")
                if self.flags[s] & HEAD:
                    why.add("head")
                if k == n - 1:
                    why.add("n")
                if why:
                    break
            m = len(slots)
            r = [float(self.rew[s]) for s in slots]
            if fp32_sum:
                acc, g = np.float32(0), np.float32(1)
                for x in r:
                    acc, g = np.float32(acc + g * np.float32(x)), np.float32(g * np.float32(gamma))
                acc = float(acc)
            elif descending:
                acc = 0.0
                for k in reversed(range(m)):
                    acc += gamma ** k * r[k]
            else:
                acc, g = 0.0, 1.0
                for x in r:
                    acc += g * x
                    g *= gamma
            g, mag = 1.0, 0.0
            for x in r:
                mag += g * abs(x)
                g *= gamma
            out["ret64"].append(acc), out["disc64"].append(g), out["steps"].append(m), out["tail"].append(slots[-1])
            out["done"].append(self.done[slots[-1]]), out["why"].append(frozenset(why))
            out["tol"].append(m * 2.0 ** -52 * mag)
        res = dict(ret64=np.array(out["ret64"], np.float64), disc64=np.array(out["disc64"], np.float64), steps=np.array(out["steps"], np.int32),
                   tail=np.array(out["tail"], np.int64), done=np.array(out["done"], np.float32), why=out["why"])
        res["rew"], res["discount"] = res["ret64"].astype(np.float32), res["disc64"].astype(np.float32)
        res["tol"] = 2.0 ** -23 * np.abs(res["ret64"]) + np.array(out["tol"], np.float64)
        return res


def truth(stream, t, n, gamma):
    """(ret, discount, m, tail position, done of the tail, stop reasons) of the n-step transition that starts at stream position t, from
    the stream alone: ``stream`` is the list of (rew, done, end) of every transition offered so far"""
    gamma = float(gamma)
    acc, g, why, k = 0.0, 1.0, set(), 0
    while True:
        rew, done, end = stream[t + k]
        acc += g * float(rew)
        g *= gamma
        if done != 0:
            why.add("done")
        if end:
            why.add("end")
        if t + k == len(stream) - 1:
            why.add("head")
        if k == n - 1:
            why.add("n")
        k += 1
        if why:
            return acc, g, k, t + k - 1, np.float32(done), frozenset(why)


def scenario(total=TOTAL, seed=5, max_call=5):
    """(stream, ops): ``stream`` the list of (rew, done, end) of `total` transitions, ``ops`` the calls that offer them, in order:
    ("add", t), ("add_batch", [t, ...]) or ("episode_end",) -- t a stream position"""
    g = np.random.default_rng(seed)
    stream = []
    while len(stream) < total:
        length = int(g.choice(LENGTHS))
        how = ("done", "end", "both")[int(g.integers(3))]
        for j in range(length):
            last = j == length - 1
            rew = np.float32(int(g.integers(-256, 257)) / 256.0)
            stream.append((rew, np.float32(1.0 if last and how in ("done", "both") else 0.0), bool(last and how in ("end", "both"))))
    stream = stream[:total]
    ops, t = [], 0
    while t < total:
        want = int(g.integers(1, max_call + 1))
        call = []
        while t < total and len(call) < want:
            call.append(t)
            t += 1
            if stream[t - 1][2]:
                break
        ops.append(("add", call[0]) if len(call) == 1 else ("add_batch", call))
        if stream[call[-1]][2]:
            ops.append(("episode_end",))
    return stream, ops


def offer(ring, stream, ops):
    """the ops on a reference ring"""
    for op in ops:
        if op[0] == "episode_end":
            ring.episode_end()
        else:
            ts = [op[1]] if op[0] == "add" else op[1]
            ring.store([stream[t][0] for t in ts], [stream[t][1] for t in ts], ts)
    return ring
