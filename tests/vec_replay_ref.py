"""The replay ring of E parallel environments (dgvit_amd.replay: DeviceReplayBuffer(num_envs=E), add_vec) restated in numpy:
the slot layout, the flag rules of dgvit_ring_store_small and the strided walk of dgvit_nstep_walk_strided.

Vector step t lies in the E consecutive slots base .. base + E - 1, base = (t E) mod size, environment e in slot base + e; E divides size,
so the successor of slot s in its episode is (s + E) mod size and the lane s mod E survives the wrap.

``streams(E, T)`` are E independent episode streams, ``nstep_ref.scenario(total=T, seed=5 + e)[0]``: episodes that end by done, by `end`
or by both, rewards that are multiples of 1/256.  The yardstick of every n-step value is ``truth(streams, e, t, newest, n, gamma)``:
``nstep_ref.truth`` on environment e's stream ALONE, cut behind the newest step -- no ring in it.  The tolerance is nstep_ref's derived one,
2^-23 |ref| + m 2^-52 sum_k gamma^k |r_k| (``tolerance``)."""
import numpy as np

import nstep_ref as N

END, HEAD = N.END, N.HEAD
FRAME, PSTATE, ACT = N.FRAME, N.PSTATE, N.ACT


def streams(E, T):
    return [N.scenario(total=T, seed=5 + e)[0] for e in range(E)]


def truth(strs, e, t, newest, n, gamma):
    """nstep_ref.truth of environment e's transition t when step `newest` is the last one stored"""
    return N.truth(strs[e][:newest + 1], t, n, gamma)


def tolerance(stream, t, m, gamma, ret):
    g, mag = 1.0, 0.0
    for k in range(m):
        mag += g * abs(float(stream[t + k][0]))
        g *= float(gamma)
    return 2.0 ** -23 * abs(ret) + m * 2.0 ** -52 * mag


class VecRing:
    """rew, done, the episode flags and, per slot, the step t of the transition it holds (-1: never written); the environment of slot s
    is s % E"""

    def __init__(self, E, size, tracked=True):
        assert 1 <= E <= size and size % E == 0
        self.E, self.size = int(E), int(size)
        self.rew, self.done = np.zeros(size, np.float32), np.zeros(size, np.float32)
        self.pos = np.full(size, -1, np.int64)
        self.flags = np.zeros(size, np.uint8) if tracked else None
        self.next_index = self.stored = 0

    def track(self):
        if self.flags is None:
            self.flags = np.zeros(self.size, np.uint8)
            if self.stored:
                base = (self.next_index - self.E) % self.size
                self.flags[base:base + self.E] = HEAD

    def mark(self, start, n, end):
        """the flag part of dgvit_ring_store_small"""
        assert 1 <= n <= self.size and self.size % n == 0 and 0 <= start < self.size
        j = np.arange(n)
        self.flags[(start + j) % self.size] = HEAD | np.where(np.asarray(end) != 0, END, 0).astype(np.uint8)
        if n < self.size:
            self.flags[(start - n + j) % self.size] &= END

    def add_vec(self, rew, done, t, end=None):
        """one vector step: environment e's transition t into slot next_index + e"""
        E = self.E
        rew, done = np.asarray(rew, np.float32).reshape(E), np.asarray(done, np.float32).reshape(E)
        assert self.next_index % E == 0
        slots = self.next_index + np.arange(E)
        self.rew[slots], self.done[slots], self.pos[slots] = rew, done, t
        if end is not None:
            self.track()
        if self.flags is not None:
            self.mark(self.next_index, E, np.zeros(E) if end is None else end)
        self.next_index = (self.next_index + E) % self.size
        self.stored = min(self.stored + E, self.size)

    def offer(self, strs, t):
        """step t of the streams, the ends passed as episode_end"""
        self.add_vec([s[t][0] for s in strs], [s[t][1] for s in strs], t, [s[t][2] for s in strs])

    def episode_end(self, envs):
        """on_episode_end(envs): a bool mask (E,) or indices"""
        assert self.stored
        self.track()
        envs = np.asarray(envs)
        mask = envs if envs.dtype == np.bool_ else np.isin(np.arange(self.E), envs)
        base = (self.next_index - self.E) % self.size
        self.flags[base:base + self.E] |= np.where(mask, END, 0).astype(np.uint8)

    def walk(self, idx, n, gamma, stride=None):
        """dgvit_nstep_walk_strided on the slots idx (stride = E): as nstep_ref.Ring.walk, lane k visiting (i + k stride) mod size"""
        self.track()
        stride, gamma = self.E if stride is None else int(stride), float(gamma)
        idx = np.clip(np.asarray(idx, np.int64).reshape(-1), 0, self.size - 1)
        out = {k: [] for k in ("ret64", "disc64", "steps", "tail", "done", "tol", "why")}
        for i in idx:
            slots, why = [], set()
            for k in range(n):
                s = (int(i) + k * stride) % self.size
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
            acc, g, mag = 0.0, 1.0, 0.0
            for s in slots:
                acc += g * float(self.rew[s])
                mag += g * abs(float(self.rew[s]))
                g *= gamma
            m = len(slots)
            out["ret64"].append(acc), out["disc64"].append(g), out["steps"].append(m), out["tail"].append(slots[-1])
            out["done"].append(self.done[slots[-1]]), out["why"].append(frozenset(why))
            out["tol"].append(2.0 ** -23 * abs(acc) + m * 2.0 ** -52 * mag)
        res = dict(ret64=np.array(out["ret64"], np.float64), disc64=np.array(out["disc64"], np.float64), steps=np.array(out["steps"], np.int32),
                   tail=np.array(out["tail"], np.int64), done=np.array(out["done"], np.float32), why=out["why"],
                   tol=np.array(out["tol"], np.float64))
        res["rew"], res["discount"] = res["ret64"].astype(np.float32), res["disc64"].astype(np.float32)
        return res
