"""The replay ring that stores each frame once (dgvit_amd.replay: DeviceReplayBuffer(shared_next_obs=True)) restated in numpy
on top of vec_replay_ref.VecRing / nstep_ref: the ``next_row`` table, the terminal pool's FIFO {head, tail, lost} and the frame arena, a
frame being ONE integer id.

``frames(stream)`` gives every transition of a (rew, done, end) stream its two frames as ids, honouring the buffer's contract: inside an
episode the obs of step t + 1 IS the next_obs of step t (the same id); the step behind an episode's last one (done != 0 or end) starts with
a frame never seen before.  Ids are unique over all streams that share a ``counter``.  The truth of a transition is then its own stream's
next id and nothing else: no ring in it.

``SharedRing`` is the store path in slot order, one row at a time (include/dgvit_hip.h: dgvit_ring_plan_next, steps 1-6, and
dgvit_ring_store_frames_shared): per row the move of the terminal predecessor's frame out of the lane's pending row, the obs row, and the
row's next_obs into the pending row.  ``fifo_truth`` states the FIFO rule a second time, on the streams alone: which transitions find the
pool full when their successor arrives.  ``pixels(id, shape)`` turns an id into a k / 255 frame for the device tests."""
import itertools

import numpy as np

import nstep_ref as N
import vec_replay_ref as V

END = N.END


def default_pool(size, E):
    """replay._shared_next's default terminal_frames"""
    return E * -(-(size // E) // 2)     # every other slot of every lane


def terminal(tr):
    """(rew, done, end): the n-step walk stops behind this transition"""
    return tr[1] != 0 or bool(tr[2])


def frames(stream, counter=None):
    """[(obs id, next_obs id)] per transition of the stream"""
    counter = itertools.count() if counter is None else counter
    out = []
    for t, _ in enumerate(stream):
        obs = out[t - 1][1] if t and not terminal(stream[t - 1]) else next(counter)
        out.append((obs, next(counter)))
    return out


def all_frames(strs):
    counter = itertools.count()
    return [frames(s, counter) for s in strs]


def pixels(fid, shape, codes=False):
    """frame id -> a (H, W) frame of values k / 255 (or the codes k, uint8); ids below 2^16 give different frames: the even pixels carry
    the id's low byte, the odd ones its high byte"""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    k = np.where(i % 2 == 0, i * 7 + int(fid) % 256, i * 5 + int(fid) // 256 % 256)
    k = (k % 256).astype(np.uint8).reshape(shape)
    return k if codes else k.astype(np.float32) / np.float32(255.0)


class SharedRing(V.VecRing):
    """VecRing (episodes tracked from the first slot) with the frame arena: ``arena`` (size + E + P ids, -1 = nothing), ``next_row``
    (size int32, -1 = never written), ``head`` / ``tail`` / ``lost``"""

    def __init__(self, E, size, P=None):
        super().__init__(E, size)
        self.P = default_pool(size, E) if P is None else int(P)
        assert 1 <= self.P <= size
        self.arena_rows = size + E + self.P
        self.arena = np.full(self.arena_rows, -1, np.int64)
        self.next_row = np.full(size, -1, np.int32)
        self.head = self.tail = self.lost = 0
        self.max_live = 0

    def _frames(self, start, n, obs, nxt):
        """the bookkeeping and the frames of n rows at `start`, after their small fields and marks are in the ring"""
        E, size, P = self.E, self.size, self.P
        pool = size + E
        for j in range(n):
            s = (start + j) % size
            pending = size + s % E
            if self.next_row[s] >= pool:                       # 1. the overwritten slot's pool entry is free
                self.head += 1
            self.next_row[s] = pending                         # 2.
            p = (s - E) % size
            if size > E and self.next_row[p] != -1 and (j >= E or n < size):   # 3. the lane predecessor, unless this call overwrites it
                if not (self.done[p] != 0 or self.flags[p] & END):
                    self.next_row[p] = s                       # 4. its next_obs is this row's obs
                elif self.tail - self.head < P:                # 5. into the pool, out of the pending row
                    row = pool + self.tail % P
                    self.next_row[p] = row
                    self.arena[row] = self.arena[pending]
                    self.tail += 1
                else:                                          # 6. lost: its own obs stands in
                    self.next_row[p] = p
                    self.lost += 1
            self.max_live = max(self.max_live, self.tail - self.head)
            self.arena[s] = obs[j]
            self.arena[pending] = nxt[j]

    def add_vec_frames(self, strs, frs, t):
        """step t of E streams: VecRing.offer, then the frames"""
        start = self.next_index
        self.offer(strs, t)
        self._frames(start, self.E, [f[t][0] for f in frs], [f[t][1] for f in frs])

    def store(self, stream, frs, ts):
        """add (one position) / add_batch (several) of a single-environment ring: nstep_ref.Ring.store's slots and marks, then the frames"""
        assert self.E == 1
        ts = list(ts)[-self.size:]
        n, start = len(ts), self.next_index
        slots = (start + np.arange(n)) % self.size
        self.rew[slots], self.done[slots], self.pos[slots] = [stream[t][0] for t in ts], [stream[t][1] for t in ts], ts
        N.Ring.mark(self, start, n)
        self.next_index = (start + n) % self.size
        self.stored = min(self.stored + n, self.size)
        self._frames(start, n, [frs[t][0] for t in ts], [frs[t][1] for t in ts])

    def next_frame(self, s):
        """the id sample() returns as next_obs of slot s"""
        return int(self.arena[self.next_row[s]])

    def state(self):
        return [self.head, self.tail, self.lost]


def fifo_truth(strs, E, size, P, steps):
    """The FIFO rule on the streams alone, after `steps` vector steps: (lost, live) -- ``lost`` the set of (e, t) still in the ring whose
    successor found the pool full, ``live`` the transitions that own a pool entry, oldest first.  Transition (e, t) leaves the ring when
    step t + size / E is stored; its successor is (e, t + 1)."""
    depth = size // E
    live, lost = [], set()
    for T in range(steps):
        for e in range(E):
            gone = (e, T - depth)
            if live and live[0] == gone:
                live.pop(0)
            lost.discard(gone)
            if T >= 1 and depth > 1 and terminal(strs[e][T - 1]):
                if len(live) < P:
                    live.append((e, T - 1))
                else:
                    lost.add((e, T - 1))
    return lost, live
