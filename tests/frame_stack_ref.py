"""Frame stacks at sample time (dgvit_amd.replay: sample(..., frame_stack=K), FrameStack) restated in numpy on top of
vec_replay_ref.VecRing, a frame being ONE integer id as in shared_next_ref.

``StackRing`` is the ring model: driven by the same add_vec / on_episode_end stream as the buffers, it keeps per slot the ids of the two
frames stored there and restates dgvit_ring_stack_rows -- the n-step walk backward: predecessor k of slot s is (s - k E) mod size, linked
iff k E < size, it does not lie before slot 0 of a ring that is not full, and neither its flags nor its done stop a walk behind it.
``obs_stack`` / ``next_stack`` give the K ids of a slot's stacks, oldest channel first; ``next_stack`` takes the n-step tail and, for a
``shared_next_obs`` ring, the function that resolves a slot's next_obs (shared_next_ref.SharedRing.next_frame, lost frames included).

``truth_obs`` / ``truth_next`` state the same stacks a second time from each environment's own stream alone -- no ring in it: the frames
of steps t, t - 1, ... of ITS episode that are still stored, the oldest of them repeated.  They hold for rings that tracked episodes from
the first slot; what an oldest slot loses at the ring's seam is part of the truth (the frames are gone).

``render`` turns ids into the (H, W, K) fp32 stack the device returns, with an optional (dy, dx) applied to all channels: copies, so
every comparison is bit-exact."""
import numpy as np

import nstep_ref as N
import shared_next_ref as S
import vec_replay_ref as V

END, HEAD = N.END, N.HEAD
STACK_MAX = 16


class StackRing(V.VecRing):
    """VecRing with the ids of the obs and next_obs frame of every slot (-1: never written)"""

    def __init__(self, E, size, tracked=True):
        super().__init__(E, size, tracked)
        self.obs = np.full(size, -1, np.int64)
        self.nxt = np.full(size, -1, np.int64)

    def add_vec_frames(self, strs, frs, t, ends=True):
        """step t of E streams; ``ends``: pass the streams' ends as episode_end (which starts tracking), else store without"""
        slots = self.next_index + np.arange(self.E)
        if ends:
            self.offer(strs, t)
        else:
            self.add_vec([s[t][0] for s in strs], [s[t][1] for s in strs], t)
        self.obs[slots] = [f[t][0] for f in frs]
        self.nxt[slots] = [f[t][1] for f in frs]

    def clear(self):
        self.next_index = self.stored = 0
        if self.flags is not None:
            self.flags[:] = 0

    def preds(self, s, K, full=None):
        """[pred_0 .. pred_d] of slot s: itself and its d linked predecessors, d <= K - 1 (dgvit_ring_stack_rows).  ``full`` is the bit
        the kernel gets by value; None: the ring's own, stored == size"""
        self.track()
        full = self.stored == self.size if full is None else bool(full)
        s = min(max(int(s), 0), self.size - 1)
        out = [s]
        for k in range(1, K):
            if k * self.E >= self.size:
                break
            q = s - k * self.E
            if q < 0 and not full:
                break
            p = q % self.size
            if self.flags[p] != 0 or self.done[p] != 0:
                break
            out.append(p)
        return out

    def obs_stack(self, s, K, full=None):
        """the K obs ids of slot s's stack, channel 0 (the oldest) first"""
        p = self.preds(s, K, full)
        return [int(self.obs[p[min(K - 1 - c, len(p) - 1)]]) for c in range(K)]

    def next_stack(self, s, K, tail=None, next_frame=None, full=None):
        """the K ids of the next_obs stack of the transition that starts at s and ends at ``tail`` (None: s itself); ``next_frame``
        resolves a slot's next_obs (None: the two-matrix ring's own row)"""
        t = min(max(int(s if tail is None else tail), 0), self.size - 1)
        p = self.preds(t, K, full)
        ids = [int(self.obs[p[min(K - 2 - c, len(p) - 1)]]) for c in range(K - 1)]
        return ids + [int(self.nxt[t] if next_frame is None else next_frame(t))]


def episode_start(stream, t):
    """the first position of the episode that position t belongs to"""
    while t > 0 and not S.terminal(stream[t - 1]):
        t -= 1
    return t


def truth_obs(strs, frs, e, t, newest, K, E, size):
    """ids of the obs stack of environment e's transition t when step `newest` is the last one stored, from e's stream alone: steps
    t, t - 1, ... down to the first of t's episode that the ring still holds -- step newest - size / E + 1 is its oldest -- then that
    one repeated"""
    first = max(episode_start(strs[e], t), newest - size // E + 1, 0)
    assert first <= t <= newest
    return [frs[e][max(t - (K - 1 - c), first)][0] for c in range(K)]


def truth_next(strs, frs, e, t, newest, K, E, size, n=None, gamma=0.5):
    """ids of the next_obs stack: the n-step tail's next frame on top of the obs frames of the tail and the steps before it"""
    tail = t if n is None else N.truth(strs[e][:newest + 1], t, n, gamma)[3]
    below = truth_obs(strs, frs, e, tail, newest, K - 1, E, size) if K > 1 else []
    return below + [frs[e][tail][1]]


def render(ids, shape, shift=(0, 0)):
    """ids (K,) -> the (H, W, K) fp32 stack of k / 255 frames, every channel moved by the one (dy, dx) with its border replicated"""
    H, W = shape
    dy, dx = int(shift[0]), int(shift[1])
    yy = np.clip(np.arange(H) + dy, 0, H - 1)
    xx = np.clip(np.arange(W) + dx, 0, W - 1)
    return np.stack([S.pixels(i, shape)[np.ix_(yy, xx)] for i in ids], axis=-1)


def render_batch(stacks, shape, shifts=None):
    """[ids] per sample (+ (B, 2) shifts) -> (B, H, W, K) fp32"""
    return np.stack([render(ids, shape, (0, 0) if shifts is None else shifts[b]) for b, ids in enumerate(stacks)])
