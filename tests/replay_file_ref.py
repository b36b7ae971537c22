"""The replay ring as a file (dgvit_amd.replay: save_transitions / load_transitions) restated in numpy: the layout of an
exported chunk (``layout``, what dgvit_ring_export packs and replay.export_layout returns) and the arrays of a save_transitions directory
(``expected``), built from the streams the other references generate -- vec_replay_ref.streams, nstep_ref.scenario and the frame ids of
shared_next_ref -- and from their numpy rings, which say where a transition lies and which flags it has.

The format.  Transitions are numbered by AGE: age a lies in slot (oldest + a) % size, oldest = next_index when the ring is full, else 0.
Every field file has first axis = age; frames are dense (H, W) rows in the ring's own format (uint8 codes or the fp32 values code / 255);
``end`` is one byte per transition, bit 0 = the slot's END flag (zeros when episodes were never tracked); ``next_obs`` of a shared ring
is the frame the slot resolves to: its stream's next frame, or the slot's own obs where the terminal pool lost it.

A chunk of n transitions is field-major: obs, next_obs, pobs, act, rew, next_pobs, done, end and, with a tree, priority; block b starts
at off_b, off_0 = 0, off_{b+1} = the next multiple of 16 at or behind off_b + bytes_b."""
import numpy as np

import nstep_ref as N
import shared_next_ref as S

FIELDS = ("obs", "next_obs", "pobs", "act", "rew", "next_pobs", "done")
FRAMES = ("obs", "next_obs")
END = N.END
META_KEYS = ("format_version", "stored", "size", "num_envs", "oldest_slot", "next_index", "obs_shape", "pstate_dim", "act_dim", "frame_dtype",
             "shared_next_obs", "terminal_frames", "lost_terminal_frames", "episodes_tracked", "prioritized", "alpha", "eps", "max_leaf_bits",
             "update_max_bits")


def layout(n, obs_shape, pstate_dim, act_dim, itemsize, prioritized=False):
    """({block: (byte offset, bytes)}, bytes of the chunk)"""
    hw = int(obs_shape[0]) * int(obs_shape[1])
    sizes = [("obs", n * hw * itemsize), ("next_obs", n * hw * itemsize), ("pobs", n * pstate_dim * 4), ("act", n * act_dim * 4),
             ("rew", n * 4), ("next_pobs", n * pstate_dim * 4), ("done", n * 4), ("end", n)]
    if prioritized:
        sizes.append(("priority", n * 4))
    blocks, off = {}, 0
    for k, b in sizes:
        assert off % 16 == 0
        blocks[k] = (off, b)
        off = -(-(off + b) // 16) * 16
    return blocks, off


def without_ends(strs):
    """the streams with every `end` dropped: episodes end by done alone (where an `end` stood the episode simply goes on)"""
    return [[(r, d, False) for r, d, _ in s] for s in strs]


def data(strs, frs, shape):
    """data[k][t, e]: field k of environment e's transition t; the frames from their ids (shared_next_ref.pixels), as the exact floats
    code / 255 and, under data["codes"], as the codes; pobs, next_pobs and act seeded normals; rew, done and end the streams'"""
    T, E = len(strs[0]), len(strs)
    g = np.random.default_rng(100 * E + T)
    d = {"codes": {}}
    for j, k in enumerate(FRAMES):
        d["codes"][k] = np.stack([np.stack([S.pixels(frs[e][t][j], shape, codes=True) for e in range(E)]) for t in range(T)])
        d[k] = d["codes"][k].astype(np.float32) / np.float32(255.0)
    d.update({k: g.standard_normal((T, E, 2)).astype(np.float32) for k in ("pobs", "next_pobs", "act")})
    d["rew"] = np.array([[[s[t][0]] for s in strs] for t in range(T)], np.float32)
    d["done"] = np.array([[[s[t][1]] for s in strs] for t in range(T)], np.float32)
    d["end"] = np.array([[s[t][2] for s in strs] for t in range(T)], bool)
    return d


def ages(ring):
    """(slots, t, e) of the stored transitions of a numpy ring (nstep_ref.Ring, vec_replay_ref.VecRing, shared_next_ref.SharedRing),
    oldest first"""
    E = getattr(ring, "E", 1)
    oldest = ring.next_index if ring.stored == ring.size else 0
    slots = (oldest + np.arange(ring.stored)) % ring.size
    return slots, ring.pos[slots], slots % E


def expected(ring, d, shape, u8):
    """{file name: array} of the save_transitions directory of a device ring that took the calls the numpy ``ring`` took, fed from ``d``"""
    slots, t, e = ages(ring)
    assert (t >= 0).all()
    out = {k: ((d["codes"][k] if u8 else d[k]) if k in FRAMES else d[k])[t, e] for k in FIELDS}
    if isinstance(ring, S.SharedRing):          # what the slot resolves to, by frame id
        codes = np.stack([S.pixels(ring.next_frame(s), shape, codes=True) for s in slots])
        out["next_obs"] = codes if u8 else codes.astype(np.float32) / np.float32(255.0)
    out["end"] = (ring.flags[slots] & END).astype(np.uint8) if ring.flags is not None else np.zeros(ring.stored, np.uint8)
    return out


def stream_order(ring):
    """the same ages from the streams alone: the last stored // E steps, step-major, environment-minor (a ring fed by whole vector steps)"""
    E = getattr(ring, "E", 1)
    newest = int(ring.pos.max())
    first = newest + 1 - ring.stored // E
    return np.repeat(np.arange(first, newest + 1), E), np.tile(np.arange(E), ring.stored // E)
