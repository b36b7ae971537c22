"""Device-resident replay storage and sampling.

The reference keeps transitions in a host-side ``cpprb.PrioritizedReplayBuffer`` used as a plain uniform sampler
(priorities are never updated, DRL.py:80-100, 365-368) and, every ``learn()``, converts the sampled numpy batch to
tensors and copies it to the device synchronously from pageable memory (DRL.py:375-386): 2 x (B,128,160) fp32 =
84 MB at B=512.  An MI355X has 288 GB of HBM: 100k transitions of two 128x160 fp32 frames are 16 GB, so the ring
lives on the device, ``store_transition`` becomes one small H2D copy per environment step, and ``sample`` is an
index draw plus one HBM-bound gather kernel per field -- the encoder never waits for PCIe.  The reference's frames are k / 255 with k in
0..255 (env_lab.py:420-434, 348-349), so ``frame_dtype=torch.uint8`` stores them as bytes, a quarter of the ring, and the gather restores
the fp32 frame.

Consecutive ring slots are consecutive environment steps, so ``sample(..., n_step=n, gamma=g)`` returns multi-step transitions -- cpprb's
``Nstep`` option -- by a walk along the ring at sample time: nothing extra is stored and n and gamma may change from call
to call.  What a walk may not cross is kept in ``episode_flags``, one byte per slot on the device.  With ``num_envs=E`` the ring holds E
parallel environments, a vector step in E consecutive slots, and an environment's steps lie E slots apart: ``add_vec``
stores such a step from device tensors without visiting the host.  ``shared_next_obs=True`` stores each frame once: a transition's
``next_obs`` is its successor's ``obs`` row, and only the frames without a successor slot are kept apart.
``sample(..., frame_stack=K)`` returns channel-last stacks of the last K frames of each slot's episode, built at sample time by the same
walk run backward, and ``FrameStack`` keeps that stack on the acting side: the ring never stores a frame twice.
``sample_mixed`` draws one batch from several rings -- the agent's and a demonstration ring -- each ring's launches writing straight into
its row range of the shared tensors, and ``update_priorities_mixed`` routes the TD errors back.  There is one sampling
path: ``sample``, the prioritized ``sample`` and ``sample_mixed`` check their keywords, make one batch (``_Rows``), let each ring issue
its launches into its rows of it (``_sample_rows``) and shape the result in one place (``_finish``).

Field names follow the reference's buffer (DRL.py:80-100): obs, pobs, act, rew, next_obs, next_pobs, done.
"""
import json
import os
import shutil
from typing import Dict, Optional, Tuple

import numpy as np
from numpy.lib.format import open_memmap
import torch

from . import _lib
from .functional import _ptr, _seed_args, _stream
from .preprocess import _gather_shift, _shift_pad, _shift_seed


def _al4(n: int) -> int:
    return (n + 3) & ~3


def _al16(n: int) -> int:
    return (n + 15) & ~15


FRAME_FIELDS = ("obs", "next_obs")
FLAG_END, FLAG_HEAD = 1, 2  # include/dgvit_hip.h: DGVIT_RING_END, DGVIT_RING_HEAD (bits of episode_flags)
_INDEX_DTYPES = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)
NSTEP_MAX = 64              # one lane of a wave per visited slot


def _frame_dtype(dtype):
    """``frame_dtype`` after its check: host-only, runs before anything touches a device"""
    if dtype is not torch.float32 and dtype is not torch.uint8:
        raise ValueError(f"frame_dtype must be torch.float32 or torch.uint8, got {dtype!r}")
    return dtype


def _n_step(n):
    """``n_step`` after its check (None: one-step sampling): host-only, runs before anything touches a device"""
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= NSTEP_MAX:
        raise ValueError(f"n_step must be None or an int in [1, {NSTEP_MAX}], got {n!r}")
    return int(n)


STACK_MAX = 16              # one lane of a wave per predecessor (csrc/replay_ring.hip: STACK_MAX)


def _frame_stack(k, what="frame_stack"):
    """``frame_stack`` (None: single frames) or ``frames`` after its check: host-only, runs before anything touches a device"""
    if k is None:
        return None
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= STACK_MAX:
        raise ValueError(f"{what} must be {'None or ' if what == 'frame_stack' else ''}an int in [1, {STACK_MAX}], got {k!r}")
    return int(k)


def _num_envs(num_envs, size):
    """``num_envs`` after its check: host-only, runs before anything touches a device"""
    if isinstance(num_envs, bool) or not isinstance(num_envs, (int, np.integer)) or not 1 <= int(num_envs) <= int(size) \
            or int(size) % int(num_envs):
        raise ValueError(f"num_envs must be an int in [1, size] that divides size={int(size)}, got {num_envs!r}")
    return int(num_envs)


def _shared_next(shared, terminal_frames, size, num_envs):
    """``shared_next_obs`` and ``terminal_frames`` after their checks (``size`` and ``num_envs`` have passed theirs) -> (bool, P or None):
    host-only, runs before anything touches a device"""
    if not isinstance(shared, (bool, np.bool_)):
        raise ValueError(f"shared_next_obs must be a bool, got {shared!r}")
    if terminal_frames is None:
        return bool(shared), num_envs * -(-(size // num_envs) // 2) if shared else None   # every other slot of every lane
    if not shared:
        raise ValueError(f"terminal_frames={terminal_frames!r} sizes the terminal pool of a shared ring: pass shared_next_obs=True with it")
    if isinstance(terminal_frames, bool) or not isinstance(terminal_frames, (int, np.integer)) or not 1 <= int(terminal_frames) <= size:
        raise ValueError(f"terminal_frames must be None or an int in [1, size] = [1, {size}], got {terminal_frames!r}")
    return True, int(terminal_frames)


SMALL_FIELDS = ("pobs", "act", "rew", "next_pobs", "done")   # what one dgvit_ring_store_small launch stores
_NO_SHIFTS = dict.fromkeys(FRAME_FIELDS)                     # a sample that returns no shift tables: no launch writes one

# ---- the ring as a file
FILE_FIELDS = FRAME_FIELDS + SMALL_FIELDS    # the field files of save_transitions and the blocks of a chunk, in this order
FILE_FORMAT_VERSION = 1
LOAD_CHUNK = 4096                            # transitions per host -> device copy of load_transitions
META_KEYS = ("format_version", "stored", "size", "num_envs", "oldest_slot", "next_index", "obs_shape", "pstate_dim", "act_dim", "frame_dtype",
             "shared_next_obs", "terminal_frames", "lost_terminal_frames", "episodes_tracked", "prioritized", "alpha", "eps", "max_leaf_bits",
             "update_max_bits")


def export_layout(n: int, obs_shape, pstate_dim: int, act_dim: int, frame_dtype, prioritized: bool = False):
    """({block: (byte offset, bytes)}, bytes of the whole chunk) of n transitions as dgvit_ring_export packs them (include/dgvit_hip.h):
    field-major, the blocks ``FILE_FIELDS`` in their order -- n dense rows each, a frame row H*W elements of ``frame_dtype``, the small
    fields fp32 -- then ``end``, n bytes, and ``priority``, n fp32 leaves, when ``prioritized``.  Every block starts at a multiple of 16
    bytes.  Host-only."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 1:
        raise ValueError(f"n must be an int >= 1, got {n!r}")
    n, item = int(n), 1 if _frame_dtype(frame_dtype) is torch.uint8 else 4
    cols = {"obs": int(np.prod(obs_shape)) * item, "next_obs": int(np.prod(obs_shape)) * item, "pobs": 4 * int(pstate_dim),
            "act": 4 * int(act_dim), "rew": 4, "next_pobs": 4 * int(pstate_dim), "done": 4, "end": 1}
    if prioritized:
        cols["priority"] = 4
    blocks, off = {}, 0
    for k in (*FILE_FIELDS, "end", "priority")[:len(cols)]:
        blocks[k] = (off, n * cols[k])
        off = _al16(off + n * cols[k])
    return blocks, off


def _chunk(chunk):
    """``chunk`` after its check: host-only, runs before anything touches a device"""
    if isinstance(chunk, bool) or not isinstance(chunk, (int, np.integer)) or int(chunk) < 1:
        raise ValueError(f"chunk must be an int >= 1 (transitions per device -> host copy), got {chunk!r}")
    return int(chunk)


def _load_options(priorities, restore_rng):
    """``priorities`` and ``restore_rng`` of load_transitions after their checks: host-only, runs before anything touches a device"""
    if not isinstance(priorities, str) or priorities not in ("file", "reset"):
        raise ValueError(f"priorities must be 'file' or 'reset', got {priorities!r}")
    if restore_rng is not None and not isinstance(restore_rng, (bool, np.bool_)):
        raise ValueError(f"restore_rng must be None, True or False, got {restore_rng!r}")
    return priorities, None if restore_rng is None else bool(restore_rng)


class _Rows:
    """The raw buffers of one batch, every sampling call's: tensors of ``total`` rows, one per output name, allocated when a launch first
    asks for it.  A ring writes rows [r0, r0 + n) of each: all of them in its own ``sample`` -- the tensor itself is then handed out, not
    a slice of it -- and its share in ``sample_mixed``, which moves ``r0`` from ring to ring.  ``_finish`` makes the result of them."""

    def __init__(self, total, device):
        self.total, self.device, self.r0, self.bufs = total, device, 0, {}

    def empty(self, name, n, tail, dtype):
        buf = self.bufs.get(name)
        if buf is None:
            buf = self.bufs[name] = torch.empty(self.total, *tail, dtype=dtype, device=self.device)
        return buf if n == self.total else buf[self.r0:self.r0 + n]       # (the whole tensor: r0 is 0 then)


def _dense(buf, cols):
    """a raw (B, al4(cols)) buffer without its row padding: the buffer itself where there is none (the slice would be its twin)"""
    return buf if cols % 4 == 0 else buf[:, :cols]


def _finish(batch, fields, shapes, pad, return_shifts, n_step, K):
    """The result dict of ``sample`` and of ``sample_mixed`` out of a batch's raw buffers, the one place where an output is shaped: the
    row padding goes, a field takes its ``shapes[k]`` -- ``rew``, ``done`` and ``discount`` (B, 1), a stack (B, H, W, K) by the call's one
    ``.contiguous()``, a copy only where H W K is no multiple of 4 -- and ``return_shifts`` without a shift gets its tables of zeros."""
    out, bufs, B = {}, batch.bufs, batch.total
    for k, cols in fields.items():
        buf = bufs[k]
        if K is not None and k in FRAME_FIELDS:
            out[k] = _dense(buf, cols * K).reshape(B, *shapes[k], K).contiguous()
        elif n_step is not None and k in ("rew", "done"):     # the walk's own, one value a row
            out[k] = buf.view(B, 1)
        else:
            out[k] = _dense(buf, cols).reshape(B, *shapes[k])
        if return_shifts and k in FRAME_FIELDS:
            out[k + "_shift"] = bufs[k + "_shift"] if pad else torch.zeros(B, 2, dtype=torch.int32, device=batch.device)
    if n_step is not None:
        out["discount"], out["steps"] = bufs["discount"].view(B, 1), bufs["steps"]
    out["indexes"] = bufs["indexes"]
    if "weights" in bufs:
        out["weights"] = bufs["weights"]
    return out


class DeviceReplayBuffer:
    """The replay ring in HBM.  ``frame_dtype=torch.uint8`` (keyword-only; default ``torch.float32``) stores ``obs`` and ``next_obs`` as
    one byte per pixel, a quarter of the fp32 ring: ``store["obs"]`` and ``store["next_obs"]`` are then
    ``(size, al16(H*W))`` uint8 matrices, the other fields unchanged.  The stored value is code / 255: a frame given as floats is
    quantised on the device, code = rint(clamp(255 x, 0, 255)) with halves to even, so inputs outside [0, 1] clamp (NaN stores 0); this
    is exact for the reference's k / 255 frames and round-to-nearest otherwise (error at most 1/510 + 2^-23).  ``sample`` returns fp32
    frames, bit-equal to numpy's and CPU torch's ``codes / 255`` in fp32.  With a uint8 ring ``add`` / ``add_batch`` take each frame
    field, independently, as host floats (they travel in the one staged matrix and are quantised from it), as host uint8 (numpy or CPU
    tensor: the codes themselves, four to a float of the same matrix) or as a device tensor, fp32 or uint8.  A device tensor given to
    ``add`` / ``add_batch`` never visits the host, whatever the ring's format and whichever field it is.
    ``save_transitions`` / ``load_transitions`` / ``clear`` keep the ring beyond the process.

    Episodes.  ``episode_flags`` is None until ``track_episodes()``, ``on_episode_end()`` or ``sample(n_step=...)`` is first
    used; from then on it is a (size,) uint8 device tensor that the store path keeps current, inside the second launch of an ``add`` or
    ``add_vec`` and with one more launch per ``add_batch``: bit 0 (END) marks the last transition of an episode, whatever its ``done`` says (time limits, truncations -- the
    reference fetches ``done`` and never applies it, so ``done`` alone cannot mark episodes), bit 1 (HEAD) the newest slot written.  A
    buffer that never uses them allocates nothing and launches nothing more than before.  Episode ends before tracking started are
    unknown, apart from ``done``: call ``track_episodes()`` before the first ``add`` if n-step sampling is meant.  ``add_batch`` writes
    consecutive slots, so demonstrations go in one episode per call, each followed by ``on_episode_end()`` -- or rely on their ``done``.

    Parallel environments.  ``num_envs=E`` (keyword-only; an int in [1, size] that divides ``size``; default 1) gives the ring
    a second axis: ``add_vec`` stores one step of E environments in the E consecutive slots ``base .. base + E - 1``, ``base`` a multiple
    of E, environment e in slot ``base + e``.  The successor of slot s in its episode is ``(s + E) % size``, and because E divides ``size``
    the lane ``s % E`` survives the wrap; ``sample(n_step=...)`` walks with that stride, ``idx % num_envs`` is a sampled slot's
    environment, and ``stored`` / ``next_index`` keep counting slots.  HEAD then marks the E newest slots.  With E > 1 ``add`` and
    ``add_batch`` are refused (a demonstration episode has no lane) and ``on_episode_end`` takes the environments that ended.

    Each frame once.  ``shared_next_obs=True`` (keyword-only; default False, which changes nothing) keeps ONE frame arena,
    ``self.arena``, of ``arena_rows = size + num_envs + terminal_frames`` rows in the ring's frame format in the place of the two frame
    matrices.  The contract: inside an episode, the ``obs`` of a lane's step t + 1 is the frame that was ``next_obs`` of its step t --
    what every environment loop passes anyway.  That ``next_obs`` is then not kept: the successor's ``obs`` row is it.  Rows [0, size)
    of the arena are the ``obs`` ring (``store["obs"]`` is that view, and ``store`` has no ``"next_obs"``), rows [size, size + E) one
    *pending* row per lane with the ``next_obs`` of the lane's newest transition, and the last ``terminal_frames`` rows a FIFO pool for
    the ``next_obs`` of transitions that ended an episode -- END flag or ``done != 0``, where the n-step walk stops too -- and are still
    in the ring.  ``add``, ``add_batch`` and ``add_vec`` keep their keywords (``next_obs`` is still passed), ``sample`` returns the same
    batches, and the constructor starts ``track_episodes()``.  ``terminal_frames=P`` (an int in [1, size]) sizes the pool; when more
    than P ended transitions are in the ring at once the newest of them lose their last frame (``lost_terminal_frames()``).  The
    default is ``E * ceil(size / E / 2)``, every other slot of every lane: it cannot overflow while episodes last two steps or more,
    because two neighbouring slots of a lane are then never both an episode's last.  Where episodes are known to be long, a smaller
    pool saves more: ``size // L`` entries and some slack serve episodes of L steps.  The frames take (size + E + P) rows against
    2 size."""

    def __init__(self, size: int, obs_shape: Tuple[int, int] = (128, 160), pstate_dim: int = 2, act_dim: int = 2,
                 device="cuda", seed: Optional[int] = None, *, frame_dtype=torch.float32, num_envs=1, shared_next_obs=False,
                 terminal_frames=None):
        self.frame_dtype = _frame_dtype(frame_dtype)
        self.num_envs = _num_envs(num_envs, size)
        self.shared_next_obs, self.terminal_frames = _shared_next(shared_next_obs, terminal_frames, int(size), self.num_envs)
        self.size, self.device = int(size), torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DgvitError("DeviceReplayBuffer lives in HBM; pass a ROCm device")
        self.fields = {"obs": int(np.prod(obs_shape)), "pobs": pstate_dim, "act": act_dim, "rew": 1,
                       "next_obs": int(np.prod(obs_shape)), "next_pobs": pstate_dim, "done": 1}
        self.shapes = {"obs": tuple(obs_shape), "next_obs": tuple(obs_shape), "pobs": (pstate_dim,), "next_pobs": (pstate_dim,),
                       "act": (act_dim,), "rew": (1,), "done": (1,)}
        # every field is a (size, row) fp32 matrix whose row length is padded to a multiple of 4 floats (float4 gather)
        self.rows = {k: _al4(n) for k, n in self.fields.items()}
        # where the frames live, said once.  frame_ld: the row stride of a frame matrix in elements -- al16(H*W) bytes on a uint8 ring
        # (``row_bytes`` there; the rows sample() returns stay al4(H*W) floats), al4(H*W) floats on an fp32 ring
        shared = self.shared_next_obs
        self.frame_ld = self.rows["obs"]
        if self.frame_dtype is torch.uint8:
            self.frame_ld = self.row_bytes = _al16(self.fields["obs"])
        self.arena = self.arena_rows = None
        if shared:                               # one arena of size + E + P frame rows; store["obs"] is its first `size` rows
            self.arena_rows = self.size + self.num_envs + self.terminal_frames
            self.arena = torch.zeros(self.arena_rows, self.frame_ld, dtype=self.frame_dtype, device=self.device)
        self.store = {}
        for k, r in self.rows.items():
            if k not in FRAME_FIELDS:
                self.store[k] = torch.zeros(self.size, r, dtype=torch.float32, device=self.device)
            elif not shared:
                self.store[k] = torch.zeros(self.size, self.frame_ld, dtype=self.frame_dtype, device=self.device)
            elif k == "obs":                     # (a shared ring has no store["next_obs"])
                self.store[k] = self.arena[:self.size]
        # the matrix next_obs is gathered from, and its rows: the arena at the rows ``next_row`` names, or the field's own matrix
        self.next_frames, self.next_frame_rows = (self.arena, self.arena_rows) if shared else (self.store["next_obs"], self.size)
        if shared:
            self.next_row = torch.full((self.size,), -1, dtype=torch.int32, device=self.device)    # the arena row of each slot's next_obs
            self._pool_state = torch.zeros(3, dtype=torch.int64, device=self.device)               # head, tail, lost of the pool's FIFO
            self._step_moves = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)   # a step's move list, rewritten per store
        self.next_index, self.stored = 0, 0
        self.episode_flags = None                # (size,) uint8 once episodes are tracked
        self.gen = torch.Generator(device=self.device)
        if seed is not None:
            self.gen.manual_seed(int(seed))
        if self.shared_next_obs:                 # the bookkeeping reads END from the first slot on
            self.track_episodes()

    def lost_terminal_frames(self) -> int:
        """How many transitions that ended an episode found the terminal pool full when their successor was stored (a shared ring; 0 on
        any other).  Such a slot returns its own ``obs`` as ``next_obs``.  A non-zero value means that ``terminal_frames`` is too small
        for the episode lengths: more than that many ended transitions were in the ring at once.  A device read: it synchronises."""
        return int(self._pool_state[2].item()) if self.shared_next_obs else 0

    def get_stored_size(self) -> int:
        return self.stored

    def _on_store(self, start: int, n: int) -> None:
        """hook: ring slots start .. start + n - 1 (mod size) have just been written"""

    def track_episodes(self) -> None:
        """Start keeping ``episode_flags`` (idempotent).  On allocation the flags are zeros with HEAD on the newest slot (the
        ``num_envs`` slots of the newest vector step), if anything is stored: episode ends from before are unknown, apart from ``done``.
        The allocation cannot happen inside a stream capture."""
        if self.episode_flags is not None:
            return
        if torch.cuda.is_current_stream_capturing():
            raise _lib.DgvitError("track_episodes() allocates the episode flags, which a stream capture cannot: call it (or on_episode_end(), "
                                  "or an eager sample(n_step=...)) before capturing")
        flags = torch.zeros(self.size, dtype=torch.uint8, device=self.device)
        if self.stored and self.num_envs == 1:
            flags[(self.next_index - 1) % self.size] = FLAG_HEAD
        elif self.stored:                        # the newest vector step: base is a multiple of num_envs, so the slice does not wrap
            base = (self.next_index - self.num_envs) % self.size
            flags[base:base + self.num_envs] = FLAG_HEAD
        self.episode_flags = flags

    def on_episode_end(self, envs=None) -> None:
        """The newest transition is the last of its episode, whatever its ``done`` says (cpprb's name): ORs END into its flags on the
        device, without a host synchronisation.  With ``num_envs > 1`` ``envs`` says whose: a bool mask (E,) or an integer index tensor or
        array, on the host or on the device (a device mask or index never visits the host); with ``num_envs == 1`` it must be None."""
        E = self.num_envs
        if E == 1 and envs is not None:
            raise ValueError("on_episode_end(envs=...) is for buffers with num_envs > 1; this one has a single environment")
        if E > 1 and envs is None:
            raise ValueError(f"on_episode_end() on a buffer with num_envs={E} needs envs=: a bool mask ({E},) or the indices of the "
                             "environments whose episode ended")
        if self.stored == 0:
            raise RuntimeError("on_episode_end() on an empty buffer: there is no newest transition")
        self.track_episodes()
        if E == 1:
            newest = (self.next_index - 1) % self.size
            self.episode_flags[newest:newest + 1].bitwise_or_(FLAG_END)
            return
        if not (torch.is_tensor(envs) and envs.device.type != "cpu"):
            envs = np.asarray(envs.numpy() if torch.is_tensor(envs) else envs)
            envs = torch.from_numpy(np.ascontiguousarray(envs if envs.size else envs.astype(np.int64)))     # [] : nobody's episode ended
            if envs.dtype != torch.bool and envs.numel() and not (envs.dtype in _INDEX_DTYPES and 0 <= int(envs.min()) and int(envs.max()) < E):
                raise ValueError(f"envs: indices must be integers in [0, {E}), got {envs.tolist()!r}")
            envs = envs.to(self.device)
        elif envs.device != self.episode_flags.device:
            raise ValueError(f"envs: the tensor is on {envs.device}, the ring on {self.episode_flags.device}")
        if envs.dtype == torch.bool:
            if tuple(envs.shape) != (E,):
                raise ValueError(f"envs: a mask must be ({E},), got {tuple(envs.shape)}")
            mask = envs.to(torch.uint8)          # END is bit 0: the mask as bytes is what is ORed in
        elif envs.dtype in _INDEX_DTYPES:
            mask = torch.zeros(E, dtype=torch.uint8, device=self.device).index_fill_(0, envs.reshape(-1).to(torch.int64), FLAG_END)
        else:
            raise ValueError(f"envs must be a bool mask or an integer index tensor or array, got dtype {envs.dtype}")
        base = (self.next_index - E) % self.size
        self.episode_flags[base:base + E].bitwise_or_(mask)

    def _travel(self, k, v, n):
        """Field k of n transitions as add / add_batch take it -- any dtype, a tensor on any device, a scalar for ``rew`` / ``done``, any
        shape that reshapes to (n, cnt); uint8 means codes for a frame field of a uint8 ring and the values 0..255 everywhere else -- in
        the form ``_vec_field`` returns.  A device tensor stays on the device and is converted there if it must be."""
        codes_ok = self.frame_dtype is torch.uint8 and k in FRAME_FIELDS
        if torch.is_tensor(v) and v.device.type != "cpu":
            v = v.detach().to(self.device)
            v = (v if v.dtype == torch.float32 or (codes_ok and v.dtype == torch.uint8) else v.float()).reshape(n, -1).contiguous()
        else:
            if torch.is_tensor(v):
                v = (v if v.dtype == torch.uint8 else v.detach().float()).numpy()
            v = np.asarray(v)
            v = np.ascontiguousarray(v.reshape(n, -1), dtype=np.uint8 if codes_ok and v.dtype == np.uint8 else np.float32)
        if v.shape[1] != self.fields[k]:
            raise ValueError(f"{k}: expected {self.fields[k]} values per transition, got {v.shape[1]}")
        return v

    def _commit(self, rows, n, end=None) -> None:
        """The one store path of add, add_batch and add_vec: ``rows`` holds every field of n <= size transitions as ``_vec_field`` returns
        it, ``end`` the episode ends of an ``add_vec``, normalised.  Every host field's columns lie side by side in ONE staged fp32 matrix,
        each block a multiple of 4 floats wide (codes four to a float), and behind its n rows the n ends of a host ``end``: one
        host->device copy from pinned memory -- the reference converts and copies every field of every sampled batch instead
        (DRL.py:379-386).  Which fields the matrix holds is the call's, so its column offsets are too.  Then dgvit_ring_store_frames for
        ``obs`` and ``next_obs`` and dgvit_ring_store_small for the other five fields, both wrapping the ring per row.  The marks of one
        step (n == num_envs: ``add``, ``add_vec``) are the second launch's; a longer run of one episode's slots (``add_batch``) is marked
        by dgvit_ring_mark, only its last slot the HEAD, and only when episodes are tracked.  A ``shared_next_obs`` ring stores its frames
        last and in another way: dgvit_ring_plan_next, the bookkeeping of ``next_row`` and the terminal pool, which reads ``done`` and END of
        the slots before the new ones from the ring, and dgvit_ring_store_frames_shared into the one arena."""
        off, row = {}, 0
        for k, v in rows.items():
            if not torch.is_tensor(v):
                off[k] = row
                row += _al4(self.fields[k]) if v.dtype == np.float32 else _al4(_al4(self.fields[k]) // 4)
        host_end = end is not None and not torch.is_tensor(end)
        dev = None
        if off or host_end:
            host = np.zeros(n * row + (n if host_end else 0), dtype=np.float32)
            mat = host[:n * row].reshape(n, row)
            for k, o in off.items():
                if rows[k].dtype == np.float32:
                    mat[:, o:o + self.fields[k]] = rows[k]
                else:
                    mat.view(np.uint8)[:, 4 * o:4 * o + self.fields[k]] = rows[k]
            if host_end:
                host[n * row:] = end
            stage = torch.from_numpy(host).pin_memory()
            dev = stage.to(self.device, non_blocking=True)
            self._last_stage = [stage, dev]      # keep the pinned buffer alive until the async copy has certainly been issued

        def source(k):
            """(pointer, 1 for uint8 codes, row stride in elements) of field k's rows on the device"""
            v = rows[k]
            if torch.is_tensor(v):
                return v.data_ptr(), int(v.dtype == torch.uint8), self.fields[k]
            codes = v.dtype == np.uint8
            return dev.data_ptr() + 4 * off[k], int(codes), 4 * row if codes else row

        lib, st, i = _lib.load(), _stream(), self.next_index
        u8 = self.frame_dtype is torch.uint8
        small = _lib.dgvit_small_fields()
        for j, k in enumerate(SMALL_FIELDS):
            small.src[j], _, small.src_ld[j] = source(k)
            small.ring[j], small.cols[j], small.ring_ld[j] = self.store[k].data_ptr(), self.fields[k], self.rows[k]
        end_ptr = None if end is None else (end.data_ptr() if torch.is_tensor(end) else dev.data_ptr() + 4 * n * row)
        end_f32 = int(host_end or (end is not None and end.dtype == torch.float32))
        step = n == self.num_envs
        with torch.cuda.device(self.device):
            (p0, c0, ld0), (p1, c1, ld1) = source("obs"), source("next_obs")
            if not self.shared_next_obs:
                rc = lib.dgvit_ring_store_frames(p0, c0, ld0, p1, c1, ld1, _ptr(self.store["obs"]), _ptr(self.store["next_obs"]), int(u8),
                                                 self.frame_ld, n, self.fields["obs"], self.size, i, st)
                _lib.check(rc, "dgvit_ring_store_frames")
            rc = lib.dgvit_ring_store_small(small, _ptr(self.episode_flags if step else None), end_ptr, end_f32, n, self.size, i, st)
            _lib.check(rc, "dgvit_ring_store_small")
            if self.episode_flags is not None and not step:
                _lib.check(lib.dgvit_ring_mark(_ptr(self.episode_flags), self.size, i, n, st), "dgvit_ring_mark")
            if self.shared_next_obs:             # the frames go last: where they go depends on done and END of the slots before
                E, P = self.num_envs, self.terminal_frames
                moves = self._step_moves if step else torch.empty(n, dtype=torch.int32, device=self.device)
                rc = lib.dgvit_ring_plan_next(_ptr(self.next_row), _ptr(self._pool_state), _ptr(moves), _ptr(self.store["done"]),
                                              self.rows["done"], _ptr(self.episode_flags), n, self.size, i, E, P, st)
                _lib.check(rc, "dgvit_ring_plan_next")
                rc = lib.dgvit_ring_store_frames_shared(p0, c0, ld0, p1, c1, ld1, _ptr(self.arena), _ptr(moves), int(u8), self.frame_ld, n,
                                                        self.fields["obs"], self.size, i, E, P, st)
                _lib.check(rc, "dgvit_ring_store_frames_shared")
        self.next_index = (i + n) % self.size
        self.stored = min(self.stored + n, self.size)
        self._on_store(i, n)

    # ---- the ring as a file
    def _leaves(self):
        """the (size,) leaves of the priority tree, a view; None: a ring without one"""
        return None

    def _priority_meta(self):
        """(alpha, eps, the two header words of the priority tree, a view) for meta.json and the check of a file; None: a ring without one"""
        return None

    def _file_spec(self, frame, leaves):
        """{array of a ring file: (numpy dtype, shape of a transition)} with frames of dtype ``frame``: ``FILE_FIELDS``, ``end`` and, with
        ``leaves``, ``priority``"""
        spec = {k: (np.dtype(frame if k in FRAME_FIELDS else np.float32), self.shapes[k]) for k in FILE_FIELDS}
        spec["end"] = (np.dtype(np.uint8), ())
        if leaves:
            spec["priority"] = (np.dtype(np.float32), ())
        return spec

    def _layout(self, n, frame_dtype=None, leaves=None):
        return export_layout(n, self.shapes["obs"], self.fields["pobs"], self.fields["act"], frame_dtype or self.frame_dtype,
                             self._leaves() is not None if leaves is None else leaves)

    def _export_chunk(self, a0: int, n: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The one dgvit_ring_export launch of a chunk: ages [a0, a0 + n) of the ring -- age a lies in slot ``(oldest + a) % size``,
        ``oldest = next_index`` when the ring is full, else 0 -- packed as ``export_layout`` says into ``out``, a uint8 device tensor
        (allocated when None), which is returned."""
        if not 0 <= a0 < a0 + n <= self.stored:
            raise ValueError(f"ages [{a0}, {a0 + n}) must be a non-empty range inside [0, stored={self.stored})")
        nbytes = self._layout(n)[1]
        if out is None:
            out = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        leaves = self._leaves()
        view = _lib.dgvit_ring_view()
        view.obs = self.store["obs"].data_ptr()
        view.next_obs = self.next_frames.data_ptr()
        view.next_row = self.next_row.data_ptr() if self.shared_next_obs else None
        for j, k in enumerate(SMALL_FIELDS):
            view.small[j], view.small_cols[j], view.small_ld[j] = self.store[k].data_ptr(), self.fields[k], self.rows[k]
        view.flags = None if self.episode_flags is None else self.episode_flags.data_ptr()
        view.leaves = None if leaves is None else leaves.data_ptr()
        view.frame_ld = self.frame_ld
        view.next_rows = self.next_frame_rows
        view.frame_u8 = int(self.frame_dtype is torch.uint8)
        oldest = self.next_index if self.stored == self.size else 0
        with torch.cuda.device(self.device):
            rc = _lib.load().dgvit_ring_export(view, _ptr(out), out.numel(), self.fields["obs"], self.size, oldest, a0, n, _stream())
        _lib.check(rc, "dgvit_ring_export")
        return out

    def _meta(self) -> dict:
        """meta.json of save_transitions; the two device reads (the pool's counters, the tree's header) synchronise"""
        u8, per = self.frame_dtype is torch.uint8, self._priority_meta()
        alpha, eps, header = (None, None, [None, None]) if per is None else (*per[:2], per[2].view(torch.int32).tolist())
        return {"format_version": FILE_FORMAT_VERSION, "stored": self.stored, "size": self.size, "num_envs": self.num_envs,
                "oldest_slot": self.next_index if self.stored == self.size else 0, "next_index": self.next_index,
                "obs_shape": list(self.shapes["obs"]), "pstate_dim": self.fields["pobs"], "act_dim": self.fields["act"],
                "frame_dtype": "uint8" if u8 else "float32", "shared_next_obs": self.shared_next_obs, "terminal_frames": self.terminal_frames,
                "lost_terminal_frames": self.lost_terminal_frames(), "episodes_tracked": self.episode_flags is not None,
                "prioritized": per is not None, "alpha": alpha, "eps": eps, "max_leaf_bits": header[0], "update_max_bits": header[1]}

    def save_transitions(self, path, *, chunk: int = 4096, overwrite: bool = False) -> None:
        """Write the stored transitions to the directory ``path`` (cpprb's name): ``meta.json`` (``META_KEYS``) and one plain
        ``.npy`` per field of ``FILE_FIELDS``, first axis = age, the oldest stored transition first -- age a lies in slot
        ``(oldest + a) % size``.  Frames are the ring's own: uint8 codes from a uint8 ring, fp32 from an fp32 ring, dense (H, W) rows
        without the ring's padding; ``next_obs`` of a shared ring is the frame ``sample`` returns for the slot.  ``end.npy`` is uint8,
        bit 0 the slot's END flag (HEAD is derived on load; zeros when episodes were never tracked), ``priority.npy`` the fp32 leaves
        ``(|p| + eps)^alpha`` of a prioritized ring, ``rng.npy`` the bytes of ``self.gen.get_state()``.  Every array file can be read with
        ``numpy.load(..., mmap_mode="r")``.

        ``chunk`` transitions at a time are packed by one dgvit_ring_export launch into one of two device buffers and leave in ONE copy to
        one of two pinned buffers on a side stream, so the copy of chunk c overlaps the host's write of chunk c - 1 into the memory-mapped
        files: host memory stays bounded by two chunks.  The host waits on events, never on the device as a whole.  The directory is
        written under a temporary name beside ``path`` and renamed at the end.  An existing ``path`` raises FileExistsError unless
        ``overwrite=True``; an empty ring raises RuntimeError; a call inside a stream capture raises DgvitError."""
        chunk = _chunk(chunk)
        if not isinstance(overwrite, (bool, np.bool_)):
            raise ValueError(f"overwrite must be a bool, got {overwrite!r}")
        path = os.path.abspath(os.fspath(path))
        if torch.cuda.is_current_stream_capturing():
            raise _lib.DgvitError("save_transitions() copies to the host and waits for it, which a stream capture cannot")
        if self.stored == 0:
            raise RuntimeError("save_transitions() on an empty buffer: there is nothing to save")
        if os.path.lexists(path) and not overwrite:
            raise FileExistsError(f"{path} exists: pass overwrite=True to replace it")
        stored, leaves = self.stored, self._leaves() is not None
        chunk = min(chunk, stored)
        tmp = f"{path}.tmp-{os.getpid()}"
        if os.path.lexists(tmp):
            shutil.rmtree(tmp)
        os.makedirs(tmp)
        try:
            spec = self._file_spec(np.uint8 if self.frame_dtype is torch.uint8 else np.float32, leaves)
            files = {k: open_memmap(os.path.join(tmp, k + ".npy"), mode="w+", dtype=dt, shape=(stored, *shape)) for k, (dt, shape) in spec.items()}
            nbytes = self._layout(chunk)[1]
            dev = [torch.empty(nbytes, dtype=torch.uint8, device=self.device) for _ in range(2)]
            pin = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            cur, side = torch.cuda.current_stream(self.device), torch.cuda.Stream(self.device)
            copied = [None, None]

            def write(a0, n, p):
                """the host's part: chunk [a0, a0 + n) out of pinned buffer p into the files, once its copy has arrived"""
                copied[p].synchronize()
                host, blocks = pin[p].numpy(), self._layout(n)[0]
                for k, (dt, shape) in spec.items():
                    off, nb = blocks[k]
                    files[k][a0:a0 + n] = host[off:off + nb].view(dt).reshape(n, *shape)

            waiting = None
            for c, a0 in enumerate(range(0, stored, chunk)):
                n, p = min(chunk, stored - a0), c & 1
                if copied[p] is not None:
                    cur.wait_event(copied[p])        # device buffer p is free once chunk c - 2 has left it
                self._export_chunk(a0, n, out=dev[p])
                exported = torch.cuda.Event()
                exported.record(cur)
                side.wait_event(exported)
                need = self._layout(n)[1]
                with torch.cuda.stream(side):        # pinned buffer p is free: the host wrote chunk c - 2 in the round before
                    pin[p][:need].copy_(dev[p][:need], non_blocking=True)
                copied[p] = torch.cuda.Event()
                copied[p].record(side)
                if waiting is not None:
                    write(*waiting)
                waiting = (a0, n, p)
            write(*waiting)
            for f in files.values():
                f.flush()
            del files
            np.save(os.path.join(tmp, "rng.npy"), self.gen.get_state().numpy())
            with open(os.path.join(tmp, "meta.json"), "w") as f:
                json.dump(self._meta(), f, indent=1)
            if os.path.lexists(path):
                shutil.rmtree(path) if os.path.isdir(path) and not os.path.islink(path) else os.remove(path)
            os.rename(tmp, path)
        except BaseException:
            shutil.rmtree(tmp, ignore_errors=True)
            raise

    def _set_leaves(self, start: int, leaves: torch.Tensor) -> None:
        """hook: ring slots start .. (mod size) have just been loaded with these leaves of a file; a ring without a tree ignores them"""

    def _restore_max_leaf(self, meta: dict) -> None:
        """hook: the last chunk of a file with priorities is in"""

    def _check_file(self, path, priorities):
        """meta.json and the memory-mapped arrays of a save_transitions directory, checked against this ring -> (meta, arrays); ``arrays``
        has ``priority`` only when the file's leaves are to be loaded.  Nothing is stored and no device is touched."""
        with open(os.path.join(path, "meta.json")) as f:
            meta = json.load(f)
        if meta.get("format_version") != FILE_FORMAT_VERSION:
            raise ValueError(f"{path}: format_version={meta.get('format_version')!r}, this package reads {FILE_FORMAT_VERSION}")
        for k in META_KEYS:
            if k not in meta:
                raise ValueError(f"{path}: meta.json has no {k}")
        mine = {"num_envs": self.num_envs, "obs_shape": list(self.shapes["obs"]), "pstate_dim": self.fields["pobs"], "act_dim": self.fields["act"]}
        for k, v in mine.items():
            if (list(meta[k]) if k == "obs_shape" else meta[k]) != v:
                raise ValueError(f"{path}: {k}={meta[k]!r} in the file, {v!r} in this ring")
        stored = meta["stored"]
        if not isinstance(stored, int) or stored < 1 or stored % self.num_envs:
            raise ValueError(f"{path}: stored={stored!r} must be a positive multiple of num_envs={self.num_envs}")
        if meta["frame_dtype"] not in ("float32", "uint8"):
            raise ValueError(f"{path}: frame_dtype={meta['frame_dtype']!r} must be 'float32' or 'uint8'")
        with_leaves = (priorities == "file" and self._leaves() is not None and bool(meta["prioritized"])
                       and os.path.exists(os.path.join(path, "priority.npy")))
        if with_leaves:
            alpha, eps, _ = self._priority_meta()
            if (meta["alpha"], meta["eps"]) != (alpha, eps):
                raise ValueError(f"{path}: the leaves are (|p| + eps)^alpha with alpha={meta['alpha']!r} eps={meta['eps']!r}, this ring has "
                                 f"alpha={alpha!r} eps={eps!r}: pass priorities='reset'")
        arrays = {}
        for k, (dt, shape) in self._file_spec(meta["frame_dtype"], with_leaves).items():
            a = np.load(os.path.join(path, k + ".npy"), mmap_mode="r", allow_pickle=False)
            if a.dtype != dt or a.shape != (stored, *shape):
                raise ValueError(f"{path}: {k}.npy is {a.dtype} {a.shape}, expected {dt} {(stored, *shape)}")
            arrays[k] = a
        return meta, arrays

    def load_transitions(self, path, *, priorities: str = "file", restore_rng: Optional[bool] = None) -> int:
        """Store the transitions of a ``save_transitions`` directory, oldest first, through the ring's own store path (``_commit``) -> how
        many were stored.  What is stored, the flags, a shared ring's bookkeeping and the refusals are therefore ``add_batch``'s and
        ``add_vec``'s.  ``LOAD_CHUNK`` transitions at a time are packed into a pinned buffer, go to the device in ONE copy, and are handed
        to ``_commit`` as device views of that chunk.  The episode structure is replayed: a ring with ``num_envs = E > 1`` takes one
        ``_commit`` per vector step with the step's END bits as its ``episode_end``; a ring with E = 1 one ``_commit`` per run of slots up
        to and including an END, followed by ``on_episode_end()``; a file without tracked episodes one ``_commit`` per chunk (per step where
        a ring of several lanes tracks episodes itself, so that its marks are a step's).

        The file's ``num_envs``, ``obs_shape``, ``pstate_dim`` and ``act_dim`` must be the ring's (ValueError naming the key, before
        anything is stored); ``size``, ``frame_dtype``, ``shared_next_obs`` and ``terminal_frames`` may differ.  A uint8 file into an fp32
        ring stores the correctly rounded ``codes.float() / 255``, the bits ``sample`` returns from a uint8 ring, formed on the device
        by a lookup in the table of the 256 quotients; an fp32 file into a uint8 ring is quantised by the store path.  A ring
        smaller than the file ends with the newest transitions.  When the ring is empty and the file's ``size`` and ``num_envs`` are the
        ring's -- a *same-geometry* load -- ``next_index`` first moves to the file's ``oldest_slot``, so every transition returns to the
        slot it had and ``next_index`` and ``stored`` end as they were.  ``restore_rng=None`` restores ``self.gen`` from ``rng.npy``
        exactly then (True / False force it): the resumed run then draws the indices the saved run would have drawn.

        On a prioritized ring each ``_commit`` leaves the max leaf in its slots; with ``priorities="file"`` the file's leaves are then
        written over them (dgvit_per_set_leaves) and the max leaf is restored after the last chunk -- ``alpha`` and ``eps`` must equal
        the file's, else ValueError.  ``priorities="reset"``, or a file without ``priority.npy``, leaves every slot at the max leaf."""
        priorities, restore_rng = _load_options(priorities, restore_rng)
        path = os.path.abspath(os.fspath(path))
        if torch.cuda.is_current_stream_capturing():
            raise _lib.DgvitError("load_transitions() reads files and stages them through the host, which a stream capture cannot")
        meta, arrays = self._check_file(path, priorities)
        rng = np.load(os.path.join(path, "rng.npy"), allow_pickle=False)
        stored, E, leaves = meta["stored"], self.num_envs, "priority" in arrays
        same = self.stored == 0 and meta["size"] == self.size and meta["num_envs"] == E
        if same:
            self.next_index = int(meta["oldest_slot"])
        tracked = bool(meta["episodes_tracked"])
        if tracked:
            self.track_episodes()
        if self.stored and self.episode_flags is not None:      # what is there does not go on into the file: its episodes end here
            self.on_episode_end(None if E == 1 else torch.ones(E, dtype=torch.bool, device=self.device))
        by_step = E > 1 and self.episode_flags is not None
        file_dtype = torch.uint8 if meta["frame_dtype"] == "uint8" else torch.float32
        chunk = min(max(LOAD_CHUNK // E, 1) * E, self.size, stored)       # a multiple of E (E divides size and stored)
        nbytes = self._layout(chunk, file_dtype, leaves)[1]
        pin = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        arrived = [None, None]
        cur = torch.cuda.current_stream(self.device)
        if file_dtype is torch.uint8 and self.frame_dtype is torch.float32:
            # fl(k / 255), the 256 values a uint8 ring's gather returns: looked up on the device, because a device division by a
            # scalar is a multiplication by fl(1 / 255), which differs from the quotient in 126 of the 256 codes (replay_ring.hip)
            table = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255.0)).to(self.device)
        for c, a0 in enumerate(range(0, stored, chunk)):
            n, p = min(chunk, stored - a0), c & 1
            blocks, need = self._layout(n, file_dtype, leaves)
            if arrived[p] is not None:
                arrived[p].synchronize()             # pinned buffer p has been read: chunk c - 2 is on the device
            host = pin[p].numpy()
            for k, (off, nb) in blocks.items():
                host[off:off + nb].view(arrays[k].dtype).reshape(arrays[k][a0:a0 + n].shape)[...] = arrays[k][a0:a0 + n]
            dev[:need].copy_(pin[p][:need], non_blocking=True)      # behind the launches that read chunk c - 1 out of `dev`
            arrived[p] = torch.cuda.Event()
            arrived[p].record(cur)
            views = {}
            for k in FILE_FIELDS:
                off, nb = blocks[k]
                v = dev[off:off + nb]
                if k in FRAME_FIELDS and file_dtype is torch.uint8:
                    v = v.view(n, -1)
                    views[k] = v if self.frame_dtype is torch.uint8 else table.index_select(0, v.reshape(-1).int()).view(n, -1)
                else:
                    views[k] = v.view(torch.float32).view(n, -1)
            ends = dev[blocks["end"][0]:blocks["end"][0] + n]
            prio = dev[blocks["priority"][0]:blocks["priority"][0] + 4 * n].view(torch.float32) if leaves else None

            def commit(lo, hi, end=None):
                start = self.next_index
                self._commit({k: v[lo:hi] for k, v in views.items()}, hi - lo, end)
                if leaves:
                    self._set_leaves(start, prio[lo:hi])

            if by_step:
                for lo in range(0, n, E):
                    commit(lo, lo + E, ends[lo:lo + E])
            elif tracked and E == 1:
                lo = 0
                for e in np.flatnonzero(np.asarray(arrays["end"][a0:a0 + n]) & FLAG_END).tolist():
                    commit(lo, e + 1)
                    self.on_episode_end()
                    lo = e + 1
                if lo < n:
                    commit(lo, n)
            else:
                commit(0, n)
        for ev in arrived:
            if ev is not None:
                ev.synchronize()                     # the pinned buffers go out of scope
        if leaves:
            self._restore_max_leaf(meta)
        if same if restore_rng is None else restore_rng:
            self.gen.set_state(torch.from_numpy(rng))
        return stored

    def clear(self) -> None:
        """Empty the ring without reallocating (cpprb's name): ``next_index`` and ``stored`` to 0, the episode flags to zeros (they stay
        allocated), a shared ring's ``next_row`` to -1 and its pool's counters to 0; the frame matrices are not touched."""
        self.next_index = self.stored = 0
        if self.episode_flags is not None:
            self.episode_flags.zero_()
        if self.shared_next_obs:
            self.next_row.fill_(-1)
            self._pool_state.zero_()

    def _add(self, kw, n) -> None:
        """add / add_batch: of n > size transitions the last ``size`` are the ones that stay"""
        if self.num_envs > 1:
            raise _lib.DgvitError(f"add() / add_batch() write consecutive slots of one episode, and this ring has num_envs={self.num_envs} "
                                  "lanes: store a step of all environments with add_vec()")
        for k in self.fields:
            if k not in kw:
                raise KeyError(f"missing field {k}")
        self._commit({k: self._travel(k, kw[k], n)[-self.size:] for k in self.fields}, min(n, self.size))

    def add(self, **kw) -> None:
        """One transition (numpy arrays / scalars / tensors), same keywords as replay_buffer.add in DRL.py:439-448: one staged
        host->device copy for the host fields of the whole transition and two launches (``_commit``)."""
        self._add(kw, 1)

    def add_batch(self, **kw) -> None:
        """Many transitions at once (first axis = transitions), e.g. the expert demonstrations of DRL.py:469-478: assembled on
        the host with numpy slicing, one host->device copy, two launches and a third for the marks when episodes are tracked."""
        self._add(kw, len(kw["obs"]))

    def _vec_field(self, k, v):
        """Field k of one vector step, checked -> the (E, cnt) device tensor where it lies (fp32, or the uint8 codes of a frame of a uint8
        ring; made contiguous on the device), or the (E, cnt) host array, float32 or uint8 codes, that will travel in the staged matrix."""
        E, cnt = self.num_envs, self.fields[k]
        codes_ok = self.frame_dtype is torch.uint8 and k in FRAME_FIELDS
        on_device = torch.is_tensor(v) and v.device.type != "cpu"
        if on_device:
            home = self.store["obs"].device      # every field's: a shared ring has no store["next_obs"]
            if v.device != home:
                raise ValueError(f"{k}: the tensor is on {v.device}, the ring on {home}")
            v = v.detach()
            codes = v.dtype == torch.uint8
            if not codes and v.dtype != torch.float32:
                raise ValueError(f"{k}: a device tensor must be float32{' or uint8' if codes_ok else ''}, got {v.dtype}")
        else:
            v = np.asarray(v.detach().numpy() if torch.is_tensor(v) else v)
            codes = v.dtype == np.uint8 and k in FRAME_FIELDS
        if codes and not codes_ok:
            raise ValueError(f"{k}: uint8 codes can only be stored in the frame fields of a frame_dtype=torch.uint8 ring")
        shape = tuple(v.shape)
        if len(shape) == 0 or shape[0] != E or int(np.prod(shape)) != E * cnt:
            raise ValueError(f"{k}: expected first axis num_envs={E} and {cnt} values per environment, got shape {shape}")
        if on_device:
            return v.reshape(E, cnt).contiguous()
        return np.ascontiguousarray(v.reshape(E, cnt), dtype=np.uint8 if codes else np.float32)

    def add_vec(self, *, obs, pobs, act, rew, next_obs, next_pobs, done, episode_end=None) -> None:
        """One step of all ``num_envs`` environments: every field has first axis E, environment e goes to slot
        ``next_index + e``; ``rew`` and ``done`` may be (E,) or (E, 1).  A field may be a tensor on the buffer's device -- fp32, or uint8
        codes for the frame fields of a uint8 ring; it is read where it lies -- or a host array, CPU tensor or list; all host fields of a
        call travel in ONE pinned staging matrix and one host->device copy, and the same kernels read them from there.  Per field, freely
        mixed.  A wrong dtype, device or shape raises ValueError naming the field.

        ``episode_end`` -- None, a host bool array-like (E,), or a device tensor (E,) of bool, uint8 or fp32, nonzero = end -- says that
        environment e's transition of this step is the last of its episode, whatever its ``done`` says: ``on_episode_end()``'s meaning.
        Passing it starts ``track_episodes()`` if nothing has, so the first such call must happen outside a capture.

        Two launches (``_commit``): dgvit_ring_store_frames for ``obs`` and ``next_obs``, dgvit_ring_store_small for the other five fields
        and, when episodes are tracked, the marks (the new slots get HEAD, and END where ``episode_end`` says so; the previous step's slots
        keep only their END); the prioritized subclass adds its dgvit_per_set_range.  With every field and ``episode_end`` on the device nothing
        synchronises with the host and nothing pinned is allocated.  ``num_envs == 1`` is allowed: the device-side ``add``."""
        E, kw = self.num_envs, dict(obs=obs, pobs=pobs, act=act, rew=rew, next_obs=next_obs, next_pobs=next_pobs, done=done)
        rows = {k: self._vec_field(k, kw[k]) for k in self.fields}
        end = episode_end
        if end is not None:
            if torch.is_tensor(end) and end.device.type != "cpu":
                if end.device != self.store["obs"].device or end.dtype not in (torch.bool, torch.uint8, torch.float32) or end.numel() != E:
                    raise ValueError(f"episode_end: a device tensor must be ({E},) bool, uint8 or float32 on {self.store['obs'].device}, got "
                                     f"{tuple(end.shape)} {end.dtype} on {end.device}")
                end = end.detach().reshape(E).contiguous()
            else:
                end = np.asarray(end.detach().numpy() if torch.is_tensor(end) else end).reshape(-1)
                if end.size != E:
                    raise ValueError(f"episode_end: expected {E} entries, got {end.size}")
                end = (end != 0).astype(np.float32)
            self.track_episodes()
        self._commit(rows, E, end)

    def sample_indices(self, batch_size: int) -> torch.Tensor:
        if self.stored == 0:
            raise RuntimeError("cannot sample from an empty buffer")
        return torch.randint(0, self.stored, (batch_size,), device=self.device, dtype=torch.int64, generator=self.gen)

    def sample(self, batch_size: int, indices: Optional[torch.Tensor] = None, random_shift: int = 0,
               return_shifts: bool = False, n_step: Optional[int] = None, gamma: float = 0.99,
               frame_stack: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Uniform sample with replacement -> dict of DEVICE tensors shaped like the reference's batch
        (obs (B,H,W), pobs (B,2), act (B,2), rew (B,1), ...), ready for the networks: no host round trip.

        ``random_shift=p`` (p > 0) applies the DrQ augmentation inside the gather of ``obs`` and ``next_obs``: each sampled frame is
        padded by p pixels with its border and cropped back at its own random offset, the two fields drawing independently (streams
        0 and 1 of one seed per call; the seed comes from torch's CPU generator, or from the device inside a stream capture, and is
        kept in ``self.shift_seed``).  ``return_shifts=True`` adds ``obs_shift`` and ``next_obs_shift``, (B, 2) int32 (dy, dx).
        With ``random_shift=0`` nothing is drawn and the launches are the plain gathers.  A uint8 ring (``frame_dtype``) takes the
        ``_u8`` forms of the two frame launches and returns the same fp32 frames, code / 255.

        ``n_step=n`` (an int in [1, 64]; ``gamma`` in [0, 1]) returns n-step transitions, cpprb's ``Nstep``: from the sampled slot the
        walk follows the ring for m <= n slots and stops behind the first one with ``done != 0`` or an episode flag (END or HEAD).
        ``rew`` is then sum_{k<m} gamma^k rew_k (summed in double, rounded once), ``next_obs``, ``next_pobs`` and ``done`` are those of
        the walk's last slot, and the dict gains ``discount`` (B, 1) fp32 = gamma^m -- what ``sac_losses.critic_loss(discount=...)``
        takes in the place of gamma -- and ``steps`` (B,) int32 = m.  ``indexes`` stays the start slot, which is what
        ``update_priorities`` must get.  Five launches instead of seven: the ``obs``, ``pobs`` and ``act`` gathers, the walk (which
        produces ``rew``, ``done`` and ``next_pobs`` itself) and the ``next_obs`` gather at the walk's last slot.  Outside a capture
        the call starts ``track_episodes()`` if nothing has; inside one the flags must exist already, and a replayed graph follows
        the ring as later ``add()``s move it.  ``n_step=None`` is the one-step path above, launch for launch.  On a ring with
        ``num_envs=E > 1`` the walk follows the slot's own environment, ``(i + k E) % size``, and nothing else changes: ``indexes`` are
        slots, ``indexes % num_envs`` their environments.

        On a ``shared_next_obs=True`` ring ``next_obs`` comes out of the arena with the same gather, at the rows ``next_row`` names for
        the sampled slots (the walk's last ones for ``n_step``): one small launch more, dgvit_ring_next_rows, and nothing else changes --
        a replayed graph follows later ``add()``s because the table lives on the device.

        ``frame_stack=K`` (an int in [1, 16]) returns ``obs`` and ``next_obs`` as ``(B, H, W, K)`` fp32, contiguous and
        channel-last, channel K - 1 the newest frame: the sampled slot's frame and the K - 1 frames before it in ITS episode and lane,
        found by the n-step walk run backward -- predecessor ``(s - k E) % size`` counts while its flags and ``done`` are zero and, in a
        ring that is not full yet, while it does not lie before slot 0.  Frames from before the episode's first stored slot repeat that
        first frame, as Gym's ``FrameStack`` does at reset.  The ``next_obs`` stack is the ``obs`` stack moved on by one: channel K - 1
        is the transition's ``next_obs`` (the n-step tail's with ``n_step``, from whose slot the walk back then starts), the channels
        below are ``obs`` frames.  ``K = 1`` equals the plain sample's ``unsqueeze(-1)``; every other key is unchanged.  ``random_shift``
        draws ONE (dy, dx) per sample and field for all K channels, the very draw of the unstacked call: equal seeds give equal
        ``obs_shift`` / ``next_obs_shift``.  Three launches in the place of the two frame gathers: dgvit_ring_stack_rows, which names
        every sample's 2 K rows, and one dgvit_gather_stack_frames (``_shift_`` with ``random_shift``) per field; the uint8 ring,
        ``num_envs``, ``shared_next_obs``, prioritization, ``n_step`` and capture compose.  Like ``n_step`` the eager call starts
        ``track_episodes()``, and inside a capture the flags must exist.  A replayed graph follows later ``add()``s through the flags
        and ``next_row``, but "the ring is full" is passed by value and frozen: a graph captured before the ring first fills keeps
        treating the seam between slot ``size - 1`` and slot 0 as an episode start (conservative: it never reads an unwritten slot) --
        re-capture once the ring has filled, and re-capture a full ring's graph after ``clear()``.  Known limit: the oldest slot of a
        full ring has the HEAD slot before it, so its stack repeats its own frame although its episode may be older; those frames are
        gone.  ``frame_stack=None`` is the path above, launch for launch."""
        n_step, gamma, K = _n_step(n_step), _unit("gamma", gamma), _frame_stack(frame_stack)
        pad = _shift_pad(random_shift, self.shapes["obs"], "random_shift")
        # the slots are the batch's ``indexes`` from the start: a given contiguous int64 tensor on the ring's device is adopted, not copied
        idx = self.sample_indices(batch_size) if indices is None else indices.to(self.device, torch.int64).contiguous()
        batch = _Rows(idx.numel(), self.device)
        batch.bufs["indexes"] = idx
        self._sample_rows(batch, idx, pad, return_shifts, n_step, gamma, K)
        return _finish(batch, self.fields, self.shapes, pad, return_shifts, n_step, K)

    def _slots_of_mixed(self, batch, n, indices):
        """this ring's n rows of a ``sample_mixed`` batch's ``indexes``, filled: the draw ``sample_indices`` makes, written there by the
        draw itself, or the given ``indices`` copied there"""
        idx = batch.empty("indexes", n, (), torch.int64)
        if indices is None:
            return torch.randint(0, self.stored, (n,), generator=self.gen, out=idx)
        return idx.copy_(indices.to(self.device, torch.int64).reshape(-1))

    def _sample_rows(self, batch, idx, pad, return_shifts, n_step, gamma, K):
        """The one sampling path of ``sample``, the prioritized ``sample`` and ``sample_mixed``: this ring's launches of a call at the
        slots ``idx`` -- its rows of the batch's ``indexes``, already drawn or given -- written into the same rows of ``batch``
        (``_Rows``); the keywords have passed their checks, and nothing is shaped here (``_finish``).  The launches stand in the order
        they depend on each other."""
        if n_step is not None or K is not None:
            self.track_episodes()
        lib, st, dev, u8, n = _lib.load(), _stream(), self.device, self.frame_dtype is torch.uint8, idx.numel()
        if pad:
            self.shift_seed = _shift_seed(dev)
        shifts = _NO_SHIFTS
        if pad and return_shifts:
            shifts = {k: batch.empty(k + "_shift", n, (2,), torch.int32) for k in FRAME_FIELDS}
        with torch.cuda.device(dev):
            tail = None                          # 1. the walk: rew, done, next_pobs, discount and steps, and the slots where it ended
            if n_step is not None:
                tail = self._walk(batch, idx, n, n_step, gamma)
            if K is not None:                    # 2. the stacks' row tables, from the walk's tails on, and 4. the stacks
                rows = self._stack_rows(idx, tail, K)
                for k in FRAME_FIELDS:
                    self._gather_stack(k, rows[k], K, pad, shifts[k], batch.empty(k, n, (_al4(self.fields[k] * K),), torch.float32))
            else:
                last = idx if tail is None else tail
                if self.shared_next_obs:         # 3. next_obs lies in the arena, at the rows next_row names
                    slots, last = last, torch.empty(n, dtype=torch.int64, device=dev)
                    _lib.check(lib.dgvit_ring_next_rows(_ptr(self.next_row), _ptr(slots), _ptr(last), n, self.size, st), "dgvit_ring_next_rows")
                # 4. the two frame outputs: obs at the slots, next_obs at the walk's last slots or at the arena rows just looked up
                for k, src, nrows, at in (("obs", self.store["obs"], self.size, idx), ("next_obs", self.next_frames, self.next_frame_rows, last)):
                    buf = batch.empty(k, n, (self.rows[k],), torch.float32)
                    if pad:
                        _gather_shift(src, at, buf, shifts[k], self.shapes[k], nrows, pad, int(k == "next_obs"), self.shift_seed)
                    elif u8:
                        rc = lib.dgvit_gather_rows_u8(_ptr(src), _ptr(at), _ptr(buf), n, self.fields[k], self.frame_ld, self.rows[k], nrows, st)
                        _lib.check(rc, "dgvit_gather_rows_u8")
                    else:
                        _lib.check(lib.dgvit_gather_rows(_ptr(src), _ptr(at), _ptr(buf), n, self.rows[k], nrows, st), "dgvit_gather_rows")
            for k in SMALL_FIELDS if n_step is None else ("pobs", "act"):     # 5. the small fields the walk has not produced
                buf = batch.empty(k, n, (self.rows[k],), torch.float32)
                _lib.check(lib.dgvit_gather_rows(_ptr(self.store[k]), _ptr(idx), _ptr(buf), n, self.rows[k], self.size, st), "dgvit_gather_rows")

    def _stack_rows(self, idx, tail, K):
        """the one dgvit_ring_stack_rows launch of a stacked sample: {field: (B, K) int64 rows of its K frames}; ``tail`` the n-step
        walk's last slots or None"""
        B = idx.numel()
        rows = {k: torch.empty(B, K, dtype=torch.int64, device=self.device) for k in FRAME_FIELDS}
        rc = _lib.load().dgvit_ring_stack_rows(_ptr(idx), _ptr(tail), _ptr(self.episode_flags), _ptr(self.store["done"]), self.rows["done"],
                                               _ptr(self.next_row if self.shared_next_obs else None), _ptr(rows["obs"]), _ptr(rows["next_obs"]),
                                               B, self.size, self.num_envs, K, int(self.stored == self.size), self.next_frame_rows, _stream())
        _lib.check(rc, "dgvit_ring_stack_rows")
        return rows

    def _gather_stack(self, k, rows, K, pad, shifts, buf):
        """frame field k of a stacked sample into ``buf``, (B, al4(H W K)): dgvit_gather_stack_frames, or its shifted form, over the obs
        matrix and -- for the newest channel of next_obs -- the matrix ``next_obs`` is gathered from"""
        B, cols, (H, W), row = rows.shape[0], self.fields[k], self.shapes[k], buf.shape[1]
        u8, src0 = int(self.frame_dtype is torch.uint8), self.store["obs"]
        src1, nrows1 = (src0, self.size) if k == "obs" else (self.next_frames, self.next_frame_rows)
        lib = _lib.load()
        if pad:
            seed_val, seed_dev = _seed_args(self.shift_seed)
            rc = lib.dgvit_gather_shift_stack_frames(_ptr(src0), _ptr(src1), _ptr(rows), _ptr(buf), _ptr(shifts), B, H, W, K, u8, self.frame_ld,
                                                     row, self.size, nrows1, pad, int(k == "next_obs"), seed_val, _ptr(seed_dev), _stream())
            _lib.check(rc, "dgvit_gather_shift_stack_frames")
        else:
            rc = lib.dgvit_gather_stack_frames(_ptr(src0), _ptr(src1), _ptr(rows), _ptr(buf), B, cols, K, u8, self.frame_ld, row, self.size,
                                               nrows1, _stream())
            _lib.check(rc, "dgvit_gather_stack_frames")

    def _walk(self, batch, idx, B, n_step, gamma):
        """the one dgvit_nstep_walk launch of an n-step sample (dgvit_nstep_walk_strided on a ring of several environments): rew, done,
        next_pobs, discount and steps into the batch -> the (B,) int64 slots where the walks ended"""
        f32 = lambda name, *tail: batch.empty(name, B, tail, torch.float32)   # noqa: E731
        ret, done, disc, small = f32("rew"), f32("done"), f32("discount"), f32("next_pobs", self.rows["next_pobs"])
        steps, tail = batch.empty("steps", B, (), torch.int32), torch.empty(B, dtype=torch.int64, device=self.device)
        ring = (_ptr(self.store["rew"]), self.rows["rew"], _ptr(self.store["done"]), self.rows["done"], _ptr(self.episode_flags),
                _ptr(self.store["next_pobs"]), self.rows["next_pobs"], _ptr(idx), B, self.size)
        outs = (n_step, gamma, _ptr(ret), _ptr(done), _ptr(disc), _ptr(small), _ptr(steps), _ptr(tail), _stream())
        if self.num_envs == 1:
            _lib.check(_lib.load().dgvit_nstep_walk(*ring, *outs), "dgvit_nstep_walk")
        else:                                    # an environment's next transition is num_envs slots on
            _lib.check(_lib.load().dgvit_nstep_walk_strided(*ring, self.num_envs, *outs), "dgvit_nstep_walk_strided")
        return tail


PER_MAX_SIZE = 1 << 24      # include/dgvit_hip.h: the radix-64 tree has at most four levels


def _unit(name: str, v) -> float:
    """a real number in [0, 1] (bools and everything else: ValueError)"""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= 1.0:
        raise ValueError(f"{name} must be a number in [0, 1], got {v!r}")
    return float(v)


def per_tree_layout(capacity: int):
    """[(offset of the sums, padded length)] per level and the floats of the whole tree, as dgvit_per_tree_floats lays it out: a 64-float
    header, then for each level pad64(n_l) sums and pad64(n_l) mins; n_0 = capacity, n_l = ceil(n_{l-1} / 64), last level n_l <= 64."""
    if not 1 <= capacity <= PER_MAX_SIZE:
        raise ValueError(f"size must be in [1, 2^24], got {capacity}")
    levels, off, n = [], 64, int(capacity)
    while True:
        pad = (n + 63) // 64 * 64
        levels.append((off, pad))
        off += 2 * pad
        if n <= 64:
            return levels, off
        n = (n + 63) // 64


class PrioritizedDeviceReplayBuffer(DeviceReplayBuffer):
    """``DeviceReplayBuffer`` with proportional prioritization (Schaul et al. 2016) kept on the device: a radix-64 sum / min tree over the
    ring's slots in one fp32 tensor (``self.tree``; layout and draw in include/dgvit_hip.h).  A stored transition gets the
    largest priority seen so far, ``sample`` draws slot i with probability leaf_i / total, leaf_i = (|priority_i| + eps)^alpha, and adds
    the importance weights (p_min / leaf_i)^beta -- cpprb's (N P(i))^-beta normalised by its maximum.  Nothing synchronises with the host,
    so the draw, the gathers and the write-back are capturable in one graph.  What a SAC critic needs::

        w = batch["weights"]
        critic_loss = (w * (q - y) ** 2).mean()
        buf.update_priorities(batch["indexes"], (q - y).abs().detach())

    ``sac_losses.critic_loss(weights=batch["weights"], done=batch["done"], ...)`` is that loss in one launch, and its ``.td`` the write-back.
    ``save_transitions`` writes the leaves as ``priority.npy`` and ``load_transitions`` puts them back; rank-based
    prioritization is not implemented."""

    def __init__(self, size: int, obs_shape: Tuple[int, int] = (128, 160), pstate_dim: int = 2, act_dim: int = 2, device="cuda",
                 seed: Optional[int] = None, alpha: float = 0.6, eps: float = 1e-4, *, frame_dtype=torch.float32, num_envs=1,
                 shared_next_obs=False, terminal_frames=None):
        _frame_dtype(frame_dtype)
        _shared_next(shared_next_obs, terminal_frames, int(size), _num_envs(num_envs, size))
        self.alpha = _unit("alpha", alpha)
        if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not 0.0 <= float(eps) < float("inf"):
            raise ValueError(f"eps must be a finite number >= 0, got {eps!r}")
        self.eps = float(eps)
        self._levels, floats = per_tree_layout(int(size))
        super().__init__(size, obs_shape, pstate_dim, act_dim, device, seed, frame_dtype=frame_dtype, num_envs=num_envs,
                         shared_next_obs=shared_next_obs, terminal_frames=terminal_frames)
        lib = _lib.load()
        if lib.dgvit_per_tree_floats(self.size) != floats:
            raise _lib.DgvitError("dgvit_per_tree_floats disagrees with replay.per_tree_layout; rebuild the library")
        self.tree = torch.empty(floats, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(lib.dgvit_per_init(_ptr(self.tree), self.size, _stream()), "dgvit_per_init")

    def _on_store(self, i: int, n: int) -> None:
        """the max priority for ring slots i .. i + n - 1 (mod size), an overwritten slot forgetting its old one: the base's one store
        path ends here"""
        first = min(n, self.size - i)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            for start, count in ((i, first), (0, n - first)):
                if count > 0:
                    _lib.check(lib.dgvit_per_set_range(_ptr(self.tree), self.size, start, count, _stream()), "dgvit_per_set_range")

    def _leaves(self):
        off = self._levels[0][0]
        return self.tree[off:off + self.size]

    def _priority_meta(self):
        return self.alpha, self.eps, self.tree[:2]

    def _set_leaves(self, start: int, leaves: torch.Tensor) -> None:
        """the file's leaves over the max leaf that ``_on_store`` has just given ring slots start .. start + n - 1 (mod size):
        dgvit_per_set_leaves, twice when the slots wrap"""
        n = leaves.numel()
        first = min(n, self.size - start)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            for slot, lo, count in ((start, 0, first), (0, first, n - first)):
                if count > 0:
                    rc = lib.dgvit_per_set_leaves(_ptr(self.tree), self.size, slot, count, leaves[lo:].data_ptr(), _stream())
                    _lib.check(rc, "dgvit_per_set_leaves")

    def _restore_max_leaf(self, meta: dict) -> None:
        """The tree's header after a load, two words written on the device: the max leaf (word 0) is the larger of the ring's and the
        file's -- it never falls -- and word 1, the scratch of the last update, the file's, so that a tree loaded into a fresh ring is
        the saved one bit for bit."""
        header = torch.tensor([meta["max_leaf_bits"], meta["update_max_bits"]], dtype=torch.int32).view(torch.float32).to(self.device)
        self.tree[0:1] = torch.maximum(self.tree[0:1], header[0:1])
        self.tree[1:2] = header[1:2]

    def clear(self) -> None:
        """the base's ``clear`` and the tree as a new buffer's: dgvit_per_init"""
        super().clear()
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().dgvit_per_init(_ptr(self.tree), self.size, _stream()), "dgvit_per_init")

    def draw(self, batch_size: int, beta: float = 0.4, stratified: bool = False,
             uniforms: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The index draw alone: ((B,) int64 indices, (B, 1) fp32 importance weights).  ``uniforms`` ((B,) fp32 on the device, values in
        [0, 1]) makes the draw reproducible; absent, it comes from ``self.gen``.  ``stratified`` draws sample j from the j-th of B equal
        slices of the total priority."""
        beta = _unit("beta", beta)
        return self._draw(_Rows(int(batch_size), self.device), int(batch_size), beta, stratified, uniforms)

    def _draw(self, batch, B, beta, stratified, uniforms):
        """``draw`` into this ring's B rows of the batch's ``indexes`` and ``weights``, which are returned; ``beta`` has passed its check"""
        if self.stored == 0:
            raise RuntimeError("cannot sample from an empty buffer")
        if uniforms is None:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.DgvitError("sample() inside a stream capture needs uniforms=: pass a persistent (B,) fp32 device tensor and refill "
                                      "it inside the capture (tensor.uniform_() there uses torch's graph-safe default generator)")
            uniforms = torch.rand(B, dtype=torch.float32, device=self.device, generator=self.gen)
        elif (not torch.is_tensor(uniforms) or uniforms.dtype != torch.float32 or uniforms.device != self.store["obs"].device
              or uniforms.numel() != B or not uniforms.is_contiguous()):
            raise ValueError(f"uniforms must be a contiguous fp32 tensor of {B} values on {self.store['obs'].device}")
        idx, weights = batch.empty("indexes", B, (), torch.int64), batch.empty("weights", B, (1,), torch.float32)
        with torch.cuda.device(self.device):
            rc = _lib.load().dgvit_per_sample(_ptr(self.tree), self.size, _ptr(uniforms), B, int(bool(stratified)), beta, _ptr(idx),
                                              _ptr(weights), _stream())
        _lib.check(rc, "dgvit_per_sample")
        return idx, weights

    def sample(self, batch_size: int, beta: float = 0.4, stratified: bool = False, uniforms: Optional[torch.Tensor] = None,
               random_shift: int = 0, return_shifts: bool = False, n_step: Optional[int] = None, gamma: float = 0.99,
               frame_stack: Optional[int] = None) -> Dict[str, torch.Tensor]:
        """Prioritized sample with replacement: ``draw`` into the batch and then the base class's launches at the drawn indices
        (``random_shift``, ``return_shifts``, ``n_step``, ``gamma`` and ``frame_stack`` as there; the draw and the weights do not depend on
        them).  The base's dict plus ``weights`` (B, 1) fp32; ``indexes`` is the drawn tensor, the start slots of an n-step sample."""
        n_step, gamma, K, beta = _n_step(n_step), _unit("gamma", gamma), _frame_stack(frame_stack), _unit("beta", beta)
        batch = _Rows(int(batch_size), self.device)
        idx, _ = self._draw(batch, batch.total, beta, stratified, uniforms)
        pad = _shift_pad(random_shift, self.shapes["obs"], "random_shift")     # (after the draw, as ever: an empty ring is reported first)
        self._sample_rows(batch, idx, pad, return_shifts, n_step, gamma, K)
        return _finish(batch, self.fields, self.shapes, pad, return_shifts, n_step, K)

    def update_priorities(self, indexes: torch.Tensor, priorities: torch.Tensor) -> None:
        """leaf[indexes[j]] <- (|priorities[j]| + eps)^alpha: ``indexes`` any integer tensor of B entries, ``priorities`` (B,) or (B, 1)
        fp32 on the device, typically ``|TD error|.detach()``.  Indices outside [0, stored) are ignored, a repeated index keeps the
        largest of its new values, a non-finite priority takes the max priority."""
        if not torch.is_tensor(indexes) or indexes.dtype.is_floating_point or indexes.dtype.is_complex or indexes.dtype == torch.bool:
            raise ValueError("indexes must be an integer tensor")
        if not torch.is_tensor(priorities) or priorities.dtype != torch.float32 or priorities.device != self.store["obs"].device:
            raise ValueError(f"priorities must be an fp32 tensor on {self.store['obs'].device}")
        idx = indexes.to(self.device, torch.int64).reshape(-1).contiguous()
        prio = priorities.detach().reshape(-1).contiguous()
        if prio.numel() != idx.numel() or priorities.dim() > 2 or (priorities.dim() == 2 and priorities.shape[1] != 1) or idx.numel() == 0:
            raise ValueError(f"priorities must be (B,) or (B, 1) with B = {idx.numel()} >= 1 entries, got {tuple(priorities.shape)}")
        with torch.cuda.device(self.device):
            rc = _lib.load().dgvit_per_update(_ptr(self.tree), self.size, self.stored, _ptr(idx), _ptr(prio), idx.numel(), self.alpha,
                                              self.eps, _stream())
        _lib.check(rc, "dgvit_per_update")

    def priorities(self) -> torch.Tensor:
        """the (stored,) fp32 leaf values (|priority| + eps)^alpha, a copy"""
        off = self._levels[0][0]
        return self.tree[off:off + self.stored].clone()

    @property
    def total_priority(self) -> torch.Tensor:
        """the sum of all leaves (0-d device tensor): the top block's sums added up"""
        off = self._levels[-1][0]
        return self.tree[off:off + 64].sum()

    @property
    def min_priority(self) -> torch.Tensor:
        """the smallest stored leaf (0-d device tensor; +inf while empty): the p_min of the importance weights"""
        off, pad = self._levels[-1]
        return self.tree[off + pad:off + pad + 64].min()

    @property
    def max_priority(self) -> torch.Tensor:
        """the largest leaf ever written (0-d device tensor; 1 at first, never falls): what a newly stored transition gets"""
        return self.tree[0].clone()


# ---- one batch from several rings
MIXED_MAX_RINGS = 4


class MixedBatch(dict):
    """``sample_mixed``'s result: ``sample()``'s dict with ``source`` and ``counts``; ``rings`` are the rings of the call, in list order,
    which is how ``update_priorities_mixed`` finds them"""
    rings = ()


def _mixed_pairs(pairs):
    """``pairs`` of sample_mixed after its checks -> [(ring, n)]: host-only, runs before anything is launched"""
    if not isinstance(pairs, (list, tuple)) or not 1 <= len(pairs) <= MIXED_MAX_RINGS:
        raise ValueError(f"sample_mixed: pairs must be a list of 1 to {MIXED_MAX_RINGS} (ring, n) pairs, got {pairs!r}")
    out = []
    for i, p in enumerate(pairs):
        if not isinstance(p, (list, tuple)) or len(p) != 2:
            raise ValueError(f"sample_mixed: pairs[{i}] must be (ring, n), got {p!r}")
        ring, n = p
        if not isinstance(ring, DeviceReplayBuffer):
            raise ValueError(f"sample_mixed: pairs[{i}][0] must be a DeviceReplayBuffer, got {type(ring).__name__}")
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 0:
            raise ValueError(f"sample_mixed: pairs[{i}][1], the ring's share of the batch, must be an int >= 0, got {n!r}")
        if any(ring is r for r, _ in out):
            raise ValueError(f"sample_mixed: pairs[{i}] names a ring that the list holds already; give a ring once, with its whole share")
        out.append((ring, int(n)))
    if sum(n for _, n in out) < 1:
        raise ValueError("sample_mixed: the shares add up to 0 rows; at least one row must be drawn")
    first = out[0][0]
    for i, (ring, _) in enumerate(out[1:], 1):
        for what, a, b in (("obs_shape", first.shapes["obs"], ring.shapes["obs"]), ("pstate_dim", first.fields["pobs"], ring.fields["pobs"]),
                           ("act_dim", first.fields["act"], ring.fields["act"]), ("device", first.store["obs"].device, ring.store["obs"].device)):
            if a != b:
                raise ValueError(f"sample_mixed: the rings must agree in {what}: {a!r} in pairs[0], {b!r} in pairs[{i}]")
    return out


def _per_ring(name, value, pairs, wanted):
    """a keyword of sample_mixed with one entry per pair (``uniforms``, ``indices``) after its checks -> list; ``wanted(ring)`` says which
    rings may have an entry"""
    if value is None:
        return [None] * len(pairs)
    if not isinstance(value, (list, tuple)) or len(value) != len(pairs):
        raise ValueError(f"sample_mixed: {name} must be None or a list with one entry per pair ({len(pairs)}), got {type(value).__name__}"
                         + (f" of {len(value)}" if isinstance(value, (list, tuple)) else ""))
    for i, ((ring, _), v) in enumerate(zip(pairs, value)):
        if v is not None and not wanted(ring):
            kind = "prioritized" if isinstance(ring, PrioritizedDeviceReplayBuffer) else "uniform"
            raise ValueError(f"sample_mixed: {name}[{i}] must be None: pairs[{i}] is a {kind} ring, which takes no {name}")
        if v is not None and not torch.is_tensor(v):
            raise ValueError(f"sample_mixed: {name}[{i}] must be None or a tensor, got {type(v).__name__}")
    out = []
    for i, ((_, n), v) in enumerate(zip(pairs, value)):
        if n == 0:                               # a skipped ring reads nothing, its entry included
            v = None
        elif v is not None and v.numel() != n:   # the row range is fixed by the share: sample() would take its B from the entry
            raise ValueError(f"sample_mixed: {name}[{i}] must hold {n} values, one per row of pairs[{i}]'s share, got {v.numel()}")
        elif v is not None and name == "indices" and (v.dtype.is_floating_point or v.dtype.is_complex or v.dtype == torch.bool):
            raise ValueError(f"sample_mixed: indices[{i}] must be an integer tensor, got {v.dtype}")
        out.append(v)
    return out


def sample_mixed(pairs, *, indices=None, random_shift: int = 0, return_shifts: bool = False, n_step: Optional[int] = None,
                 gamma: float = 0.99, frame_stack: Optional[int] = None, beta: float = 0.4, stratified: bool = False,
                 uniforms=None) -> MixedBatch:
    """ONE batch drawn from several rings -- the agent's and a demonstration ring, say::

        batch = sample_mixed([(agent_ring, 24), (demo_ring, 8)], random_shift=4, n_step=3, gamma=0.99, frame_stack=4, beta=0.4)
        update_priorities_mixed(batch, td)

    ``pairs`` is a list of 1 to 4 ``(ring, n_i)``, n_i >= 0 rows from that ring, at least one row in all.  A ring with n_i == 0 is skipped:
    it draws nothing, launches nothing and its generator does not move (a demonstration share that a schedule has taken to zero).  The
    rings must agree in ``obs_shape``, ``pstate_dim``, ``act_dim`` and device, and may differ in ``size``, ``frame_dtype``,
    ``shared_next_obs``, ``num_envs`` and in being uniform or prioritized; a mismatch, something that is no ring, a negative or non-integer
    n_i or the same ring twice raises ValueError before anything is launched, and an empty ring with n_i > 0 raises what ``sample`` raises.

    The keywords are ``sample()``'s and go to every ring's call; ``beta``, ``stratified`` and ``uniforms`` go to the prioritized rings
    only.  ``uniforms`` is then a list with one entry per pair, None where the ring is not prioritized (or where its draw is to come from
    its generator); ``indices`` is likewise a list with one entry per pair or None, an entry None where the ring draws for itself --
    a prioritized ring always does, so its entry must be None.  An entry holds exactly n_i values (integers for ``indices``), else
    ValueError before anything is launched: the row ranges are fixed by the shares.  The entry of a ring with n_i == 0 is not read.

    The result is ``sample()``'s dict, every key ONE ``(B, ...)`` tensor, B = sum n_i, ring 0's rows first, then ring 1's, and so on, plus
    ``source``, (B,) int32, the row's position in ``pairs``, and ``counts``, the tuple of n_i (a host value).  ``indexes`` are slots of
    the row's own ring.  ``weights`` is there when any ring of the list is prioritized: each prioritized ring's own importance weights,
    normalised within that ring as its ``sample`` does (by that ring's smallest leaf, not across rings), and 1 for the rows of uniform
    rings.  ``obs_shift`` / ``next_obs_shift``, ``discount`` and ``steps`` are there for all rows or for none, as the keywords say.

    The contract: ring i's rows of every key equal, bit for bit, what ``ring_i.sample(n_i, ...)`` returns from the same generator state,
    shift seed and keywords; the seeds of ``random_shift`` are drawn in list order.  Each ring issues the launches of its own ``sample``
    and no other, and they write straight into the ring's row range of the shared tensors: a frame is written once, there is no
    ``torch.cat`` and no staging copy.  What is added is one small fill per ring for ``source``, one for ``weights`` when uniform and
    prioritized rings mix, a copy of a given ``indices`` entry into ``indexes``, and the one trailing ``.contiguous()`` of a stack
    whose H W K is no multiple of 4, on the whole tensor.  The row ranges are host constants and nothing synchronises, so the call
    works inside ``GraphedStep`` under ``sample()``'s own conditions (``uniforms`` for prioritized rings, tracked episodes)."""
    pairs = _mixed_pairs(pairs)
    first = pairs[0][0]
    n_step, gamma, K = _n_step(n_step), _unit("gamma", gamma), _frame_stack(frame_stack)
    pad, beta = _shift_pad(random_shift, first.shapes["obs"], "random_shift"), _unit("beta", beta)
    per = [isinstance(ring, PrioritizedDeviceReplayBuffer) for ring, _ in pairs]
    uniforms = _per_ring("uniforms", uniforms, pairs, lambda ring: isinstance(ring, PrioritizedDeviceReplayBuffer))
    indices = _per_ring("indices", indices, pairs, lambda ring: not isinstance(ring, PrioritizedDeviceReplayBuffer))
    for ring, n in pairs:
        if n and ring.stored == 0:
            raise RuntimeError("cannot sample from an empty buffer")
    total, dev = sum(n for _, n in pairs), first.device
    batch = _Rows(total, dev)
    source = torch.empty(total, dtype=torch.int32, device=dev)
    if any(per) and any(n and not p for (_, n), p in zip(pairs, per)):        # rows of uniform rings: 1, the rest is overwritten
        batch.bufs["weights"] = torch.ones(total, 1, dtype=torch.float32, device=dev)
    for i, (ring, n) in enumerate(pairs):
        if n == 0:
            continue
        source[batch.r0:batch.r0 + n].fill_(i)
        idx = ring._draw(batch, n, beta, stratified, uniforms[i])[0] if per[i] else ring._slots_of_mixed(batch, n, indices[i])
        ring._sample_rows(batch, idx, pad, return_shifts, n_step, gamma, K)
        batch.r0 += n
    out = MixedBatch(_finish(batch, first.fields, first.shapes, pad, return_shifts, n_step, K))
    out["source"], out["counts"] = source, tuple(n for _, n in pairs)
    out.rings = tuple(ring for ring, _ in pairs)
    return out


def update_priorities_mixed(batch: MixedBatch, priorities: torch.Tensor) -> None:
    """``update_priorities`` for a ``sample_mixed`` batch: ``priorities`` ((B,) or (B, 1) fp32 on the device, typically
    ``critic_loss(...).td``) is cut into the rings' row ranges, and each prioritized ring with rows in the batch takes its range with its
    own ``indexes``; uniform rings and rings with a share of 0 are skipped.  The ranges are host constants: nothing synchronises."""
    if not isinstance(batch, MixedBatch) or len(batch.rings) != len(batch.get("counts", ())):
        raise ValueError("update_priorities_mixed: batch must be what sample_mixed returned")
    total = sum(batch["counts"])
    if not torch.is_tensor(priorities) or tuple(priorities.shape) not in ((total,), (total, 1)):
        got = tuple(priorities.shape) if torch.is_tensor(priorities) else type(priorities).__name__
        raise ValueError(f"update_priorities_mixed: priorities must be ({total},) or ({total}, 1), one per row of the batch, got {got}")
    flat, r0 = priorities.reshape(-1), 0
    for ring, n in zip(batch.rings, batch["counts"]):
        if n and isinstance(ring, PrioritizedDeviceReplayBuffer):
            ring.update_priorities(batch["indexes"][r0:r0 + n], flat[r0:r0 + n])
        r0 += n


def _stack_args(num_envs, obs_shape, frames):
    """``FrameStack``'s arguments after their checks -> (E, (H, W), K): host-only, runs before anything touches a device"""
    if isinstance(num_envs, bool) or not isinstance(num_envs, (int, np.integer)) or int(num_envs) < 1:
        raise ValueError(f"num_envs must be an int >= 1, got {num_envs!r}")
    shape = tuple(obs_shape) if isinstance(obs_shape, (tuple, list)) else ()
    if len(shape) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1 for v in shape):
        raise ValueError(f"obs_shape must be (H, W), two ints >= 1, got {obs_shape!r}")
    return int(num_envs), (int(shape[0]), int(shape[1])), _frame_stack(frames, "frames")


class FrameStack:
    """The acting side of ``sample(frame_stack=K)``: the last K frames of each of E environments as one live
    ``(E, H, W, K)`` fp32 device tensor, channel-last with channel K - 1 the newest -- what ``choose_action`` of a
    ``frame_channels=K`` network takes.

        fs = FrameStack(num_envs=E, obs_shape=(H, W), frames=K, device="cuda")
        stack = fs.push(frame, reset=None)

    ``push`` moves every environment's channels down by one and puts the new frame -- ``(E, H, W)``, or ``(H, W)`` when E == 1; an fp32
    tensor on the stack's device, or any host array or CPU tensor, which is copied over -- into channel K - 1.  Environments with ``reset``
    set have all K channels filled with the frame, as Gym's ``FrameStack`` does at reset: ``reset`` is None, ``True`` (everyone) or a bool
    mask ``(E,)`` on the host or the device; the first ``push`` (and the first after ``reset()``) resets everyone.  One launch,
    dgvit_frame_stack_push, thread = pixel; with device inputs (a device mask is read as the bytes it is) nothing synchronises, nothing
    else is launched and the call is capturable.  "Reset everyone" -- ``reset=True``, or the first push after construction or
    ``reset()`` -- is a host value passed to the kernel by value, so a capture freezes it: capture after a first eager ``push`` and
    pass resets as a device mask, which every replay reads anew; a push captured directly after ``reset()`` would refill every channel
    on every replay.  The returned tensor is the live buffer: valid until the next ``push``, clone it to keep it.

    Contract with the ring: in the usual loop -- ``push`` the new observation, store the transition with ``add`` / ``add_vec``, mark
    ``on_episode_end`` and pass ``reset`` for the environments that then start over -- the stack pushed at a step is bit-equal to
    ``sample(indices=[slot], frame_stack=K)["obs"]`` of the slot that step was stored in, as long as the K - 1 slots before it are still
    in the ring and, on a uint8 ring, as long as the frames are k / 255 values."""

    def __init__(self, num_envs: int = 1, obs_shape: Tuple[int, int] = (128, 160), frames: int = 4, device="cuda"):
        self.num_envs, self.obs_shape, self.frames = _stack_args(num_envs, obs_shape, frames)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DgvitError("FrameStack lives in HBM; pass a ROCm device")
        self.stack = torch.zeros(self.num_envs, *self.obs_shape, self.frames, dtype=torch.float32, device=self.device)
        self._fresh = True

    def reset(self) -> None:
        """Empty the stack: zeros, and the next ``push`` fills every environment's K channels with its frame"""
        self.stack.zero_()
        self._fresh = True

    def push(self, frame, reset=None) -> torch.Tensor:
        E, (H, W), K = self.num_envs, self.obs_shape, self.frames
        if torch.is_tensor(frame) and frame.device.type != "cpu":
            if frame.device != self.stack.device or frame.dtype != torch.float32:
                raise ValueError(f"frame: a device tensor must be float32 on {self.stack.device}, got {frame.dtype} on {frame.device}")
            frame = frame.detach()
        else:
            frame = torch.from_numpy(np.ascontiguousarray(np.asarray(frame.detach().numpy() if torch.is_tensor(frame) else frame),
                                                          dtype=np.float32)).to(self.device, non_blocking=True)
        if tuple(frame.shape) not in ((E, H, W),) + (((H, W),) if E == 1 else ()):
            raise ValueError(f"frame: expected ({E}, {H}, {W}){f' or ({H}, {W})' if E == 1 else ''}, got {tuple(frame.shape)}")
        frame = frame.reshape(E, H * W).contiguous()
        everyone, mask = self._fresh, None
        if isinstance(reset, (bool, np.bool_)):
            everyone, reset = everyone or bool(reset), None
        if reset is not None:                    # checked even where the first push resets everyone anyway
            if torch.is_tensor(reset) and reset.device.type != "cpu":
                if reset.device != self.stack.device or reset.dtype != torch.bool or tuple(reset.shape) != (E,):
                    raise ValueError(f"reset: a device mask must be ({E},) bool on {self.stack.device}, got {tuple(reset.shape)} {reset.dtype} "
                                     f"on {reset.device}")
                mask = reset.detach().contiguous().view(torch.uint8)   # the bool's own bytes: no cast launch, no allocation
            else:
                host = np.asarray(reset.numpy() if torch.is_tensor(reset) else reset)
                if host.dtype != np.bool_ or host.shape != (E,):
                    raise ValueError(f"reset must be None, True or a bool mask ({E},), got {reset!r}")
                mask = torch.from_numpy(host.astype(np.uint8)).to(self.device, non_blocking=True)
        with torch.cuda.device(self.device):
            rc = _lib.load().dgvit_frame_stack_push(_ptr(self.stack), _ptr(frame), H * W, _ptr(mask), int(everyone), E, H * W, K, _stream())
        _lib.check(rc, "dgvit_frame_stack_push")
        self._fresh = False
        return self.stack
