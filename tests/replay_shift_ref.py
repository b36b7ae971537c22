"""Host restatement of the random-shift draw of dgvit_gather_shift_frames and the torch form of the shift itself (shared by
test_replay_shift_host.py and test_gpu_replay_shift.py).

* ``draw_shifts``: Philox4x32-10 of tests/layer_dropout_ref.py keyed by the seed, counter (sample, 0, 0x53000000 | stream, 0); output word 0
  gives dy and word 1 gives dx by multiply-high, ``(r * (2*pad + 1)) >> 32) - pad`` -- written from the table in csrc/common.h and
  include/dgvit_hip.h, independent of the kernel.
* ``ref_shift``: replicate-pad then crop, in torch ops: a copy, so bit-exact.
"""
import numpy as np
import torch
import torch.nn.functional as F

from layer_dropout_ref import philox4x32_10

SHIFT_TAG = 0x53000000
# chosen on the CPU so that the restatement meets the conditions of test_replay_shift_host.py::test_restated_draw_* at pad 4, 4096 samples
SEED = 0x2545F4914F6CDD1D


def draw_shifts(n, pad, seed, stream):
    """(n, 2) int32: (dy, dx) of samples 0 .. n-1"""
    i = np.arange(n, dtype=np.uint64)
    ctr = np.stack([i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), np.full_like(i, SHIFT_TAG | stream), np.zeros_like(i)], axis=-1)
    r = philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    d = ((r[:, :2] * np.uint64(2 * pad + 1)) >> np.uint64(32)).astype(np.int64) - pad
    return d.astype(np.int32)


def ref_shift(frames, shifts, pad):
    """frames (B, H, W), shifts (B, 2) int (dy, dx) -> F.pad(mode="replicate", pad) cropped at (pad + dy, pad + dx) per frame"""
    H, W = frames.shape[-2:]
    p = F.pad(frames[:, None], (pad,) * 4, mode="replicate")[:, 0] if pad else frames
    return torch.stack([p[i, pad + dy:pad + dy + H, pad + dx:pad + dx + W] for i, (dy, dx) in enumerate(shifts.tolist())])
