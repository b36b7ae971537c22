#!/usr/bin/env python3
"""What the DrQ random shift costs inside DeviceReplayBuffer.sample.

    python tools/replay_shift_bench.py [--rounds 5]

B = 512 samples of 128x160 frames from a ring of 10 000 transitions, event-timed over 20 calls after 5, three forms:
  (a) sample(B)                       the plain gather of every field
  (b) sample(B, random_shift=4)       obs and next_obs through dgvit_gather_shift_frames
  (c) sample(B) + the shift in torch  pad (replicate), per-sample index grids, gather -- what a caller had to write before
and the two frame kernels alone on the obs field (dgvit_gather_rows / dgvit_gather_shift_frames, 100 launches after 10), with the
bytes each moves (one read and one write of B x 20 480 floats) over its time.  The forms are timed in turn, --rounds times over, so
the spread of (a) is seen beside the differences; one JSON line per form with the per-round times, their median and their range.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, PAD, RING = 512, 128, 160, 4, 10000


def _timed(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def torch_shift(frames, pad, gen):
    """the shift from torch ops after sample(): pad, per-sample index grids, gather"""
    import torch
    import torch.nn.functional as F
    n, h, w = frames.shape
    d = torch.randint(0, 2 * pad + 1, (n, 2), device=frames.device, generator=gen)
    p = F.pad(frames[:, None], (pad,) * 4, mode="replicate")[:, 0]
    ys = d[:, 0, None] + torch.arange(h, device=frames.device)
    xs = d[:, 1, None] + torch.arange(w, device=frames.device)
    flat = (ys[:, :, None] * (w + 2 * pad) + xs[:, None, :]).reshape(n, h * w)
    return p.reshape(n, -1).gather(1, flat).reshape(n, h, w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    import dgvit_amd
    from dgvit_amd import _lib as L
    from dgvit_amd.replay import DeviceReplayBuffer
    if not torch.cuda.is_available():
        raise SystemExit("replay_shift_bench needs a ROCm device")
    lib = dgvit_amd.load_library()
    buf = DeviceReplayBuffer(RING, obs_shape=(H, W), seed=0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for k, t in buf.store.items():                      # the ring is filled on the device: add_batch would stage 1.6 GB through the host
        t[:, :buf.fields[k]].uniform_(generator=g)
    buf.stored = RING
    gen = torch.Generator(device="cuda").manual_seed(1)

    def plain():
        return buf.sample(B)

    def fused():
        return buf.sample(B, random_shift=PAD)

    def restated():
        b = buf.sample(B)
        b["obs"], b["next_obs"] = torch_shift(b["obs"], PAD, gen), torch_shift(b["next_obs"], PAD, gen)
        return b

    idx = buf.sample_indices(B)
    out = torch.empty(B, H * W, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    src = buf.store["obs"]

    def k_rows():
        L.check(lib.dgvit_gather_rows(p(src), p(idx), p(out), B, H * W, RING, st), "dgvit_gather_rows")

    def k_shift():
        L.check(lib.dgvit_gather_shift_frames(p(src), p(idx), p(out), None, B, H, W, H * W, RING, PAD, 0, 12345, None, st),
                "dgvit_gather_shift_frames")

    forms = [("a_sample", plain, 20, 5), ("b_sample_random_shift_4", fused, 20, 5), ("c_sample_then_torch_shift", restated, 20, 5),
             ("kernel_gather_rows_obs", k_rows, 100, 10), ("kernel_gather_shift_frames_obs", k_shift, 100, 10)]
    times = {name: [] for name, *_ in forms}
    for _ in range(args.rounds):
        for name, fn, iters, warmup in forms:
            times[name].append(_timed(fn, iters, warmup))
    for name, *_ in forms:
        t = times[name]
        row = {"form": name, "B": B, "frame": [H, W], "ring": RING, "ms_median": round(statistics.median(t), 4),
               "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "ms_rounds": [round(x, 4) for x in t]}
        if name.startswith("kernel"):
            row["TB_per_s_at_median"] = round(2 * B * H * W * 4 / (statistics.median(t) * 1e-3) / 1e12, 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
