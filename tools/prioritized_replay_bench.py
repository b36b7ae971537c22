#!/usr/bin/env python3
"""What prioritization costs on top of DeviceReplayBuffer.sample.

    python tools/prioritized_replay_bench.py [--rounds 5] [--ring 100000]

B = 512 samples of 128x160 frames from a ring of 100 000 transitions (a three-level tree) with random priorities, event-timed over 20
calls after 5 for (a) and (b) and 500 after 20 for (c) to (e), five forms in one interleaved run:
  (a) DeviceReplayBuffer.sample(B)                 the uniform index draw and the gather of every field
  (b) PrioritizedDeviceReplayBuffer.sample(B)      torch.rand, the tree descent with the importance weights, the same gathers
  (c) draw(B)                                      indices and weights alone (torch.rand + dgvit_per_sample)
  (d) update_priorities(indexes, |td|)             dgvit_per_update: two leaf passes and one rebuild per upper level
  (e) dgvit_gather_rows on the obs field           the gather of ONE frame field of the same batch (42 MB read + 42 MB written), the
                                                   yardstick for (c) and (d), which touch about B * levels * 256 B of the tree
The forms are timed in turn, --rounds times over, so the spread of each is seen beside the differences; one JSON line per form with the
per-round times, their median and their range.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W = 512, 128, 160


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=100_000)
    args = ap.parse_args()
    import torch
    import dgvit_amd
    from dgvit_amd import _lib as L
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    if not torch.cuda.is_available():
        raise SystemExit("prioritized_replay_bench needs a ROCm device")
    lib = dgvit_amd.load_library()
    ring = args.ring
    buf = PrioritizedDeviceReplayBuffer(ring, obs_shape=(H, W), seed=0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for k, t in buf.store.items():                      # the ring is filled on the device: add_batch would stage 16 GB through the host
        t[:, :buf.fields[k]].uniform_(generator=g)
    buf.stored = ring
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    L.check(lib.dgvit_per_set_range(p(buf.tree), ring, 0, ring, st), "dgvit_per_set_range")
    buf.update_priorities(torch.arange(ring, device="cuda"), torch.rand(ring, device="cuda", generator=g) * 10)
    total = float(buf.total_priority)
    assert abs(total - float(buf.priorities().double().sum())) <= 1e-4 * total

    idx, _ = buf.draw(B)
    td = torch.rand(B, device="cuda", generator=g) * 10
    out = torch.empty(B, H * W, device="cuda")
    src = buf.store["obs"]

    def uniform():
        return DeviceReplayBuffer.sample(buf, B)

    def prioritized():
        return buf.sample(B)

    def draw():
        return buf.draw(B)

    def update():
        buf.update_priorities(idx, td)

    def k_rows():
        L.check(lib.dgvit_gather_rows(p(src), p(idx), p(out), B, H * W, ring, st), "dgvit_gather_rows")

    forms = [("a_uniform_sample", uniform, 20, 5), ("b_prioritized_sample", prioritized, 20, 5), ("c_draw_indices_and_weights", draw, 500, 20),
             ("d_update_priorities", update, 500, 20), ("e_kernel_gather_rows_obs", k_rows, 500, 20)]
    times = {name: [] for name, *_ in forms}
    for _ in range(args.rounds):
        for name, fn, iters, warmup in forms:
            times[name].append(_timed(fn, iters, warmup))
    for name, *_ in forms:
        t = times[name]
        row = {"form": name, "B": B, "frame": [H, W], "ring": ring, "tree_levels": len(buf._levels), "ms_median": round(statistics.median(t), 4),
               "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "ms_rounds": [round(x, 4) for x in t]}
        if name.startswith("e_"):
            row["TB_per_s_at_median"] = round(2 * B * H * W * 4 / (statistics.median(t) * 1e-3) / 1e12, 3)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
