#!/usr/bin/env python3
"""What the uint8 replay ring costs and saves beside the fp32 ring.

    python tools/replay_u8_bench.py [--rounds 5] [--ring 100000] [--out profiles/replay_u8_bench.jsonl]

B = 512 samples of 128x160 frames from two rings of 100 000 transitions, one fp32 and one uint8, in one process.  The forms are timed in
turn, --rounds times over, so the spread of each is seen beside the differences; one JSON line per form with the per-round times, their
median and their range, printed and written to --out:
  kernel_gather_rows_fp32 / _u8      the plain frame gather on the obs field (100 launches after 10, device events), with the bytes each
                                     moves over its time: fp32 reads and writes B x 20 480 floats, u8 reads a quarter and writes the same
  kernel_gather_shift_fp32 / _u8     the shifted frame gather (pad 4), same counts
  kernel_quantize_u8                 dgvit_quantize_rows_u8 on B rows of an fp32 device matrix into the byte ring, same counts: reads B x
                                     20 480 floats and writes as many bytes
  sample_fp32 / sample_u8            the whole sample(B): seven launches and the index draw (20 calls after 5, device events)
  add_batch_fp32_floats / add_batch_u8_floats / add_batch_u8_bytes
                                     add_batch of 512 host frames (wall clock around the call and a synchronize, 5 calls after 2)
  ring_bytes                         torch.cuda.memory_allocated before and after each buffer is built
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, PAD = 512, 128, 160, 4


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


def _walled(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_u8_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import dgvit_amd
    from dgvit_amd import _lib as L
    from dgvit_amd.replay import DeviceReplayBuffer
    if not torch.cuda.is_available():
        raise SystemExit("replay_u8_bench needs a ROCm device")
    lib = dgvit_amd.load_library()
    ring = args.ring
    rows = []

    def built(dtype):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        buf = DeviceReplayBuffer(ring, obs_shape=(H, W), seed=0, frame_dtype=dtype)
        return buf, torch.cuda.memory_allocated() - before
    buf32, bytes32 = built(torch.float32)
    buf8, bytes8 = built(torch.uint8)
    rows.append({"form": "ring_bytes", "ring": ring, "frame": [H, W], "fp32": bytes32, "u8": bytes8, "u8_over_fp32": round(bytes8 / bytes32, 4)})
    g = torch.Generator(device="cuda").manual_seed(0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    every = torch.arange(ring, device="cuda")
    for k in ("obs", "next_obs"):                           # the rings are filled on the device, with the same k / 255 frames:
        buf8.store[k].random_(0, 256, generator=g)          # the fp32 ring is the identity gather of the byte ring
        L.check(lib.dgvit_gather_rows_u8(p(buf8.store[k]), p(every), p(buf32.store[k]), ring, H * W, H * W, H * W, ring, st),
                "dgvit_gather_rows_u8")
    for k in buf32.fields:
        if k not in ("obs", "next_obs"):
            buf32.store[k].uniform_(generator=g)
            buf8.store[k].copy_(buf32.store[k])
    buf32.stored = buf8.stored = ring

    idx = buf32.sample_indices(B)
    out = torch.empty(B, H * W, device="cuda")
    s32, s8 = buf32.store["obs"], buf8.store["obs"]

    def k_rows32():
        L.check(lib.dgvit_gather_rows(p(s32), p(idx), p(out), B, H * W, ring, st), "dgvit_gather_rows")

    def k_rows8():
        L.check(lib.dgvit_gather_rows_u8(p(s8), p(idx), p(out), B, H * W, H * W, H * W, ring, st), "dgvit_gather_rows_u8")

    def k_shift32():
        L.check(lib.dgvit_gather_shift_frames(p(s32), p(idx), p(out), None, B, H, W, H * W, ring, PAD, 0, 12345, None, st),
                "dgvit_gather_shift_frames")

    def k_shift8():
        L.check(lib.dgvit_gather_shift_frames_u8(p(s8), p(idx), p(out), None, B, H, W, H * W, H * W, ring, PAD, 0, 12345, None, st),
                "dgvit_gather_shift_frames_u8")

    frames32 = torch.rand(B, H * W, device="cuda", generator=g)

    def k_quantize8():                                      # the exported entry point alone; the package stores through ring_store_frames
        L.check(lib.dgvit_quantize_rows_u8(p(frames32), H * W, p(s8), B, H * W, H * W, ring, 0, st), "dgvit_quantize_rows_u8")

    k_rows32()
    want = out.clone()
    k_rows8()
    assert torch.equal(out, want), "the two rings hold the same k / 255 frames"

    rng = np.random.default_rng(0)
    codes = {k: rng.integers(0, 256, (B, H, W), dtype=np.uint8) for k in ("obs", "next_obs")}
    small = {"pobs": np.zeros((B, 2), np.float32), "next_pobs": np.zeros((B, 2), np.float32), "act": np.zeros((B, 2), np.float32),
             "rew": np.zeros((B, 1), np.float32), "done": np.zeros((B, 1), np.float32)}
    floats = {k: v.astype(np.float32) / np.float32(255) for k, v in codes.items()}

    forms = [("kernel_gather_rows_fp32", k_rows32, 100, 10, _timed), ("kernel_gather_rows_u8", k_rows8, 100, 10, _timed),
             ("kernel_gather_shift_fp32", k_shift32, 100, 10, _timed), ("kernel_gather_shift_u8", k_shift8, 100, 10, _timed),
             ("kernel_quantize_u8", k_quantize8, 100, 10, _timed),
             ("sample_fp32", lambda: buf32.sample(B), 20, 5, _timed), ("sample_u8", lambda: buf8.sample(B), 20, 5, _timed),
             ("add_batch_fp32_floats", lambda: buf32.add_batch(**small, **floats), 5, 2, _walled),
             ("add_batch_u8_floats", lambda: buf8.add_batch(**small, **floats), 5, 2, _walled),
             ("add_batch_u8_bytes", lambda: buf8.add_batch(**small, **codes), 5, 2, _walled)]
    times = {name: [] for name, *_ in forms}
    for _ in range(args.rounds):
        for name, fn, iters, warmup, clock in forms:
            times[name].append(clock(fn, iters, warmup))
    moved = {"fp32": 2 * B * H * W * 4, "u8": B * H * W * 5}
    for name, *_ in forms:
        t = times[name]
        row = {"form": name, "B": B, "frame": [H, W], "ring": ring, "ms_median": round(statistics.median(t), 4),
               "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "ms_rounds": [round(x, 4) for x in t]}
        if name.startswith("kernel"):
            row["bytes"] = moved[name.rsplit("_", 1)[1]]
            row["TB_per_s_at_median"] = round(row["bytes"] / (statistics.median(t) * 1e-3) / 1e12, 3)
        rows.append(row)
    med = {r["form"]: r["ms_median"] for r in rows if "ms_median" in r}
    rows.append({"form": "ratios_u8_over_fp32_at_median", "bytes_predict_gather": 0.625,
                 "kernel_gather_rows": round(med["kernel_gather_rows_u8"] / med["kernel_gather_rows_fp32"], 3),
                 "kernel_gather_shift": round(med["kernel_gather_shift_u8"] / med["kernel_gather_shift_fp32"], 3),
                 "sample": round(med["sample_u8"] / med["sample_fp32"], 3),
                 "add_batch_bytes_over_fp32_floats": round(med["add_batch_u8_bytes"] / med["add_batch_fp32_floats"], 3)})
    with open(args.out, "w") as f:
        for row in rows:
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
