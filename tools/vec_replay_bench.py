#!/usr/bin/env python3
"""What a vector step costs to store, add_vec against the single-environment store path, and what the strided walk costs a sample
(DESIGN 3.35).

    python tools/vec_replay_bench.py [--rounds 5] [--ring 4096] [--tree branch] [--out profiles/vec_replay_bench.jsonl]

128x160 frames, fp32 and uint8 rings of --ring slots (a multiple of 256), E in {1, 16, 256} environments.  Per ring and E, the time of ONE
vector step (wall clock around the calls and a final synchronize, so the host's share is in it):
  add_vec_device      add_vec with every field a device tensor: two launches, no host visit
  add_vec_host        add_vec with every field a numpy array: one pinned staging matrix, one copy, the same two launches
  add_batch_device    the single-environment route, add_batch of the same E transitions given as device tensors (since DESIGN 3.36 the
  add_batch_host      same two launches and no host visit), and given as numpy arrays.  It lays E different episodes in consecutive
                      slots, which n-step sampling would walk across: it is timed for its cost, not for its meaning
and, with device events around 1000 launches after 50 (200 samples after 10):
  kernel_store_frames dgvit_ring_store_frames alone, the two frame fields of the step
  copy_frames         its yardstick: tensor.copy_ of the same source bytes, two (E, H W) fp32 tensors into ring-shaped fp32 rows
  sample_nstep3_E1 / sample_nstep3_E16    sample(512, n_step=3) on an E = 1 ring (dgvit_nstep_walk) and on an E = 16 ring of the same size
                      (dgvit_nstep_walk_strided), fp32 frames
The forms are timed in turn, --rounds times over, so every form's spread stands beside the differences; one JSON line per form with the
per-round times, their median and their range, printed and written to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, NSTEP, GAMMA = 512, 128, 160, 3, 0.99
ENVS = (1, 16, 256)


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
    ap.add_argument("--ring", type=int, default=4096)
    ap.add_argument("--tree", default="branch", help="a label for the rows: which tree was measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vec_replay_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import dgvit_amd
    from dgvit_amd import _lib as L
    from dgvit_amd.replay import DeviceReplayBuffer
    if not torch.cuda.is_available():
        raise SystemExit("vec_replay_bench needs a ROCm device")
    if args.ring % max(ENVS):
        raise SystemExit(f"--ring must be a multiple of {max(ENVS)}")
    lib = dgvit_amd.load_library()
    ring = args.ring
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    rng = np.random.default_rng(0)
    forms = []
    for dtype, tag in ((torch.float32, "fp32"), (torch.uint8, "u8")):
        single = DeviceReplayBuffer(ring, obs_shape=(H, W), seed=0, frame_dtype=dtype)
        for E in ENVS:
            host = {"obs": rng.random((E, H, W), dtype=np.float32), "next_obs": rng.random((E, H, W), dtype=np.float32),
                    "pobs": rng.random((E, 2), dtype=np.float32), "next_pobs": rng.random((E, 2), dtype=np.float32),
                    "act": rng.random((E, 2), dtype=np.float32), "rew": rng.random((E, 1), dtype=np.float32), "done": np.zeros((E, 1), np.float32)}
            dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
            vec = DeviceReplayBuffer(ring, obs_shape=(H, W), seed=0, frame_dtype=dtype, num_envs=E)
            iters, warmup = (60, 5) if E < 256 else (10, 3)     # every timed window is several milliseconds long
            u8 = int(dtype is torch.uint8)

            def k_frames(vec=vec, dev=dev, E=E, u8=u8):
                s = vec.store
                L.check(lib.dgvit_ring_store_frames(p(dev["obs"]), 0, H * W, p(dev["next_obs"]), 0, H * W, p(s["obs"]), p(s["next_obs"]), u8,
                                                    s["obs"].shape[1], E, H * W, ring, 0, st), "dgvit_ring_store_frames")
            forms += [(f"add_vec_device_{tag}_E{E}", lambda vec=vec, dev=dev: vec.add_vec(**dev), 300, 20, _walled),
                      (f"add_vec_host_{tag}_E{E}", lambda vec=vec, host=host: vec.add_vec(**host), iters, warmup, _walled),
                      (f"add_batch_device_{tag}_E{E}", lambda single=single, dev=dev: single.add_batch(**dev), iters, warmup, _walled),
                      (f"add_batch_host_{tag}_E{E}", lambda single=single, host=host: single.add_batch(**host), iters, warmup, _walled),
                      (f"kernel_store_frames_{tag}_E{E}", k_frames, 1000, 50, _timed)]
            if not u8:
                rows = [torch.zeros(E, H * W, device="cuda") for _ in range(2)]

                def copies(rows=rows, dev=dev, E=E):
                    rows[0].copy_(dev["obs"].view(E, -1))
                    rows[1].copy_(dev["next_obs"].view(E, -1))
                forms.append((f"copy_frames_E{E}", copies, 1000, 50, _timed))
    g = torch.Generator(device="cuda").manual_seed(0)
    for E in (1, 16):
        buf = DeviceReplayBuffer(ring, obs_shape=(H, W), seed=0, num_envs=E)
        for k in buf.fields:
            buf.store[k].uniform_(generator=g)
        buf.store["done"].copy_((buf.store["done"] < 0.02).float())
        buf.stored = ring
        buf.track_episodes()
        buf.episode_flags.copy_((torch.rand(ring, device="cuda", generator=g) < 0.02).to(torch.uint8))
        buf.episode_flags[ring - E:] |= 2
        forms.append((f"sample_nstep3_E{E}", lambda buf=buf: buf.sample(B, n_step=NSTEP, gamma=GAMMA), 200, 10, _timed))
    times = {name: [] for name, *_ in forms}
    for _ in range(args.rounds):
        for name, fn, iters, warmup, clock in forms:
            times[name].append(clock(fn, iters, warmup))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for name, *_ in forms:
            t = times[name]
            line = json.dumps({"tree": args.tree, "form": name, "frame": [H, W], "ring": ring, "ms_median": round(statistics.median(t), 4),
                               "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "ms_rounds": [round(x, 4) for x in t]})
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
