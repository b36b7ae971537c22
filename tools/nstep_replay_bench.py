#!/usr/bin/env python3
"""What n-step sampling costs beside the one-step sample(), and what episode tracking costs an add().

    python tools/nstep_replay_bench.py [--rounds 5] [--ring 100000] [--tree branch] [--out profiles/nstep_replay_bench.jsonl]

B = 512 samples of 128x160 frames from rings of 100 000 transitions (the method and the shapes of tools/replay_u8_bench.py, so the figures
stand beside its sample_fp32 / sample_u8).  The forms are timed in turn, --rounds times over, so the spread of each is seen beside the
differences; one JSON line per form with the per-round times, their median and their range, printed and written to --out:
  sample_fp32_plain / _nstep3        the whole sample(B) of an fp32 ring: seven launches and the index draw, or five with n_step=3
  sample_u8_plain / _nstep3          the same on a uint8 ring
  sample_per_plain / _nstep3         the prioritized buffer (fp32 ring): the draw in front of the same launches
  graph_fp32_plain / _nstep3         sample(indices=fixed) captured in a graph and replayed (100 replays after 10)
  kernel_nstep_walk                  the walk launch alone, n = 3 (100 launches after 10, device events)
  add_untracked / add_tracked        one add() of a host transition (wall clock around 20 calls and a synchronize, after 5) on a small
                                     ring without and with episode flags: the one dgvit_ring_mark launch
On a tree without the feature (the parent commit, --tree parent) only the plain forms exist and only they are timed: they are the
yardstick that the feature may not move.  2 % of the slots carry END and 2 % have done = 1, so walks of every length occur.
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

B, H, W, NSTEP, GAMMA = 512, 128, 160, 3, 0.99


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
    ap.add_argument("--tree", default="branch", help="a label for the rows: which tree was measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nstep_replay_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import dgvit_amd
    from dgvit_amd import _lib as L
    from dgvit_amd.replay import DeviceReplayBuffer, PrioritizedDeviceReplayBuffer
    if not torch.cuda.is_available():
        raise SystemExit("nstep_replay_bench needs a ROCm device")
    lib = dgvit_amd.load_library()
    feature = hasattr(DeviceReplayBuffer, "track_episodes")
    ring = args.ring
    g = torch.Generator(device="cuda").manual_seed(0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

    def filled(cls, dtype):
        """a full ring, filled on the device: random frames, 2 % done, and (with the feature) 2 % END under one HEAD"""
        buf = cls(ring, obs_shape=(H, W), seed=0, frame_dtype=dtype)
        for k in buf.fields:
            if dtype is torch.uint8 and k in ("obs", "next_obs"):
                buf.store[k].random_(0, 256, generator=g)
            else:
                buf.store[k].uniform_(generator=g)
        buf.store["done"].copy_((buf.store["done"] < 0.02).float())
        buf.stored = ring
        if hasattr(buf, "tree"):
            buf._on_store(0, ring)
            buf.update_priorities(torch.arange(ring, device="cuda"), torch.rand(ring, device="cuda", generator=g) + 0.1)
        if feature:
            buf.track_episodes()
            buf.episode_flags.copy_((torch.rand(ring, device="cuda", generator=g) < 0.02).to(torch.uint8))
            buf.episode_flags[ring - 1] |= 2
        return buf
    buf32, buf8, per = filled(DeviceReplayBuffer, torch.float32), filled(DeviceReplayBuffer, torch.uint8), filled(PrioritizedDeviceReplayBuffer, torch.float32)
    fixed = buf32.sample_indices(B)

    def graphed(**kw):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                buf32.sample(0, indices=fixed, **kw)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            keep = buf32.sample(0, indices=fixed, **kw)
        return graph, keep

    rng = np.random.default_rng(0)
    one = {"obs": rng.random((H, W), dtype=np.float32), "next_obs": rng.random((H, W), dtype=np.float32), "pobs": np.zeros(2, np.float32),
           "next_pobs": np.zeros(2, np.float32), "act": np.zeros(2, np.float32), "rew": np.float32(1), "done": np.float32(0)}
    small = DeviceReplayBuffer(1000, obs_shape=(H, W), seed=0)
    g_plain, keep_plain = graphed()
    forms = [("sample_fp32_plain", lambda: buf32.sample(B), 20, 5, _timed), ("sample_u8_plain", lambda: buf8.sample(B), 20, 5, _timed),
             ("sample_per_plain", lambda: per.sample(B), 20, 5, _timed), ("graph_fp32_plain", g_plain.replay, 100, 10, _timed),
             ("add_untracked", lambda: small.add(**one), 20, 5, _walled)]
    if feature:
        kw = dict(n_step=NSTEP, gamma=GAMMA)
        g_nstep, keep_nstep = graphed(**kw)
        tracked = DeviceReplayBuffer(1000, obs_shape=(H, W), seed=0)
        tracked.track_episodes()
        w = {k: torch.empty(B, device="cuda") for k in ("ret", "done", "disc")}
        w4, steps, tail = torch.empty(B, 4, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda")

        def k_walk():
            s = buf32.store
            L.check(lib.dgvit_nstep_walk(p(s["rew"]), 4, p(s["done"]), 4, p(buf32.episode_flags), p(s["next_pobs"]), 4, p(fixed), B, ring, NSTEP,
                                         GAMMA, p(w["ret"]), p(w["done"]), p(w["disc"]), p(w4), p(steps), p(tail), st), "dgvit_nstep_walk")
        forms += [("sample_fp32_nstep3", lambda: buf32.sample(B, **kw), 20, 5, _timed), ("sample_u8_nstep3", lambda: buf8.sample(B, **kw), 20, 5, _timed),
                  ("sample_per_nstep3", lambda: per.sample(B, **kw), 20, 5, _timed), ("graph_fp32_nstep3", g_nstep.replay, 100, 10, _timed),
                  ("kernel_nstep_walk", k_walk, 100, 10, _timed), ("add_tracked", lambda: tracked.add(**one), 20, 5, _walled)]
    times = {name: [] for name, *_ in forms}
    for _ in range(args.rounds):
        for name, fn, iters, warmup, clock in forms:
            times[name].append(clock(fn, iters, warmup))
    rows = []
    for name, *_ in forms:
        t = times[name]
        rows.append({"tree": args.tree, "form": name, "B": B, "frame": [H, W], "ring": ring, "ms_median": round(statistics.median(t), 4),
                     "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "ms_rounds": [round(x, 4) for x in t]})
    if feature:
        med = {r["form"]: r["ms_median"] for r in rows}
        rows.append({"tree": args.tree, "form": "ratios_nstep3_over_plain_at_median", "steps_mean": round(float(keep_nstep["steps"].float().mean()), 3),
                     **{k: round(med[f"{k}_nstep3"] / med[f"{k}_plain"], 3) for k in ("sample_fp32", "sample_u8", "sample_per", "graph_fp32")},
                     "add_tracked_over_untracked": round(med["add_tracked"] / med["add_untracked"], 3)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in rows:
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
