#!/usr/bin/env python3
"""What storing each frame once costs and saves: DeviceReplayBuffer(shared_next_obs=True) against the two-matrix ring.

    python tools/shared_next_bench.py [--rounds 5] [--ring 100000] [--tree branch] [--out profiles/shared_next_bench.jsonl]

128x160 frames, fp32 and uint8 rings of --ring slots (a multiple of 16), E in {1, 16} environments.  Per ring format and E two buffers of
the same class live side by side, one of them shared; both are filled to the brim through the store path (2 % of the transitions end
their episode by done, so the pool is in use) and then, form by form and --rounds times over, the two are measured in turn:
  add_vec_device      add_vec with every field a device tensor (wall clock around the calls and a final synchronize)
  add_host            add (E = 1) or add_vec (E = 16) with every field a numpy array: one pinned staging matrix, one copy
  kernel_store_frames the frame launch alone, device events around 1000 launches after 50: dgvit_ring_store_frames (two fields) against
                      dgvit_ring_store_frames_shared (the obs rows and the pending rows; no moves)
  kernel_plan_next    the shared ring's bookkeeping launch alone, dgvit_ring_plan_next (no counterpart in the two-matrix ring)
  sample              sample(512), eager, device events around 200 calls after 10
  sample_nstep3_graph sample(512, n_step=3) captured once and replayed, device events around 200 replays after 10
One JSON line per form and buffer with the per-round times, their median and their range, and one line per buffer with the bytes it
allocated (torch.cuda.memory_allocated around the constructor) beside the arithmetic (size + E + P) row against 2 size row."""
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
ENVS = (1, 16)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_next_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import dgvit_amd
    from dgvit_amd import _lib as L
    from dgvit_amd.replay import DeviceReplayBuffer
    if not torch.cuda.is_available():
        raise SystemExit("shared_next_bench needs a ROCm device")
    if args.ring % max(ENVS):
        raise SystemExit(f"--ring must be a multiple of {max(ENVS)}")
    lib = dgvit_amd.load_library()
    ring = args.ring
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    rng = np.random.default_rng(0)
    lines = []

    def emit(**row):
        line = json.dumps({"tree": args.tree, "frame": [H, W], "ring": ring, **row})
        print(line, flush=True)
        lines.append(line)

    for dtype, tag in ((torch.float32, "fp32"), (torch.uint8, "u8")):
        for E in ENVS:
            u8 = int(dtype is torch.uint8)
            bufs = {}
            for kind, kw in (("two_matrix", {}), ("shared", {"shared_next_obs": True})):
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
                bufs[kind] = DeviceReplayBuffer(ring, obs_shape=(H, W), seed=0, frame_dtype=dtype, num_envs=E, **kw)
                row = bufs[kind].store["obs"].shape[1] * bufs[kind].store["obs"].element_size()
                P = bufs[kind].terminal_frames
                emit(form=f"bytes_{tag}_E{E}", buffer=kind, bytes_allocated=torch.cuda.memory_allocated() - before,
                     frame_bytes=(ring + E + P) * row if P else 2 * ring * row, terminal_frames=P)
            n = 4096 if E == 1 else E                       # the fill: demonstrations-sized runs for one environment, steps for sixteen
            host = {"obs": rng.random((n, H, W), dtype=np.float32), "next_obs": rng.random((n, H, W), dtype=np.float32),
                    "pobs": rng.random((n, 2), dtype=np.float32), "next_pobs": rng.random((n, 2), dtype=np.float32),
                    "act": rng.random((n, 2), dtype=np.float32), "rew": rng.random((n, 1), dtype=np.float32),
                    "done": (rng.random((n, 1)) < 0.02).astype(np.float32)}
            fill = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
            dev = {k: v[:E].contiguous() for k, v in fill.items()}
            step_host = {k: v[:E] for k, v in host.items()}
            one_host = {k: v[0] for k, v in host.items()}
            for buf in bufs.values():
                buf.track_episodes()
                while buf.stored < ring:
                    buf.add_batch(**fill) if E == 1 else buf.add_vec(**fill)
            moves = torch.full((E,), -1, dtype=torch.int32, device="cuda")
            idx = torch.randint(0, ring, (B,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
            forms = []
            for kind, buf in bufs.items():
                s, ld = buf.store, buf.store["obs"].shape[1]
                if kind == "shared":
                    def k_frames(buf=buf, ld=ld):
                        L.check(lib.dgvit_ring_store_frames_shared(p(dev["obs"]), 0, H * W, p(dev["next_obs"]), 0, H * W, p(buf.arena), p(moves),
                                                                   u8, ld, E, H * W, ring, 0, E, buf.terminal_frames, st),
                                "dgvit_ring_store_frames_shared")

                    table, fifo, plan = buf.next_row.clone(), buf._pool_state.clone(), moves.clone()   # the launch repeats on the same slots

                    def k_plan(buf=buf, table=table, fifo=fifo, plan=plan):
                        L.check(lib.dgvit_ring_plan_next(p(table), p(fifo), p(plan), p(buf.store["done"]), 4,
                                                         p(buf.episode_flags), E, ring, buf.next_index, E, buf.terminal_frames, st),
                                "dgvit_ring_plan_next")
                else:
                    def k_frames(s=s, ld=ld):
                        L.check(lib.dgvit_ring_store_frames(p(dev["obs"]), 0, H * W, p(dev["next_obs"]), 0, H * W, p(s["obs"]), p(s["next_obs"]),
                                                            u8, ld, E, H * W, ring, 0, st), "dgvit_ring_store_frames")
                    k_plan = None
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(2):
                        buf.sample(B, indices=idx, n_step=NSTEP, gamma=GAMMA)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    buf._static = buf.sample(B, indices=idx, n_step=NSTEP, gamma=GAMMA)
                host_add = (lambda buf=buf: buf.add(**one_host)) if E == 1 else (lambda buf=buf: buf.add_vec(**step_host))
                forms += [("add_vec_device", kind, lambda buf=buf: buf.add_vec(**dev), 300, 20, _walled),
                          ("add_host", kind, host_add, 60, 5, _walled),
                          ("kernel_store_frames", kind, k_frames, 1000, 50, _timed),
                          ("sample", kind, lambda buf=buf: buf.sample(B), 200, 10, _timed),
                          ("sample_nstep3_graph", kind, graph.replay, 200, 10, _timed)]
                if k_plan is not None:
                    forms.append(("kernel_plan_next", kind, k_plan, 1000, 50, _timed))
            forms.sort(key=lambda f: f[0])                  # the two buffers of a form one after the other, round after round
            times = {f[:2]: [] for f in forms}
            for _ in range(args.rounds):
                for name, kind, fn, iters, warmup, clock in forms:
                    times[(name, kind)].append(clock(fn, iters, warmup))
            for name, kind, *_ in forms:
                t = times[(name, kind)]
                emit(form=f"{name}_{tag}_E{E}", buffer=kind, ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4),
                     ms_max=round(max(t), 4), ms_rounds=[round(x, 4) for x in t])
            lost = bufs["shared"].lost_terminal_frames()
            emit(form=f"lost_terminal_frames_{tag}_E{E}", buffer="shared", lost=lost)
            del bufs, forms, graph, buf, fill, dev, s, k_frames, k_plan, host_add
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
