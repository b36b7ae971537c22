#!/usr/bin/env python3
"""What a frame stack at sample time costs: sample(frame_stack=4) against the plain sample and against stacking by hand.

    python tools/frame_stack_bench.py [--rounds 5] [--ring 100000] [--tree lds_staged_stores] [--out profiles/frame_stack_bench.jsonl]

B = 512, 128x160 frames, fp32 and uint8 rings of --ring slots filled to the brim (2 % of the transitions end their episode by done, so
stacks are cut), K = 4, with and without random_shift=4, eager and as a replayed graph.  Per ring format, form by form and --rounds times
over, measured in turn at the same indices (device events around 200 calls after 10):
  plain     sample(512)                                   the single-frame batch: baseline (a)
  stacked   sample(512, frame_stack=4)
  byhand    K sample(indices=(idx - k) % ring) calls and torch.stack(dim=-1) of obs and of next_obs: the route a user has without the
            keyword, baseline (b) -- with no episode logic at all, which flatters it
and the frame gather alone (device events around 1000 launches after 50): dgvit_gather_stack_frames on the obs field against
dgvit_gather_rows / dgvit_gather_rows_u8, with the bytes each moves (ring bytes read + fp32 bytes written) per second.
One JSON line per form with the per-round times, their median and their range."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, K, SHIFT = 512, 128, 160, 4, 4


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


def _graph(fn, keep):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep.append(fn())        # the replays' outputs stay allocated
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=100000)
    ap.add_argument("--tree", default="lds_staged_stores", help="a label for the rows: which form of the stacked gather was measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_stack_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    import dgvit_amd
    from dgvit_amd import _lib as L
    from dgvit_amd.replay import DeviceReplayBuffer
    if not torch.cuda.is_available():
        raise SystemExit("frame_stack_bench needs a ROCm device")
    lib = dgvit_amd.load_library()
    ring, cols = args.ring, H * W
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    rng = np.random.default_rng(0)
    lines = []

    def emit(**row):
        line = json.dumps({"tree": args.tree, "frame": [H, W], "ring": ring, "batch": B, "frames": K, **row})
        print(line, flush=True)
        lines.append(line)

    n = 4096
    fill = {"obs": torch.from_numpy(rng.integers(0, 256, (n, H, W), dtype=np.uint8)).cuda().float() / 255.0,
            "pobs": torch.from_numpy(rng.random((n, 2), dtype=np.float32)).cuda(),
            "next_pobs": torch.from_numpy(rng.random((n, 2), dtype=np.float32)).cuda(),
            "act": torch.from_numpy(rng.random((n, 2), dtype=np.float32)).cuda(),
            "rew": torch.from_numpy(rng.random((n, 1), dtype=np.float32)).cuda(),
            "done": torch.from_numpy((rng.random((n, 1)) < 0.02).astype(np.float32)).cuda()}
    fill["next_obs"] = fill["obs"].roll(-1, 0)
    idx = torch.randint(0, ring, (B,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    back = [(idx - k) % ring for k in range(K)]

    for dtype, tag in ((torch.float32, "fp32"), (torch.uint8, "u8")):
        buf = DeviceReplayBuffer(ring, obs_shape=(H, W), seed=0, frame_dtype=dtype)
        buf.track_episodes()
        while buf.stored < ring:
            buf.add_batch(**fill)
        u8 = int(dtype is torch.uint8)
        item, ld = (1, buf.row_bytes) if u8 else (4, buf.rows["obs"])

        def by_hand(shift):
            parts = [buf.sample(B, indices=back[K - 1 - c], random_shift=shift) for c in range(K)]
            out = dict(parts[-1])
            for k in ("obs", "next_obs"):
                out[k] = torch.stack([q[k] for q in parts], dim=-1)
            return out

        forms, keep = [], []
        for shift in (0, SHIFT):
            calls = {"plain": lambda s=shift: buf.sample(B, indices=idx, random_shift=s),
                     "stacked": lambda s=shift: buf.sample(B, indices=idx, random_shift=s, frame_stack=K),
                     "byhand": lambda s=shift: by_hand(s)}
            for name, fn in calls.items():
                forms.append((f"{name}_shift{shift}_eager_{tag}", fn, 200, 10))
                forms.append((f"{name}_shift{shift}_graph_{tag}", _graph(fn, keep).replay, 200, 10))
        rows = torch.stack(back[::-1], dim=1).contiguous()
        out1 = torch.empty(B, cols, device="cuda")
        outk = torch.empty(B, cols * K, device="cuda")
        src = buf.store["obs"]

        def k_plain():
            if u8:
                L.check(lib.dgvit_gather_rows_u8(p(src), p(idx), p(out1), B, cols, ld, cols, ring, st), "dgvit_gather_rows_u8")
            else:
                L.check(lib.dgvit_gather_rows(p(src), p(idx), p(out1), B, cols, ring, st), "dgvit_gather_rows")

        def k_stack():
            L.check(lib.dgvit_gather_stack_frames(p(src), p(src), p(rows), p(outk), B, cols, K, u8, ld, cols * K, ring, ring, st),
                    "dgvit_gather_stack_frames")

        forms += [(f"kernel_gather_plain_{tag}", k_plain, 1000, 50), (f"kernel_gather_stack_{tag}", k_stack, 1000, 50)]
        moved = {f"kernel_gather_plain_{tag}": B * cols * (item + 4), f"kernel_gather_stack_{tag}": B * cols * K * (item + 4)}
        forms.sort(key=lambda f: f[0].split("_", 1)[1])      # the forms that are compared one after the other, round after round
        times = {f[0]: [] for f in forms}
        for _ in range(args.rounds):
            for name, fn, iters, warmup in forms:
                times[name].append(_timed(fn, iters, warmup))
        for name, *_ in forms:
            t = times[name]
            extra = {}
            if name in moved:
                extra = {"bytes_moved": moved[name], "gb_per_s_median": round(moved[name] / statistics.median(t) / 1e6, 1)}
            emit(form=name, ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                 ms_rounds=[round(x, 4) for x in t], **extra)
        del buf, forms, src, calls, keep
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
