#!/usr/bin/env python3
"""What saving and loading the replay ring costs: save_transitions / load_transitions against the link's floor and against what a user
could do before they existed.

    python tools/replay_file_bench.py [--rounds 3] [--ring 20000] [--dir DIR] [--tree branch] [--out profiles/replay_file_bench.jsonl]

128x160 frames, rings of --ring slots, fp32 and uint8, two-matrix and shared, one environment.  Each ring is filled through the store
path (k / 255 frames, 2 % of the transitions end their episode by done) and then, form by form and --rounds times over:
  save            save_transitions(path, overwrite=True): wall clock around the call (it returns when the files are written)
  load            clear() and load_transitions(path) into a second ring of the same geometry, wall clock to a final synchronize
  user_save       the route without them: sample(indices=chunk) and .cpu() per field into fp32 memory-mapped .npy files
  user_load       add_batch of host arrays read from those files, chunk by chunk
  floor_d2h       device -> pinned-host copies that add up to the bytes of the save_transitions files, nothing else: the link alone
  kernel_export   the dgvit_ring_export launch of one chunk alone, device events around 20 launches after 3, against the bytes it
                  reads and writes
One JSON line per form and ring with the per-round seconds, their median and range, the bytes of the files and GB/s of file bytes (the
user route's files are fp32 whatever the ring, so its GB/s are of MORE bytes for the uint8 rings: compare the seconds).  Files go to
--dir (default: the system's temporary directory), whose file system decides what "disk" means here; it is named in every line."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, CHUNK = 128, 160, 4096
FIELDS = ("obs", "next_obs", "pobs", "act", "rew", "next_pobs", "done")


def _dir_bytes(path):
    return sum(os.path.getsize(os.path.join(path, n)) for n in os.listdir(path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ring", type=int, default=20000)
    ap.add_argument("--dir", default=None, help="where the files are written (default: the system's temporary directory)")
    ap.add_argument("--tree", default="branch", help="a label for the rows: which tree was measured")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_file_bench.jsonl"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from numpy.lib.format import open_memmap
    import dgvit_amd  # noqa: F401
    from dgvit_amd.replay import DeviceReplayBuffer
    if not torch.cuda.is_available():
        raise SystemExit("replay_file_bench needs a ROCm device")
    ring = args.ring
    work = tempfile.mkdtemp(prefix="replay_file_bench_", dir=args.dir)
    lines = []

    def emit(**row):
        line = json.dumps({"tree": args.tree, "frame": [H, W], "ring": ring, "dir": os.path.dirname(work), **row})
        print(line, flush=True)
        lines.append(line)

    def walled(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    try:
        g = torch.Generator(device="cuda").manual_seed(0)
        for dtype, tag in ((torch.float32, "fp32"), (torch.uint8, "u8")):
            for kind, kw in (("two_matrix", {}), ("shared", {"shared_next_obs": True})):
                bufs = [DeviceReplayBuffer(ring, obs_shape=(H, W), seed=0, frame_dtype=dtype, **kw) for _ in range(2)]
                buf, other = bufs
                n = min(CHUNK, ring)
                codes = torch.randint(0, 256, (n + 1, H, W), dtype=torch.uint8, device="cuda", generator=g)
                frames = codes if dtype is torch.uint8 else codes.float() / 255
                done = (torch.rand(n, 1, device="cuda", generator=g) < 0.02).float()
                fill = {"obs": frames[:n], "next_obs": frames[1:], "pobs": torch.rand(n, 2, device="cuda", generator=g),
                        "act": torch.rand(n, 2, device="cuda", generator=g), "rew": torch.rand(n, 1, device="cuda", generator=g),
                        "next_pobs": torch.rand(n, 2, device="cuda", generator=g), "done": done}
                while buf.stored < ring:
                    m = min(n, ring - buf.stored)
                    buf.add_batch(**{k: v[:m] for k, v in fill.items()})
                    buf.on_episode_end()                 # a filling run is one episode: the shared ring's contract holds at its seams
                path, user = os.path.join(work, "ring"), os.path.join(work, "user")
                buf.save_transitions(path)               # warm-up, and the file the loads read
                file_bytes = _dir_bytes(path)

                def save():
                    buf.save_transitions(path, overwrite=True)

                def load():
                    other.clear()
                    other.load_transitions(path)

                def user_save():
                    os.makedirs(user, exist_ok=True)
                    files = {k: open_memmap(os.path.join(user, k + ".npy"), mode="w+", dtype=np.float32, shape=(ring, *buf.shapes[k]))
                             for k in FIELDS}
                    oldest = buf.next_index if buf.stored == ring else 0
                    for a0 in range(0, ring, CHUNK):
                        m = min(CHUNK, ring - a0)
                        idx = (oldest + a0 + torch.arange(m, device="cuda")) % ring
                        out = buf.sample(m, indices=idx)
                        for k in FIELDS:
                            files[k][a0:a0 + m] = out[k].cpu().numpy()
                    for f in files.values():
                        f.flush()

                def user_load():
                    other.clear()
                    files = {k: np.load(os.path.join(user, k + ".npy"), mmap_mode="r") for k in FIELDS}
                    for a0 in range(0, ring, CHUNK):
                        other.add_batch(**{k: np.asarray(files[k][a0:a0 + CHUNK]) for k in FIELDS})

                piece = min(file_bytes, 1 << 30)
                src = torch.empty(piece, dtype=torch.uint8, device="cuda")
                pinned = torch.empty(piece, dtype=torch.uint8, pin_memory=True)

                def floor():
                    left = file_bytes
                    while left > 0:
                        m = min(left, piece)
                        pinned[:m].copy_(src[:m], non_blocking=True)
                        left -= m

                user_save()                              # warm-up, and the files user_load reads
                user_bytes = _dir_bytes(user)
                forms = [("save", save, file_bytes), ("load", load, file_bytes), ("user_save", user_save, user_bytes),
                         ("user_load", user_load, user_bytes), ("floor_d2h", floor, file_bytes)]
                times = {name: [] for name, _, _ in forms}
                for _ in range(args.rounds):
                    for name, fn, _ in forms:
                        times[name].append(walled(fn))
                for name, _, nbytes in forms:
                    t = times[name]
                    med = statistics.median(t)
                    emit(form=f"{name}_{tag}", buffer=kind, s_median=round(med, 4), s_min=round(min(t), 4), s_max=round(max(t), 4),
                         s_rounds=[round(x, 4) for x in t], bytes=nbytes, gb_per_s=round(nbytes / med / 1e9, 3))
                out = torch.empty(buf._layout(n)[1], dtype=torch.uint8, device="cuda")
                for _ in range(3):
                    buf._export_chunk(0, n, out=out)
                rounds = []
                for _ in range(args.rounds):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    for _ in range(20):
                        buf._export_chunk(0, n, out=out)
                    b.record()
                    torch.cuda.synchronize()
                    rounds.append(a.elapsed_time(b) / 20)
                med = statistics.median(rounds)
                emit(form=f"kernel_export_{tag}", buffer=kind, ms_median=round(med, 4), ms_min=round(min(rounds), 4),
                     ms_max=round(max(rounds), 4), ms_rounds=[round(x, 4) for x in rounds], chunk=n, bytes_read_and_written=2 * out.numel(),
                     gb_per_s=round(2 * out.numel() / med / 1e6, 1))
                del bufs, buf, other, fill, frames, codes, src, pinned, out
                torch.cuda.empty_cache()
                shutil.rmtree(path)
                shutil.rmtree(user)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
