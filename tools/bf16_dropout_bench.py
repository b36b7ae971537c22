#!/usr/bin/env python3
"""What transformer dropout costs in the bf16 configuration: forward + backward of BASELINE config 5 (224x224 @ 16, D 768,
12 layers, 12 heads, MLP 3072) at B = 256 -- the shape and batch of profiles/*_c5_bf16_train_kernel_stats.csv (tools/c5_step.py).

    python tools/bf16_dropout_bench.py [--parent-root DIR] [--out profiles/bf16_dropout_bench.jsonl]
        arms, each in its own process under `timeout -k 10`, stopping at the first failure:
          parent_p0   p = 0 on a built checkout of the parent commit at DIR (skipped without --parent-root)
          tree_p0     p = 0 on this tree: the same launches as the parent, so the two agree inside their round-to-round range
          tree_p01    p = 0.1 on this tree under set_schedule(dropout_bf16=True)
        one JSON line per arm: median, minimum and maximum of --rounds rounds of --iters event-timed steps each.
    python tools/bf16_dropout_bench.py --arm NAME --p P [--root DIR]      one arm in this process (also the program to put behind
        `rocprofv3 --kernel-trace --stats --` for the split by kernel; use --rounds 1 --iters 4)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG, PATCH, D, H, DEPTH, MLP = 224, 16, 768, 12, 12, 3072


def run_arm(name, root, p, batch, rounds, iters):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    import dgvit_amd
    torch.manual_seed(5)
    m = dgvit_amd.GoT(image_size=IMG, patch_size=PATCH, num_classes=2, dim=D, depth=DEPTH, heads=H, mlp_dim=MLP, channels=1, dropout=p)
    m = m.cuda()
    if p > 0:
        m.set_schedule(dropout_bf16=True)
    m.set_compute_dtype(torch.bfloat16).train()
    g = torch.Generator(device="cuda").manual_seed(0)
    img, goal = torch.rand(batch, IMG, IMG, device="cuda", generator=g), torch.randn(batch, D, device="cuda", generator=g)
    tgt = torch.randn(batch, D, device="cuda", generator=g)

    def step():
        for q in m.parameters():
            q.grad = None
        ((m(img, goal) - tgt) ** 2).mean().backward()
    for _ in range(3):
        step()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    med = statistics.median(ms)
    return {"arm": name, "p": p, "B": batch, "image": IMG, "patch": PATCH, "dim": D, "depth": DEPTH, "heads": H, "mlp_dim": MLP,
            "rounds": rounds, "iters": iters, "step_ms_median": round(med, 3), "step_ms_min": round(min(ms), 3),
            "step_ms_max": round(max(ms), 3), "frames_per_s": round(batch / med * 1e3, 1), "step_ms_rounds": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", help="run this one arm in this process")
    ap.add_argument("--p", type=float, default=0.0)
    ap.add_argument("--root", default=ROOT, help="checkout the arm imports dgvit_amd from")
    ap.add_argument("--parent-root", help="a built checkout of the parent commit (driver mode)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per arm (driver mode)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_dropout_bench.jsonl"))
    a = ap.parse_args()
    if a.arm:
        print(json.dumps(run_arm(a.arm, a.root, a.p, a.batch, a.rounds, a.iters)), flush=True)
        return 0
    arms = ([("parent_p0", a.parent_root, 0.0)] if a.parent_root else []) + [("tree_p0", ROOT, 0.0), ("tree_p01", ROOT, 0.1)]
    lines = []
    for name, root, p in arms:
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--arm", name, "--p", str(p),
                            "--root", root, "--batch", str(a.batch), "--rounds", str(a.rounds), "--iters", str(a.iters)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"arm {name} failed with exit status {r.returncode}; stopping", file=sys.stderr, flush=True)
            return r.returncode
        line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
