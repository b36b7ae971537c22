#!/usr/bin/env python3
"""Long-sequence fp32 attention at 224x224 @ 8x8 (785 tokens), D 256 / H 8 / dim_head 64 / B 64.

    python tools/long_seq_bench.py                 # every step below, each in its own process under `timeout -k 10`, stops at the first failure
    python tools/long_seq_bench.py --step fwd      # one step in this process: fwd | bwd | step

fwd / bwd: the tiled attention kernels alone (dgvit_attention_forward_tiled / _backward_tiled), event-timed over --iters launches;
step: one encoder forward + backward + FlatAdam step of GoT(224x224, patch 8, dim 256, depth 6, heads 8, mlp 2048) with
long_sequence=True.  Reported as ms and, for the kernels, as a fraction of the 157 TFLOP/s fp32 MFMA peak counting EXECUTED FLOPs
(32-row padded tiles: forward 2 products, backward 7 -- S and dP are recomputed in both backward passes).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, IMG, PATCH, D, H, DH, DEPTH, MLP = 64, 224, 8, 256, 8, 64, 6, 2048
N = (IMG // PATCH) ** 2 + 1
PEAK = 157e12


def _timed(fn, iters, warmup=3):
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


def run_step(step, iters):
    import torch
    import dgvit_amd
    from dgvit_amd import functional as F
    dgvit_amd.load_library()
    np_ = (N + 31) // 32 * 32
    if step in ("fwd", "bwd"):
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, N, 3 * H * DH, device="cuda", generator=g)
        dout = torch.randn(B, N, H * DH, device="cuda", generator=g)
        out, lse = F.op_attention_fwd_tiled(qkv, H, DH)
        dqkv = torch.empty_like(qkv)
        if step == "fwd":
            ms = _timed(lambda: F.op_attention_fwd_tiled(qkv, H, DH), iters)
            flops = 2 * 2.0 * B * H * np_ * np_ * DH
        else:
            ms = _timed(lambda: F.op_attention_bwd_tiled(qkv, out, dout, lse, H, DH, dqkv=dqkv), iters)
            flops = 7 * 2.0 * B * H * np_ * np_ * DH
        return {"step": step, "ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 2), "mfma_peak_fraction": round(flops / ms / 1e9 / (PEAK / 1e12), 3)}
    from dgvit_amd.optim import FlatAdam
    m = dgvit_amd.GoT(image_size=IMG, patch_size=PATCH, num_classes=2, dim=D, depth=DEPTH, heads=H, mlp_dim=MLP, channels=1, dim_head=DH)
    m = m.cuda().train().set_schedule(long_sequence=True)
    opt = FlatAdam([m], lr=1e-4)
    g = torch.Generator(device="cuda").manual_seed(0)
    img = torch.rand(B, IMG, IMG, device="cuda", generator=g)
    goal = torch.randn(B, D, device="cuda", generator=g)

    def one():
        for q in m.parameters():
            q.grad = None
        m(img, goal).square().mean().backward()
        opt.step()
    ms = _timed(one, iters, warmup=2)
    return {"step": "step", "ms": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["fwd", "bwd", "step"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step (driver mode)")
    a = ap.parse_args()
    if a.step:
        print(json.dumps({"B": B, "N": N, "D": D, "H": H, "dim_head": DH, **run_step(a.step, a.iters)}), flush=True)
        return 0
    for step in ("fwd", "bwd", "step"):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                            "--iters", str(a.iters)])
        if r.returncode != 0:
            print(f"step {step} failed with exit status {r.returncode}; stopping", file=sys.stderr, flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
