#!/usr/bin/env python3
"""Long-sequence bf16 attention: ViT-B/16 at 384x384 (577 tokens), D 768 / H 12 / dim_head 64 / depth 12 / MLP 3072.

    python tools/bf16_long_seq_bench.py                 # every step below, each in its own process under `timeout -k 10`, stops at the first failure
    python tools/bf16_long_seq_bench.py --step kernels  # one step in this process: kernels | encoder

kernels: the three tiled kernels alone (dgvit_attention_forward_bf16_tiled, and the backward's two launches together) at 577 tokens,
         with 4-wave (128-row) and 8-wave (256-row) workgroups of the diagnostic library, beside the fused kernels at 288 tokens
         (per-item: fewer than 512 (frame, head) items; persistent: 512 or more), event-timed over --iters launches after warm-up.
         Reported as ms, as ns per 32x32 TILE PRODUCT of the score matrix (time / (B H ceil(N/32)^2): what the kernels can be compared
         by across token counts) and as a fraction of the 2.5 PFLOP/s bf16 MFMA peak counting EXECUTED FLOPs on padded 32-row tiles
         (forward 2 products, backward 7 -- S and dP are recomputed in both backward passes).
encoder: GoT forward (no-grad) and forward + backward of the ViT-B/16 384x384 encoder in bf16 with long_sequence_bf16=True.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

IMG, PATCH, D, H, DH, DEPTH, MLP = 384, 16, 768, 12, 64, 12, 3072
N = (IMG // PATCH) ** 2 + 1
PEAK = 2.5e15


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


def _row(name, B, n, ms, products):
    nt = (n + 31) // 32
    tiles = B * H * nt * nt
    flops = products * 2.0 * tiles * 32 * 32 * DH
    return {"kernel": name, "B": B, "N": n, "ms": round(ms, 4), "ns_per_tile_product": round(ms * 1e6 / tiles, 3),
            "mfma_peak_fraction": round(flops / (ms * 1e-3) / PEAK, 4)}


def run_kernels(iters):
    import torch
    import dgvit_amd
    from dgvit_amd import functional as F
    rows = []

    def data(B, n):
        g = torch.Generator(device="cuda").manual_seed(0)
        qkv = torch.randn(B, n, 3 * H * DH, device="cuda", generator=g).to(torch.bfloat16)
        dout = torch.randn(B, n, H * DH, device="cuda", generator=g).to(torch.bfloat16)
        return qkv, dout
    with dgvit_amd.diagnostic_library() as lib:
        try:
            qkv, dout = data(64, N)
            for waves in (4, 8):
                lib.dgvit_set_attention_bf16_tiled_waves(waves)
                out, lse = F.op_attention_bf16_tiled(qkv, H, DH, want_lse=True)
                rows.append(_row(f"tiled forward, {waves} waves", 64, N, _timed(lambda: F.op_attention_bf16_tiled(qkv, H, DH, want_lse=True), iters), 2))
                rows.append(_row(f"tiled backward, {waves} waves", 64, N, _timed(lambda: F.op_attention_bwd_bf16_tiled(qkv, out, dout, lse, H, DH), iters), 7))
        finally:
            lib.dgvit_set_attention_bf16_tiled_waves(0)
        for B, name in ((40, "per-item"), (64, "persistent")):     # 480 / 768 (frame, head) items
            qkv, dout = data(B, 288)
            out, lse = F.op_attention_bf16(qkv, H, DH, want_lse=True)
            rows.append(_row(f"fused forward, {name}", B, 288, _timed(lambda: F.op_attention_bf16(qkv, H, DH, want_lse=True), iters), 2))
            rows.append(_row(f"fused backward, {name} batch", B, 288, _timed(lambda: F.op_attention_bwd_bf16(qkv, out, dout, lse, H, DH), iters), 7))
    return rows


def run_encoder(iters, B):
    import torch
    import dgvit_amd
    m = dgvit_amd.GoT(image_size=IMG, patch_size=PATCH, num_classes=2, dim=D, depth=DEPTH, heads=H, mlp_dim=MLP, channels=1, dim_head=DH,
                      emb_dropout=0.)
    m = m.cuda().set_compute_dtype(torch.bfloat16).set_schedule(long_sequence_bf16=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    img = torch.rand(B, IMG, IMG, device="cuda", generator=g)
    goal = torch.randn(B, D, device="cuda", generator=g)

    def fwd():
        with torch.no_grad():
            m(img, goal)

    def fwdbwd():
        for q in m.parameters():
            q.grad = None
        m(img, goal).square().mean().backward()
    m.eval()
    f = _timed(fwd, iters, warmup=2)
    m.train()
    fb = _timed(fwdbwd, iters, warmup=2)
    return [{"encoder": "ViT-B/16 384x384 bf16", "B": B, "N": N, "forward_ms": round(f, 3), "forward_frames_per_s": round(B / f * 1e3, 1),
             "forward_backward_ms": round(fb, 3), "forward_backward_frames_per_s": round(B / fb * 1e3, 1)}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "encoder"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32, help="frames of the encoder step")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per step (driver mode)")
    a = ap.parse_args()
    if a.step:
        for r in (run_kernels(a.iters) if a.step == "kernels" else run_encoder(a.iters, a.batch)):
            print(json.dumps({"H": H, "dim_head": DH, **r}), flush=True)
        return 0
    for step in ("kernels", "encoder"):
        r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--step", step,
                            "--iters", str(a.iters), "--batch", str(a.batch)])
        if r.returncode != 0:
            print(f"step {step} failed with exit status {r.returncode}; stopping", file=sys.stderr, flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
