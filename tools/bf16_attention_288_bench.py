"""bf16 attention at 197 and 257 tokens (ViT-B/16 at 224x224 and 256x256, ViT-B/14 at 224x224) and the ViT-B encoder, on one GPU.

    python tools/bf16_attention_288_bench.py kernels --tokens 257 [--batch 440 --iters 20]
        the bf16 attention forward (with lse) and backward at B x H = 440 x 12 items, once per A/B form of the diagnostic library
        (dgvit_set_attention_bf16_long bits: 3 shipped, 1 per-item 8-wave dq, 2 per-item forward, 0 eight waves everywhere).  Run it
        under `rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python ...`, one token count per run: every form launches
        kernels of its own name (attn_fwd_bf16_stream288_kernel, attn_fwd_bf16_kernel<8 / 9>, attn_bwd_dq_bf16_kernel<8 / 9>), so the
        stats table gives each form's per-launch time.  Device-event times are printed too (profiler on: indicative only).
    python tools/bf16_attention_288_bench.py encoder [--image 256 --patch 16 --batch 440]
        the ViT-B encoder (depth 12, dim 768, 12 heads, MLP 3072) in the bf16 configuration: forward (no grad) and forward + backward
        in frames/s from device events, profiler off.  Prints one JSON line.  (ViT-B/14, the same 257 tokens as 256 @ 16:
        tools/bf16_patch14_bench.py.)
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dgvit_amd  # noqa: E402
from dgvit_amd import functional as F  # noqa: E402

FORMS = {3: "shipped (persistent fwd, 9-wave dq)", 2: "per-item fwd 9 waves, 9-wave dq", 1: "persistent fwd, 8-wave dq",
         0: "per-item fwd 8 waves, 8-wave dq"}


def timeit(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def kernels(a):
    B, H, N, DH = a.batch, 12, a.tokens, 64
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B, N, 3 * H * DH, device="cuda", generator=g).to(torch.bfloat16)
    dout = torch.randn(B, N, H * DH, device="cuda", generator=g).to(torch.bfloat16)
    res = {"batch": B, "heads": H, "tokens": N}
    with dgvit_amd.diagnostic_library() as lib:
        try:
            for bits in ((3,) if N <= 224 else (3, 2, 1, 0)):
                lib.dgvit_set_attention_bf16_long(bits)
                out, lse = F.op_attention_bf16(qkv, H, DH, want_lse=True)
                fwd = timeit(lambda: F.op_attention_bf16(qkv, H, DH, want_lse=True), a.iters)
                bwd = timeit(lambda: F.op_attention_bwd_bf16(qkv, out, dout, lse, H, DH), a.iters)
                res[FORMS[bits]] = {"fwd_ms": round(fwd, 4), "bwd_ms": round(bwd, 4)}
                print(N, FORMS[bits], res[FORMS[bits]], flush=True)
        finally:
            lib.dgvit_set_attention_bf16_long(-1)
    print(json.dumps(res), flush=True)


def encoder(a):
    B, D = a.batch, 768
    m = dgvit_amd.GoT(image_size=a.image, patch_size=a.patch, num_classes=2, dim=D, depth=12, heads=12, mlp_dim=3072, channels=1)
    m = m.cuda().eval().set_compute_dtype(torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(0)
    img, goal = torch.rand(B, a.image, a.image, device="cuda", generator=g), torch.randn(B, D, device="cuda", generator=g)
    tokens = (a.image // a.patch) ** 2 + 1
    with torch.no_grad():
        fwd = timeit(lambda: m(img, goal), a.iters)
    m.train()
    tgt = torch.randn(B, D, device="cuda", generator=g)

    def step():
        for p in m.parameters():
            p.grad = None
        ((m(img, goal) - tgt) ** 2).mean().backward()
    step_ms = timeit(step, max(3, a.iters // 2))
    res = {"image": a.image, "patch": a.patch, "tokens": tokens, "batch": B,
           "forward": {"ms": round(fwd, 3), "frames_per_s": round(B / fwd * 1e3, 1)},
           "fwd_bwd": {"ms": round(step_ms, 3), "frames_per_s": round(B / step_ms * 1e3, 1)},
           "peak_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernels", "encoder"])
    ap.add_argument("--batch", type=int, default=440)
    ap.add_argument("--tokens", type=int, default=257)
    ap.add_argument("--image", type=int, default=256)
    ap.add_argument("--patch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    kernels(a) if a.what == "kernels" else encoder(a)


if __name__ == "__main__":
    main()
