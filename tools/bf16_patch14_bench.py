"""The bf16 ViT-B encoder at 257 tokens with 14x14 patches (224x224) beside 16x16 patches (256x256), on one GPU.

    python tools/bf16_patch14_bench.py [--batch 440 --iters 20 --configs 14,16]
        ViT-B (depth 12, dim 768, 12 heads, MLP 3072) in the bf16 configuration: forward (no grad) and forward + backward in frames/s
        from device events after warm-up, ViT-B/14 at 224x224 and ViT-B/16 at 256x256 in the same process.  Both have 257 tokens; they
        differ in the patch GEMM's K (196 pixels padded to 200 against 256) and in the patchify pass (the padding kernel against the
        vectorised one).  One JSON line per configuration.  For the per-launch split run one configuration under
        `rocprofv3 --kernel-trace --stats -d <dir> -o <name> -- python tools/bf16_patch14_bench.py --configs 14 --iters 5`.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dgvit_amd  # noqa: E402

VITB = dict(dim=768, depth=12, heads=12, mlp_dim=3072)
CONFIGS = {"14": (224, 14), "16": (256, 16)}


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


def encoder(image, patch, batch, iters):
    D = VITB["dim"]
    m = dgvit_amd.GoT(image_size=image, patch_size=patch, num_classes=2, channels=1, **VITB)
    m = m.cuda().eval().set_compute_dtype(torch.bfloat16)
    g = torch.Generator(device="cuda").manual_seed(0)
    img, goal = torch.rand(batch, image, image, device="cuda", generator=g), torch.randn(batch, D, device="cuda", generator=g)
    with torch.no_grad():
        fwd = timeit(lambda: m(img, goal), iters)
    m.train()
    tgt = torch.randn(batch, D, device="cuda", generator=g)

    def step():
        for p in m.parameters():
            p.grad = None
        ((m(img, goal) - tgt) ** 2).mean().backward()
    step_ms = timeit(step, max(3, iters // 2))
    res = {"image": image, "patch": patch, "patch_pixels": patch * patch, "tokens": (image // patch) ** 2 + 1, "batch": batch,
           "forward": {"ms": round(fwd, 3), "frames_per_s": round(batch / fwd * 1e3, 1)},
           "fwd_bwd": {"ms": round(step_ms, 3), "frames_per_s": round(batch / step_ms * 1e3, 1)},
           "peak_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1)}
    print(json.dumps(res), flush=True)
    del m, img, goal, tgt
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=440)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="14,16", help="comma-separated: 14 (224x224 @ 14x14), 16 (256x256 @ 16x16)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    for c in a.configs.split(","):
        encoder(*CONFIGS[c], a.batch, a.iters)


if __name__ == "__main__":
    main()
