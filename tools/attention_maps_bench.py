"""Cost of the attention maps: the no-grad forward against GoT.attention_maps(rows='goal') and rows='all' (torch events, warm-up first).

    python tools/attention_maps_bench.py [--iters 20] [--shapes c3,c5_bf16,shipped_b1]

Shapes: BASELINE config 3 (B = 512, 84x84 @ 12, D 256, L 6, H 8), the C5 bf16 shape at B = 64 (224x224 @ 16, ViT-Base) and the
shipped actor at B = 1.  One JSON line per shape (milliseconds per call, medians of --iters timed calls)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import dgvit_amd  # noqa: E402

SHAPES = {
    "c3": dict(image=(84, 84), patch=(12, 12), dim=256, depth=6, heads=8, mlp_dim=2048, B=512, bf16=False),
    "c5_bf16": dict(image=(224, 224), patch=(16, 16), dim=768, depth=12, heads=12, mlp_dim=3072, B=64, bf16=True),
    "shipped_b1": dict(image=(128, 160), patch=(16, 20), dim=64, depth=4, heads=4, mlp_dim=2048, B=1, bf16=False),
}


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    torch.manual_seed(0)
    for name in args.shapes.split(","):
        s = SHAPES[name]
        m = dgvit_amd.GoT(image_size=s["image"], patch_size=s["patch"], num_classes=2, dim=s["dim"], depth=s["depth"], heads=s["heads"],
                          mlp_dim=s["mlp_dim"], channels=1).cuda().eval()
        if s["bf16"]:
            m.set_compute_dtype(torch.bfloat16).freeze_bf16_weights()
        img = torch.rand(s["B"], *s["image"], device="cuda")
        goal = torch.randn(s["B"], s["dim"], device="cuda")
        with torch.no_grad():
            fwd = _time(lambda: m(img, goal), args.iters)
        goal_ms = _time(lambda: m.attention_maps(img, goal, rows="goal"), args.iters)
        all_ms = _time(lambda: m.attention_maps(img, goal, rows="all"), args.iters)
        print(json.dumps({"shape": name, "B": s["B"], "forward_ms": round(fwd, 4), "maps_goal_ms": round(goal_ms, 4),
                          "maps_all_ms": round(all_ms, 4), "goal_overhead": round(goal_ms / fwd - 1, 4),
                          "all_overhead": round(all_ms / fwd - 1, 4)}), flush=True)


if __name__ == "__main__":
    main()
