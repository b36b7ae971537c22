#!/usr/bin/env python3
"""What the CNN feature stack costs on frame stacks: cnn_features on (B, 128, 160, K) against torch's convolutions.

    python tools/cnn_stack_bench.py [--rounds 5] [--parent-lib libdgvit_hip.so] [--kernel-trace kernel_trace.csv]
                                    [--out profiles/cnn_stack_bench.jsonl]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/cnn_stack_bench.py --trace-run

128x160 frames, K in {1, 4} frames per stack, B in {32, 512}.  Per shape, form by form and --rounds times over, measured in turn on the
same inputs (device events around `iters` calls after a warm-up):
  hip_fwd        functional.cnn_features under no_grad
  hip_fwd_bwd    ... and the backward for the six conv parameters (the critic's training step: the stack is data, no frame gradient)
  torch_fwd      the same stack through torch.nn.functional.conv2d on the device (stack.permute(0, 3, 1, 2): a channels-last
  torch_fwd_bwd  input, no copy), relu, mean -- the outside reference
and for K = 1, with --parent-lib (the library built from the parent commit), dgvit_cnn_forward / dgvit_cnn_backward_v2 of both libraries
on the raw ABI in turn:
  this_raw_fwd, this_raw_fwd_bwd, parent_raw_fwd, parent_raw_fwd_bwd
One JSON line per form with the per-round times, their median and their range.

--trace-run runs conv1's two im2col kernels for a profiler and times nothing: the backward at B = 512 for K = 3 (im2col_cn_kernel, rows
of 76 floats, 75 real) and K = 4 (im2col_c4_kernel, rows of 100 floats).  --kernel-trace takes the profiler's per-dispatch CSV of such a
run and adds one line per kernel: the median kernel time over conv1's dispatches and the bytes per second over the bytes the pass needs
(the stack read once + the column matrix written once)."""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 128, 160
SHAPES = [(1, 32), (4, 32), (1, 512), (4, 512)]          # (K, B)
TRACE = [(3, 512), (4, 512)]
OLD = ["dgvit_cnn_workspace_floats", "dgvit_cnn_forward_scratch_floats", "dgvit_cnn_backward_scratch_floats", "dgvit_cnn_forward",
       "dgvit_cnn_backward_v2"]


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


def _al4(n):
    return (n + 3) & ~3


def im2col_bytes(K, B):
    """bytes conv1's im2col needs: the (B, H, W, K) stack read once, the M1 x KP column matrix written once"""
    m1 = B * ((H - 5) // 2 + 1) * ((W - 5) // 2 + 1)
    kp = 28 if K == 1 else _al4(25 * K)
    return 4 * (B * H * W * K + m1 * kp), m1, kp


def _params(K, dev, grad):
    import torch
    g = torch.Generator().manual_seed(K)
    shapes = [(16, K, 5, 5), (16,), (64, 16, 5, 5), (64,), (256, 64, 5, 5), (256,)]
    return [(torch.randn(s, generator=g) * (0.05 if len(s) == 4 else 0.01)).to(dev).requires_grad_(grad) for s in shapes]


def _raw(lib, img, params):
    """(forward, forward + backward) of the single-frame entry points of `lib` on preallocated buffers"""
    import torch
    B = img.shape[0]
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = lambda ts: (ctypes.c_void_p * 6)(*[t.data_ptr() for t in ts])     # noqa: E731
    nws, nf, nb = lib.dgvit_cnn_workspace_floats(B, H, W), lib.dgvit_cnn_forward_scratch_floats(B, H, W), lib.dgvit_cnn_backward_scratch_floats(B, H, W)
    ws, sc = torch.empty(nws, device="cuda"), torch.empty(max(nf, nb), device="cuda")
    feat, dfeat = torch.empty(B, 256, device="cuda"), torch.full((B, 256), 1.0 / B, device="cuda")
    grads = [torch.empty_like(p) for p in params]
    pt, gt = table(params), table(grads)

    def fwd():
        rc = lib.dgvit_cnn_forward(P(img), pt, P(feat), P(ws), nws, P(sc), nf, B, H, W, st)
        assert rc == 0, rc

    def fwd_bwd():
        fwd()
        rc = lib.dgvit_cnn_backward_v2(P(img), pt, gt, P(dfeat), None, P(ws), nws, P(sc), nb, B, H, W, st)
        assert rc == 0, rc
    return fwd, fwd_bwd


def _load_parent(path):
    from dgvit_amd import _lib as L
    lib = ctypes.CDLL(os.path.abspath(path))
    for name in OLD:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return lib


def _trace_rows(path):
    """one line per conv1 im2col kernel of a --trace-run, from the profiler's per-dispatch CSV"""
    want = {}
    for K, B in TRACE:
        nbytes, m1, kp = im2col_bytes(K, B)
        name = "im2col_c4_kernel" if K % 4 == 0 else "im2col_cn_kernel"
        threads = -(-(m1 * kp // 4) // 256) * 256
        want[name] = dict(K=K, B=B, bytes=nbytes, kp=kp, threads=threads, ns=[])
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for name, w in want.items():
                grid = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)
                if name in row["Kernel_Name"] and grid in (w["threads"], w["threads"] // 256):       # conv2 / conv3 take im2col_c4_kernel too: another grid
                    w["ns"].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    out = []
    for name, w in want.items():
        if not w["ns"]:
            raise SystemExit(f"no {name} dispatch of {w['threads']} threads in {path}")
        ns = [d for _, d in sorted(w["ns"])][len(w["ns"]) // 5:]          # the first dispatches load code objects and fault pages in
        med = statistics.median(ns)
        out.append(dict(form="kernel_" + name, frames=w["K"], batch=w["B"], row_floats=w["kp"], dispatches=len(w["ns"]), bytes_moved=w["bytes"],
                        us_median=round(med / 1e3, 2), us_min=round(min(ns) / 1e3, 2), us_max=round(max(ns) / 1e3, 2),
                        gb_per_s_median=round(w["bytes"] / med, 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libdgvit_hip.so built from the parent commit: the K = 1 comparison")
    ap.add_argument("--kernel-trace", default=None, help="per-dispatch CSV of a --trace-run under the profiler")
    ap.add_argument("--trace-run", action="store_true", help="run conv1's im2col kernels for a profiler and write nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_stack_bench.jsonl"))
    args = ap.parse_args()
    import torch
    import dgvit_amd
    from dgvit_amd import functional as F
    if not torch.cuda.is_available():
        raise SystemExit("cnn_stack_bench needs a ROCm device")
    lib = dgvit_amd.load_library()
    conv2d, lines = torch.nn.functional.conv2d, []

    def emit(**row):
        line = json.dumps({"frame": [H, W], **row})
        print(line, flush=True)
        lines.append(line)

    def stack_of(K, B):
        g = torch.Generator(device="cuda").manual_seed(B + K)
        return torch.rand((B, H, W) if K == 1 else (B, H, W, K), device="cuda", generator=g)

    if args.trace_run:
        for K, B in TRACE:
            x, params = stack_of(K, B), _params(K, "cuda", True)
            for _ in range(12):
                F.cnn_features(x, params).mean().backward()
            torch.cuda.synchronize()
            del x, params
            torch.cuda.empty_cache()
        return

    for K, B in SHAPES:
        x = stack_of(K, B)
        params, tparams = _params(K, "cuda", True), _params(K, "cuda", True)
        nchw = x.unsqueeze(1) if K == 1 else x.permute(0, 3, 1, 2)

        def hip_fwd():
            with torch.no_grad():
                return F.cnn_features(x, params)

        def hip_fwd_bwd():
            for p in params:
                p.grad = None
            F.cnn_features(x, params).mean().backward()

        def torch_feat():
            h = nchw
            for i in range(3):
                h = torch.relu(conv2d(h, tparams[2 * i], tparams[2 * i + 1], stride=2))
            return h.mean(dim=(2, 3))

        def torch_fwd():
            with torch.no_grad():
                return torch_feat()

        def torch_fwd_bwd():
            for p in tparams:
                p.grad = None
            torch_feat().mean().backward()

        err = float((hip_fwd() - torch_fwd()).abs().max())        # the two routes compute the same thing
        assert err < 1e-4, err
        iters, warmup = (200, 20) if B <= 32 else (20, 3)
        forms = [("hip_fwd", hip_fwd), ("torch_fwd", torch_fwd), ("hip_fwd_bwd", hip_fwd_bwd), ("torch_fwd_bwd", torch_fwd_bwd)]
        if K == 1 and args.parent_lib:
            raw = [t.detach() for t in params]
            tf, tfb = _raw(lib, x, raw)
            pf, pfb = _raw(_load_parent(args.parent_lib), x, raw)
            forms += [("this_raw_fwd", tf), ("parent_raw_fwd", pf), ("this_raw_fwd_bwd", tfb), ("parent_raw_fwd_bwd", pfb)]
        times = {name: [] for name, _ in forms}
        for _ in range(args.rounds):
            for name, fn in forms:
                times[name].append(_timed(fn, iters, warmup))
        for name, _ in forms:
            t = times[name]
            emit(form=name, frames=K, batch=B, iters=iters, ms_median=round(statistics.median(t), 4), ms_min=round(min(t), 4),
                 ms_max=round(max(t), 4), ms_rounds=[round(v, 4) for v in t], max_abs_vs_torch=err)
        del x, nchw, params, tparams, forms
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for rows in ([], _trace_rows(args.kernel_trace) if args.kernel_trace else None):      # the timings are on disk before the CSV is read
        if rows is None:
            break
        for row in rows:
            emit(**row)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
