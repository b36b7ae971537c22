#!/usr/bin/env python3
"""What gradient-norm clipping costs in the optimiser part of a step.

    python tools/grad_clip_bench.py [--rounds 5] [--only shipped|headline|kernel] [--profile]

After one forward + backward (the gradients then stay as they are) the optimiser part alone is event-timed, three forms:
  (a) FlatAdam.step()                                                    no clipping
  (b) torch.nn.utils.clip_grad_norm_(params, 10) then FlatAdam.step()    what a caller could write before
  (c) FlatAdam(max_grad_norm=10).step()                                  the norm, the coefficient and Adam's scaled read: 2 * runs + 1 launches
on the shipped policy (GoTPolicy L4/H4/D64, 128x160, B = 32; tools/shipped_config.py) eagerly and replayed as a HIP graph, and on the
headline dim-256 policy (84x84, patch 12, L6/H8; bench.py) the same way.  `kernel`: dgvit_grad_sqnorm_partials alone on a ViT-Base-sized
flat buffer (86 M floats) against its HBM floor, 4 B per element over the peak bandwidth.  The forms are timed in turn, --rounds times
over, so the run-to-run spread is seen beside the differences; one JSON line per form with the per-round times, their median and range.
--profile runs each form of the shipped policy a few times eagerly and nothing else (for a kernel trace: launches per form).
"""
import argparse
import copy
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

MAX_NORM = 10.0
HBM_PEAK_TB_S, HBM_MEASURED_TB_S = 8.0, 6.29     # MI355X: HBM3E specification; float4 copy as measured
VIT_BASE_FLOATS = 86_000_000 // 4 * 4


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


def _report(setting, forms, times, extra=None):
    for name, *_ in forms:
        t = times[name]
        row = {"setting": setting, "form": name, "ms_median": round(statistics.median(t), 5), "ms_min": round(min(t), 5),
               "ms_max": round(max(t), 5), "ms_rounds": [round(x, 5) for x in t]}
        row.update((extra or {}).get(name, {}))
        print(json.dumps(row), flush=True)


def _forms(make_policy, batch_inputs):
    """three copies of one policy with gradients from the same backward -> {(a), (b), (c)} optimiser parts and their launch counts"""
    import torch
    from dgvit_amd.optim import FlatAdam
    base = make_policy()
    out = {}
    for name, clip in (("a_flat_adam", None), ("b_torch_clip_then_flat_adam", None), ("c_flat_adam_max_grad_norm", MAX_NORM)):
        m = copy.deepcopy(base)
        opt = FlatAdam([m], lr=1e-3, capturable=True, max_grad_norm=clip)
        mean, log_std = m(batch_inputs)
        ((mean ** 2).mean() + (log_std ** 2).mean()).backward()
        params = [p for p in m.parameters() if p.grad is not None]
        runs = len(opt._runs())
        if name.startswith("b"):
            def fn(opt=opt, params=params):
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                opt.step()
            launches = None          # torch's multi-tensor kernels: counted in the kernel trace only
        else:
            fn = opt.step
            launches = runs + 1 if clip is None else 2 * runs + 1 + 1      # + the device-side step counter of capturable=True
        out[name] = (fn, {"tensors_with_grad": len(params), "adam_runs": runs, "launches_from_code": launches})
    return out


def _time_setting(setting, make_policy, inputs, rounds):
    import dgvit_amd
    forms = _forms(make_policy, inputs)
    for mode in ("eager", "graph"):
        fns = {k: (v[0] if mode == "eager" else dgvit_amd.GraphedStep(v[0], warmup=3)) for k, v in forms.items()}
        order = [(k, fns[k], 50, 10) for k in forms]
        times = {k: [] for k in forms}
        for _ in range(rounds):
            for name, fn, iters, warmup in order:
                times[name].append(_timed(fn, iters, warmup))
        _report(f"{setting}, {mode}", order, times, {k: v[1] for k, v in forms.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["shipped", "headline", "kernel"], default=None)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import torch
    import dgvit_amd
    import synthetic
    from dgvit_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench needs a ROCm device")
    lib = dgvit_amd.load_library()
    torch.manual_seed(3407)

    def shipped():
        return dgvit_amd.GoTPolicy(2, 2, 4, 4, 64).to("cuda")

    def headline():
        return dgvit_amd.GoTPolicy(2, 2, 6, 8, 256, image_size=(84, 84), patch_size=(12, 12)).to("cuda")

    def inputs(image, batch):
        img, ps, _, _ = (t.to("cuda") for t in synthetic.make_inputs(image, batch, 1))
        return [img, ps]

    if args.profile:
        for name, (fn, info) in _forms(shipped, inputs((128, 160), 32)).items():
            torch.cuda.synchronize()
            for _ in range(10):
                fn()
            torch.cuda.synchronize()
            print(json.dumps({"profiled": name, "calls": 10, **info}), flush=True)
        return
    if args.only in (None, "shipped"):
        _time_setting("shipped policy L4/H4/D64 128x160 B=32", shipped, inputs((128, 160), 32), args.rounds)
    if args.only in (None, "headline"):
        _time_setting("headline policy L6/H8/D256 84x84 B=32", headline, inputs((84, 84), 32), args.rounds)
    if args.only in (None, "kernel"):
        n = VIT_BASE_FLOATS
        g = torch.randn(n, device="cuda")
        scratch = torch.empty(L.GRAD_NORM_PARTIALS + 1, dtype=torch.float64, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731

        def norm():
            L.check(lib.dgvit_grad_sqnorm_partials(p(g), n, p(scratch), 0, st), "dgvit_grad_sqnorm_partials")

        def torch_norm():
            return torch.linalg.vector_norm(g)

        forms = [("kernel_grad_sqnorm_partials", norm, 50, 10), ("torch_vector_norm_same_buffer", torch_norm, 50, 10)]
        times = {name: [] for name, *_ in forms}
        for _ in range(args.rounds):
            for name, fn, iters, warmup in forms:
                times[name].append(_timed(fn, iters, warmup))
        extra = {name: {"floats": n, "partials": L.GRAD_NORM_PARTIALS,
                        "TB_per_s_at_median": round(4 * n / (statistics.median(times[name]) * 1e-3) / 1e12, 3),
                        "floor_ms_at_peak_8.0_TB_s": round(4 * n / (HBM_PEAK_TB_S * 1e12) * 1e3, 5),
                        "floor_ms_at_measured_copy_6.29_TB_s": round(4 * n / (HBM_MEASURED_TB_S * 1e12) * 1e3, 5)} for name, *_ in forms}
        _report("ViT-Base-sized flat buffer", forms, times, extra)


if __name__ == "__main__":
    main()
