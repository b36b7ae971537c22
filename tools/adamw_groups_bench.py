#!/usr/bin/env python3
"""What parameter groups and a device-side schedule cost in the optimiser step.

    python tools/adamw_groups_bench.py [--rounds 5] [--only kernel|learn] [--out profiles/adamw_groups_ab.jsonl]

`kernel`: the Adam pass over ONE run of a flat buffer, event-timed at the C ABI, three forms
  (a) adam_step            dgvit_adam_step over the whole run (device step counter): the reference, a kernel this feature does not touch
  (b) adam_step_groups     dgvit_adam_step_groups with the run's real segment table (decoupled decay, cosine schedule)
  (c) adam_step_per_segment one dgvit_adam_step per segment: what groups would cost without the table
on three runs: the encoder run of a ViT-Base GoT (BASELINE config 5: 224x224, patch 16, dim 768, L12/H12, about 86 M parameters) grouped
by no_decay_groups; the encoder run of the shipped policy (GoTPolicy L4/H4/D64, 128x160) grouped the same way; one 4-float run.
`learn`: the shipped B = 32 SAC learn() step (tools/shipped_config.py) replayed as a HIP graph, FlatAdam(lr) against
FlatAdamW(no_decay_groups, warm-up + cosine LRSchedule) on both networks.
The forms are timed in turn, --rounds times over, in one process, so the run-to-run spread is seen beside the differences; one JSON line
per form with the per-round times, their median and range, printed and appended to --out.
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

HBM_PEAK_TB_S, HBM_MEASURED_TB_S = 8.0, 6.29     # MI355X: HBM3E specification; float4 copy as measured
BETAS, EPS = (0.9, 0.999), 1e-8


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


def _interleaved(forms, rounds):
    times = {name: [] for name, *_ in forms}
    for _ in range(rounds):
        for name, fn, iters, warmup in forms:
            times[name].append(_timed(fn, iters, warmup))
    return times


def _report(out, setting, forms, times, extra=None):
    for name, *_ in forms:
        t = times[name]
        row = {"setting": setting, "form": name, "ms_median": round(statistics.median(t), 5), "ms_min": round(min(t), 5),
               "ms_max": round(max(t), 5), "ms_rounds": [round(x, 5) for x in t]}
        row.update(extra or {})
        line = json.dumps(row)
        print(line, flush=True)
        if out:
            with open(out, "a") as f:
                f.write(line + "\n")


def _p(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset)


def _kernel_forms(lib, L, n, ends, groups, hyper_rows):
    """(a), (b), (c) over fresh buffers of n floats with the segment table (ends in float4 units, groups)"""
    import torch
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, g = torch.randn(n, device="cuda"), torch.randn(n, device="cuda") * 1e-3
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    end4 = torch.tensor(ends, dtype=torch.int64).cuda()
    group = torch.tensor(groups, dtype=torch.uint8).cuda()
    hyper = torch.tensor(hyper_rows, dtype=torch.float32, device="cuda")
    lr_out = torch.zeros(len(hyper_rows), device="cuda")
    step_dev = torch.full((1,), 10, dtype=torch.int64, device="cuda")
    starts = [0] + ends[:-1]

    def whole():
        L.check(lib.dgvit_adam_step(_p(p), _p(g), _p(m), _p(v), n, 1e-4, *BETAS, EPS, 0.0, 10, _p(step_dev), st), "dgvit_adam_step")

    def grouped():
        L.check(lib.dgvit_adam_step_groups(_p(p), _p(g), _p(m), _p(v), n, _p(end4), _p(group), len(ends), _p(hyper), len(hyper_rows),
                                           _p(lr_out), *BETAS, EPS, 1, 10, 10, _p(step_dev), 1, 5, 1000, 0.1, None, st),
                "dgvit_adam_step_groups")

    def per_segment():
        for s, e, gr in zip(starts, ends, groups):
            lr, wd = hyper_rows[gr]
            rc = lib.dgvit_adam_step(_p(p, 16 * s), _p(g, 16 * s), _p(m, 16 * s), _p(v, 16 * s), 4 * (e - s), lr, *BETAS, EPS, wd, 10,
                                     _p(step_dev), st)
            L.check(rc, "dgvit_adam_step")

    return [("a_adam_step", whole, 30, 5), ("b_adam_step_groups", grouped, 30, 5), ("c_adam_step_per_segment", per_segment, 10, 2)]


def _encoder_run(module, got):
    """(n, segment ends, segment groups) of the encoder run of `module`'s home with no_decay_groups(module, 0.05)"""
    from dgvit_amd import optim
    groups = optim.no_decay_groups(module, 0.05)
    group_of = {id(p): k for k, g in enumerate(groups) for p in g["params"]}
    home = optim.home_of(module)
    idx = [optim._HOME_OF[p][1] for p in got.param_table() if p is not None and p.requires_grad]
    assert idx == list(range(idx[0], idx[0] + len(idx))), "the encoder's trainable parameters are one stretch of the home"
    tab = optim._SegmentTable(home, idx, {i: group_of[id(home.params[i])] for i in idx})
    ends = tab.end4.cpu().tolist()
    return 4 * ends[-1], ends, tab.group.cpu().tolist()


def bench_kernel(args, lib, L):
    import torch
    import dgvit_amd
    hyper = [(1e-4, 0.05), (1e-4, 0.0)]
    vit = dgvit_amd.GoT(image_size=(224, 224), patch_size=(16, 16), num_classes=2, dim=768, depth=12, heads=12, mlp_dim=3072,
                        channels=1).to("cuda")
    shipped = dgvit_amd.GoTPolicy(2, 2, 4, 4, 64).to("cuda")
    runs = [("ViT-Base GoT encoder run", *_encoder_run(vit, vit)),
            ("shipped policy L4/H4/D64 encoder run", *_encoder_run(shipped, shipped.trans)),
            ("one 4-float run", 4, [1], [0])]
    for setting, n, ends, groups in runs:
        forms = _kernel_forms(lib, L, n, ends, groups, hyper)
        times = _interleaved(forms, args.rounds)
        _report(args.out, setting, forms, times,
                {"floats": n, "segments": len(ends), "floor_ms_at_peak_8.0_TB_s": round(28 * n / (HBM_PEAK_TB_S * 1e12) * 1e3, 5),
                 "floor_ms_at_measured_copy_6.29_TB_s": round(28 * n / (HBM_MEASURED_TB_S * 1e12) * 1e3, 5)})
        torch.cuda.empty_cache()


def bench_learn(args):
    import torch
    import dgvit_amd
    import synthetic
    from dgvit_amd.optim import FlatAdam, FlatAdamW, LRSchedule, flatten_parameters, no_decay_groups, soft_update
    B, alpha, gamma, tau = 32, 0.2, 0.99, 0.005
    torch.manual_seed(3407)
    pol0 = dgvit_amd.GoTPolicy(2, 2, 4, 4, 64).to("cuda")
    crt0 = dgvit_amd.QNetwork(2, 2).to("cuda")
    img, ps, act, _ = (t.to("cuda") for t in synthetic.make_inputs((128, 160), B, 1))
    nimg, nps, _, _ = (t.to("cuda") for t in synthetic.make_inputs((128, 160), B, 2))
    rew = torch.randn(B, 1, device="cuda")

    def make(adamw):
        pol, crt = copy.deepcopy(pol0), copy.deepcopy(crt0)
        tgt = copy.deepcopy(crt)
        flatten_parameters(pol), flatten_parameters(crt), flatten_parameters(tgt)
        if adamw:
            sched = LRSchedule("cosine", warmup_steps=100, total_steps=100000, final_ratio=0.1)
            op = FlatAdamW(no_decay_groups(pol, 0.05), lr=1e-3, capturable=True, schedule=sched)
            oc = FlatAdamW(no_decay_groups(crt, 0.05), lr=1e-3, capturable=True, schedule=sched)
        else:
            op, oc = FlatAdam([pol], lr=1e-3, capturable=True), FlatAdam([crt], lr=1e-3, capturable=True)

        def step():
            with torch.no_grad():
                na, nlogp, _ = pol.sample([nimg, nps])
                q1n, q2n = tgt([nimg, nps, na])
                y = rew + gamma * (torch.min(q1n, q2n) - alpha * nlogp)
            q1, q2 = crt([img, ps, act])
            qf = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
            oc.zero_grad(), qf.backward(), oc.step()
            pi, logp, _ = pol.sample([img, ps])
            q1p, q2p = crt([img, ps, pi])
            pl = (alpha * logp - torch.min(q1p, q2p)).mean()
            op.zero_grad(), oc.zero_grad(), pl.backward(), op.step()
            soft_update(tgt, crt, tau)
        graph = dgvit_amd.GraphedStep(step, warmup=3)
        return graph, {"optimizer_launches_policy": op.last_step_launches, "optimizer_launches_critic": oc.last_step_launches,
                       "groups_policy": len(op.param_groups)}

    ga, ia = make(False)
    gb, ib = make(True)
    forms = [("flat_adam", ga, 50, 10), ("flat_adamw_groups_schedule", gb, 50, 10)]
    times = _interleaved(forms, args.rounds)
    _report(args.out, "shipped SAC learn() B=32 as one HIP graph", forms[:1], times, ia)
    _report(args.out, "shipped SAC learn() B=32 as one HIP graph", forms[1:], times, ib)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["kernel", "learn"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adamw_groups_ab.jsonl"))
    args = ap.parse_args()
    import torch
    import dgvit_amd
    from dgvit_amd import _lib as L
    if not torch.cuda.is_available():
        raise SystemExit("adamw_groups_bench needs a ROCm device")
    lib = dgvit_amd.load_library()
    torch.manual_seed(3407)
    if args.only in (None, "kernel"):
        bench_kernel(args, lib, L)
    if args.only in (None, "learn"):
        bench_learn(args)


if __name__ == "__main__":
    main()
