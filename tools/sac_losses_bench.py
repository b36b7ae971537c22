#!/usr/bin/env python3
"""What the fused SAC loss head changes in the shipped learn() step.

    python tools/sac_losses_bench.py [--rounds 5] [--profile [--calls 10]] [--count KERNEL_TRACE.csv]

The step is bench.py's small_batch.learn / tools/shipped_config.py: GoT actor L4/H4/D64, CNN critic, 128x160, B = 32, FlatAdam(capturable),
timed eagerly and replayed as a HIP graph, in four forms that share inputs and initial weights:
  (a) torch_float_alpha      the loss arithmetic as torch expressions, alpha a Python float                       (the step as it was)
  (b) fused_float_alpha      sac_losses.critic_loss / actor_loss with alpha=
  (c) torch_learned_alpha    torch expressions with alpha = log_alpha.exp() and a torch-written temperature step, FlatAdam([log_alpha])
  (d) fused_learned_alpha    sac_losses with log_alpha= and target_entropy=, FlatAdam([log_alpha])
The forms are timed in turn, --rounds times over, so the round-to-round spread is seen beside the differences; one JSON line per form
and mode with the per-round times, their median and range.

--profile runs nothing but, per form, three warm-up steps, a marker kernel (torch.flip of a small tensor: no step launches one),
--calls eager steps and the marker again -- for `rocprofv3 --kernel-trace`, a run of its own.  --count reads that run's kernel trace and
prints the dispatches between each pair of markers divided by --calls: launches per step and form, and how many of them are this
library's loss kernels.
"""
import argparse
import copy
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORMS = ("a_torch_float_alpha", "b_fused_float_alpha", "c_torch_learned_alpha", "d_fused_learned_alpha")
B, ALPHA, GAMMA, TAU, TARGET_ENTROPY, ALPHA_LR = 32, 0.2, 0.99, 0.005, -2.0, 1e-2


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


def make_steps():
    """{form: step function}; every form has its own copies of the networks and optimisers, all start from the same weights"""
    import math
    import torch
    import dgvit_amd
    import synthetic
    from dgvit_amd import sac_losses as S
    from dgvit_amd.optim import FlatAdam, flatten_parameters, soft_update
    dev = "cuda"
    torch.manual_seed(3407)
    pol0, crt0 = dgvit_amd.GoTPolicy(2, 2, 4, 4, 64).to(dev), dgvit_amd.QNetwork(2, 2).to(dev)
    img, ps, act, _ = (t.to(dev) for t in synthetic.make_inputs((128, 160), B, 1))
    nimg, nps, _, _ = (t.to(dev) for t in synthetic.make_inputs((128, 160), B, 2))
    rew = torch.randn(B, 1, device=dev)
    steps = {}
    for form in FORMS:
        pol, crt = copy.deepcopy(pol0), copy.deepcopy(crt0)
        tgt = copy.deepcopy(crt)
        flatten_parameters(crt), flatten_parameters(tgt)
        op, oc = FlatAdam([pol], lr=1e-3, capturable=True), FlatAdam([crt], lr=1e-3, capturable=True)
        fused, learned = "fused" in form, "learned" in form
        log_alpha = torch.tensor([math.log(ALPHA)], device=dev, requires_grad=True) if learned else None
        ot = FlatAdam([log_alpha], lr=ALPHA_LR, capturable=True) if learned else None

        def step(pol=pol, crt=crt, tgt=tgt, op=op, oc=oc, ot=ot, log_alpha=log_alpha, fused=fused, learned=learned):
            temp = dict(log_alpha=log_alpha) if learned else dict(alpha=ALPHA)
            with torch.no_grad():
                na, nlogp, _ = pol.sample([nimg, nps])
                q1n, q2n = tgt([nimg, nps, na])
                if not fused:
                    alpha = log_alpha.exp() if learned else ALPHA
                    y = rew + GAMMA * (torch.min(q1n, q2n) - alpha * nlogp)
            q1, q2 = crt([img, ps, act])
            if fused:
                qf = S.critic_loss(q1, q2, rew, q1n, q2n, nlogp, gamma=GAMMA, **temp).loss
            else:
                qf = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
            oc.zero_grad(); qf.backward(); oc.step()
            pi, logp, _ = pol.sample([img, ps])
            q1p, q2p = crt([img, ps, pi])
            if fused:
                pl, al = S.actor_loss(logp, q1p, q2p, target_entropy=TARGET_ENTROPY if learned else None, **temp)
            else:
                alpha = log_alpha.detach().exp() if learned else ALPHA
                pl = (alpha * logp - torch.min(q1p, q2p)).mean()
                al = -(log_alpha * (logp.detach() + TARGET_ENTROPY).mean()).sum() if learned else None
            op.zero_grad(); oc.zero_grad(); pl.backward(); op.step()
            if learned:
                ot.zero_grad(); al.backward(); ot.step()
            soft_update(tgt, crt, TAU)
            return qf.detach(), pl.detach()

        steps[form] = step
    return steps


def count_launches(path, calls):
    """dispatches between each pair of markers in a rocprofv3 kernel trace, per step"""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    marks = [i for i, n in enumerate(names) if "flip" in n]
    if len(marks) != 2 * len(FORMS):
        raise SystemExit(f"{path}: expected {2 * len(FORMS)} marker dispatches, found {len(marks)}")
    for form, lo, hi in zip(FORMS, marks[0::2], marks[1::2]):
        inside = names[lo + 1:hi]
        ours = sum("sac_" in n for n in inside)
        print(json.dumps({"form": form, "calls": calls, "launches_per_step": len(inside) / calls, "sac_loss_kernels_per_step": ours / calls}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--count", metavar="KERNEL_TRACE.csv", default=None)
    args = ap.parse_args()
    if args.count:
        return count_launches(args.count, args.calls)
    import torch
    import dgvit_amd
    if not torch.cuda.is_available():
        raise SystemExit("sac_losses_bench needs a ROCm device")
    dgvit_amd.load_library()
    steps = make_steps()
    if args.profile:
        marker = torch.arange(8, device="cuda", dtype=torch.float32)
        for form, step in steps.items():
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            torch.flip(marker, [0])
            for _ in range(args.calls):
                step()
            torch.flip(marker, [0])
            torch.cuda.synchronize()
            print(json.dumps({"profiled": form, "calls": args.calls}), flush=True)
        return
    for mode in ("eager", "graph"):
        fns = {k: (v if mode == "eager" else dgvit_amd.GraphedStep(v, warmup=3)) for k, v in steps.items()}
        times = {k: [] for k in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                times[name].append(_timed(fn, 30, 5))
        for name, t in times.items():
            print(json.dumps({"setting": f"shipped learn() step, B={B}, {mode}", "form": name, "ms_median": round(statistics.median(t), 4),
                              "ms_min": round(min(t), 4), "ms_max": round(max(t), 4), "ms_rounds": [round(x, 4) for x in t]}), flush=True)


if __name__ == "__main__":
    main()
