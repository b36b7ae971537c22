#!/usr/bin/env python3
"""What the learning-from-demonstrations pieces cost and save.

    python tools/demo_bench.py [--rounds 3] [--only a,b,c] [--out FILE.jsonl]

  (a) replay.sample_mixed: 384 rows of a 100 000-slot ring + 128 rows of a 10 000-slot demonstration ring, 128x160 uint8 frames, plain and
      with frame_stack=4, random_shift=4, n_step=3 -- against the two sample() calls and a torch.cat per key.  The slots are given
      (persistent index tensors), so that both forms gather the same rows and the call can be captured.
  (b) functional.tanh_gaussian_log_prob, forward + backward at B = 32 and 512, A = 2 -- against the same formula written in torch ops.
  (c) the demonstration-regularised learn() step at B = 24 + 8 (tools/shipped_config.py's networks: GoT actor L4/H4/D64, CNN critic,
      128x160, FlatAdam(capturable)) with sac_losses.bc_loss -- against the same step with the term written in torch.
Every pair is timed eagerly and as a replayed HIP graph, the two forms in turn, --rounds times over, with device events; one JSON line
per measurement with the per-round times, their median and range.  (a) also states the bytes of frame traffic each form moves,
computed from the shapes."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 128, 160
COUNTS, SLOTS = (384, 128), (100_000, 10_000)


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


def _compare(name, forms, rounds, iters, extra=None, out=None):
    """forms: {form: fn}; each timed eagerly and as a graph, in turn, rounds times"""
    import dgvit_amd
    graphs = {f: dgvit_amd.GraphedStep(fn, warmup=2) for f, fn in forms.items()}
    times = {(f, m): [] for f in forms for m in ("eager", "graph")}
    for _ in range(rounds):
        for f, fn in forms.items():
            times[(f, "eager")].append(_timed(fn, iters, 3))
            times[(f, "graph")].append(_timed(graphs[f], iters, 3))
    for (f, m), ts in times.items():
        line = dict(bench=name, form=f, mode=m, ms=[round(t, 5) for t in ts], median_ms=round(statistics.median(ts), 5),
                    range_ms=[round(min(ts), 5), round(max(ts), 5)], **((extra or {}).get(f, {})))
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")


def bench_sample_mixed(rounds, out):
    import torch
    from dgvit_amd import replay
    rings = []
    for slots in SLOTS:
        ring = replay.DeviceReplayBuffer(slots, obs_shape=(H, W), frame_dtype=torch.uint8, seed=0)
        ring.track_episodes()
        for lo in range(0, slots, 5000):
            n = min(5000, slots - lo)
            ring.add_batch(obs=torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda"),
                           next_obs=torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda"), pobs=torch.randn(n, 2, device="cuda"),
                           next_pobs=torch.randn(n, 2, device="cuda"), act=torch.randn(n, 2, device="cuda"), rew=torch.randn(n, 1, device="cuda"),
                           done=(torch.rand(n, 1, device="cuda") < 0.01).float())
            ring.on_episode_end()
        rings.append(ring)
    idx = [torch.randint(0, s, (n,), device="cuda") for n, s in zip(COUNTS, SLOTS)]
    total = sum(COUNTS)
    for tag, kw, k in (("plain", dict(), 1), ("stack4_shift4_nstep3", dict(frame_stack=4, random_shift=4, n_step=3), 4)):
        def mixed():
            return replay.sample_mixed(list(zip(rings, COUNTS)), indices=idx, **kw)

        def two_and_cat():
            parts = [r.sample(n, indices=i, **kw) for r, n, i in zip(rings, COUNTS, idx)]
            return {key: torch.cat([p[key] for p in parts]) for key in parts[0]}
        a, b = mixed(), two_and_cat()
        assert all(torch.equal(a[key], b[key]) for key in b) or kw.get("random_shift"), "the two forms return the same batch"
        read, write = 2 * total * k * H * W, 2 * total * k * H * W * 4        # uint8 ring rows in, fp32 batch rows out, obs and next_obs
        extra = {"sample_mixed": dict(frame_bytes_read=read, frame_bytes_written=write),
                 "two_samples_and_cat": dict(frame_bytes_read=read + write, frame_bytes_written=2 * write)}
        _compare(f"a_sample_mixed_{tag}", {"sample_mixed": mixed, "two_samples_and_cat": two_and_cat}, rounds, 20, extra, out)


def bench_log_prob(rounds, out):
    import math
    import torch
    from dgvit_amd import functional as F
    for B in (32, 512):
        g = torch.Generator().manual_seed(B)
        mean, lsr = (torch.randn(B, 2, generator=g).cuda().requires_grad_(True) for _ in range(2))
        scale, bias = torch.tensor([1.0, 0.5]).cuda(), torch.tensor([0.0, 0.1]).cuda()
        action = torch.tanh(1.5 * torch.randn(B, 2, generator=g)).cuda() * scale + bias

        def fused():
            mean.grad = lsr.grad = None
            lp = F.tanh_gaussian_log_prob(mean, lsr, action, scale, bias, -20, 2)
            lp.sum().backward()
            return lp, mean.grad, lsr.grad

        def torch_ops():
            mean.grad = lsr.grad = None
            y = ((action - bias) / scale).clamp(-(1 - 1e-6), 1 - 1e-6)
            x = 0.5 * torch.log((1 + y) / (1 - y))
            ls = lsr.clamp(-20, 2)
            e = (x - mean) * torch.exp(-ls)
            lp = (-0.5 * e * e - ls - 0.5 * math.log(2 * math.pi) - torch.log(scale * (1 - y * y) + 1e-6)).sum(1, keepdim=True)
            lp.sum().backward()
            return lp, mean.grad, lsr.grad
        _compare(f"b_log_prob_B{B}", {"fused": fused, "torch_ops": torch_ops}, rounds, 50, None, out)


def bench_learn(rounds, out):
    import torch
    import dgvit_amd
    from dgvit_amd import replay, sac_losses as S
    from dgvit_amd.optim import FlatAdam, soft_update
    counts, alpha, gamma, tau, lam = (24, 8), 0.2, 0.99, 0.005, 0.5
    torch.manual_seed(3407)
    pol0, crt0 = dgvit_amd.GoTPolicy(2, 2, 4, 4, 64).cuda(), dgvit_amd.QNetwork(2, 2).cuda()
    rings = []
    for slots in (256, 64):
        ring = replay.DeviceReplayBuffer(slots, obs_shape=(H, W), frame_dtype=torch.uint8, seed=0)
        ring.add_batch(obs=torch.randint(0, 256, (slots, H, W), dtype=torch.uint8, device="cuda"),
                       next_obs=torch.randint(0, 256, (slots, H, W), dtype=torch.uint8, device="cuda"), pobs=torch.randn(slots, 2, device="cuda"),
                       next_pobs=torch.randn(slots, 2, device="cuda"), act=torch.rand(slots, 2, device="cuda") * 2 - 1, rew=torch.randn(slots, 1, device="cuda"),
                       done=torch.zeros(slots, 1, device="cuda"))
        rings.append(ring)
    idx = [torch.randint(0, r.size, (n,), device="cuda") for r, n in zip(rings, counts)]

    def make(fused):
        pol, crt = copy.deepcopy(pol0), copy.deepcopy(crt0)
        tgt = copy.deepcopy(crt)
        op, oc = FlatAdam([pol], lr=1e-4, capturable=True), FlatAdam([crt], lr=1e-4, capturable=True)

        def learn():
            b = replay.sample_mixed(list(zip(rings, counts)), indices=idx)
            with torch.no_grad():
                na, nlogp, _ = pol.sample([b["next_obs"], b["next_pobs"]])
                q1n, q2n = tgt([b["next_obs"], b["next_pobs"], na])
            q1, q2 = crt([b["obs"], b["pobs"], b["act"]])
            c = S.critic_loss(q1, q2, b["rew"], q1n, q2n, nlogp, alpha=alpha, gamma=gamma)
            oc.zero_grad(); c.loss.backward(); oc.step()
            pi, logp, _ = pol.sample([b["obs"], b["pobs"]])
            q1p, q2p = crt([b["obs"], b["pobs"], pi])
            if fused:
                bc = S.bc_loss(pi, b["act"], mask=b["source"] == 1).loss
            else:
                m = (b["source"] == 1).float()
                used = m.sum()
                bc = torch.where(used > 0, (m * ((pi - b["act"]) ** 2).mean(1)).sum() / used.clamp(min=1.0), torch.zeros_like(used))
            pl = S.actor_loss(logp, q1p, q2p, alpha=alpha).policy_loss + lam * bc
            op.zero_grad(); oc.zero_grad(); pl.backward(); op.step()
            soft_update(tgt, crt, tau)
            return c.loss.detach(), pl.detach()
        return learn
    _compare("c_learn_step_B32", {"bc_loss_fused": make(True), "bc_term_in_torch": make(False)}, rounds, 10, None, out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a ROCm device"
    sink = open(args.out, "w") if args.out else None
    for key, fn in (("a", bench_sample_mixed), ("b", bench_log_prob), ("c", bench_learn)):
        if key in args.only.split(","):
            fn(args.rounds, sink)
    if sink:
        sink.close()
