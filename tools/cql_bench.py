#!/usr/bin/env python3
"""What Q for many actions per state and the CQL penalty cost.

    python tools/cql_bench.py [--rounds 3] [--only q,p] [--batches 32,256] [--out profiles/cql_bench.jsonl]

  (q) Q(s, a_m) for M = 30 actions per state on 128x160 frames, forward + backward, for the GoT critic (L4/H4/D64) and the CNN critic of
      the shipped configuration, at B = 32 and B = 256 states:
        a_q_many            critic.q_many([frames, pstate], actions): the encoder once on B frames, the head on B * M rows with the
                            feature pieces shared
        b_forward_repeated  critic([frames repeated M times, pstate repeated, actions]): the public route before q_many
        c_encoder_once_head_on_repeated
                            the encoder once, then the unshared head on feat.repeat_interleave(M, 0): what q_many saves beyond (b) is
                            the M-fold copy of the features and the sum of its gradient
  (p) sac_losses.cql_penalty forward + backward on (B, 30, 2) against the same formula in torch ops (logsumexp, mean, autograd).
Every form is timed eagerly and as a replayed HIP graph, the forms in turn, --rounds times over, with device events; one JSON line per
measurement with the per-round times, their median and range."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, M, A = 128, 160, 30, 2


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


def _compare(name, forms, rounds, iters, out, extra=None):
    """forms: {form: fn}; each timed eagerly and as a graph, in turn, rounds times"""
    import dgvit_amd
    graphs = {f: dgvit_amd.GraphedStep(fn, warmup=2) for f, fn in forms.items()}
    times = {(f, m): [] for f in forms for m in ("eager", "graph")}
    for _ in range(rounds):
        for f, fn in forms.items():
            times[(f, "eager")].append(_timed(fn, iters, 2))
            times[(f, "graph")].append(_timed(graphs[f], iters, 2))
    for (f, m), ts in times.items():
        line = dict(bench=name, form=f, mode=m, ms=[round(t, 5) for t in ts], median_ms=round(statistics.median(ts), 5),
                    range_ms=[round(min(ts), 5), round(max(ts), 5)], **(extra or {}))
        print(json.dumps(line), flush=True)
        if out:
            out.write(json.dumps(line) + "\n")
            out.flush()


def bench_q_many(rounds, batches, out):
    import torch
    import dgvit_amd
    from dgvit_amd.sac_networks import _head, _lin
    for kind in ("got", "cnn"):
        torch.manual_seed(3407)
        net = (dgvit_amd.GoTQNetwork(A, 2, 4, 4, 64) if kind == "got" else dgvit_amd.QNetwork(A, 2)).cuda().eval()
        towers = [(net.fc1, net.fc2, [net.fc3]), (net.fc11, net.fc21, [net.fc31])]
        for B in batches:
            g = torch.Generator().manual_seed(B)
            frames, pstate = torch.rand(B, H, W, generator=g).cuda(), torch.randn(B, 2, generator=g).cuda()
            actions = (torch.rand(B, M, A, generator=g) * 2 - 1).cuda()
            w1, w2 = torch.randn(B, M, A, generator=g).cuda(), torch.randn(B, M, A, generator=g).cuda()
            frames_m, pstate_m = frames.repeat_interleave(M, 0), pstate.repeat_interleave(M, 0)      # made once, outside the timing

            def finish(q1, q2):
                for p in net.parameters():
                    p.grad = None
                ((q1.reshape(B, M, A) * w1).sum() + (q2.reshape(B, M, A) * w2).sum()).backward()
                return q1, q2

            def q_many():
                return finish(*net.q_many([frames, pstate], actions))

            def forward_repeated():
                return finish(*net([frames_m, pstate_m, actions.view(B * M, A)]))

            def encoder_once_head_on_repeated():
                if kind == "got":
                    feat = net.trans(frames, _lin(net.fc_embed, pstate, relu=True))
                    pieces = [feat.view(B, -1).repeat_interleave(M, 0)]
                else:
                    pieces = [net._features(frames).repeat_interleave(M, 0), _lin(net.fc_embed, pstate, relu=True).repeat_interleave(M, 0)]
                (q1,), (q2,) = _head(pieces + [actions.view(B * M, A)], towers)
                return finish(q1, q2)

            # (checked without autograd: a backward on the default stream before the captures would leave AccumulateGrad nodes of that
            # stream alive, and a capture must not be made to run work there)
            with torch.no_grad():
                qa = net.q_many([frames, pstate], actions)[0]
                qb = net([frames_m, pstate_m, actions.view(B * M, A)])[0]
            assert torch.allclose(qa.reshape(B * M, A), qb, rtol=1e-4, atol=1e-5), "q_many and forward on repeated frames agree"
            del qa, qb
            forms = {"a_q_many": q_many, "b_forward_repeated": forward_repeated, "c_encoder_once_head_on_repeated": encoder_once_head_on_repeated}
            _compare(f"q_{kind}_B{B}_M{M}", forms, rounds, 10 if B * M <= 1024 else 4, out, dict(states=B, actions_per_state=M, critic=kind))


def bench_penalty(rounds, batches, out):
    import torch
    from dgvit_amd import sac_losses as S
    for B in batches:
        g = torch.Generator().manual_seed(B)
        qs = [torch.randn(*s, generator=g).cuda().requires_grad_(True) for s in ((B, M, A), (B, M, A), (B, A), (B, A))]
        log_w = torch.randn(B, M, generator=g).cuda()
        mask = (torch.rand(B, generator=g) < 0.75).cuda()

        def clear():
            for t in qs:
                t.grad = None

        def fused():
            clear()
            out_ = S.cql_penalty(*qs, log_w=log_w, temperature=1.0, weight=5.0, mask=mask)
            out_.loss.backward()
            return out_.loss, out_.gap, qs[0].grad

        def torch_ops():
            clear()
            m = mask.float()
            used = m.sum()
            gaps = []
            for qc, qd in ((qs[0], qs[2]), (qs[1], qs[3])):
                lse = torch.logsumexp(qc - log_w[:, :, None], dim=1)
                gaps.append((m[:, None] * (lse - qd)).sum() / (used * A).clamp(min=1.0))
            loss = 5.0 * (gaps[0] + gaps[1])
            loss.backward()
            return loss, torch.stack(gaps).detach(), qs[0].grad
        _compare(f"p_cql_penalty_B{B}_M{M}", {"cql_penalty": fused, "torch_ops": torch_ops}, rounds, 50, out, dict(states=B, actions_per_state=M))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default="q,p")
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cql_bench.jsonl"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a ROCm device"
    assert args.rounds >= 3, "at least 3 rounds: the result is a median and a range"
    batches = [int(b) for b in args.batches.split(",")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as sink:
        for key, fn in (("p", bench_penalty), ("q", bench_q_many)):
            if key in args.only.split(","):
                fn(args.rounds, batches, sink)
