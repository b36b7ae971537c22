"""GPU: several SAC learn() steps of the HIP networks -- bench.py's small_batch.learn(), step for step -- followed against the float64
learner of tests/sac_trajectory_ref.py.  What only matters from the second update on is under test here: Adam's moments and its host or
device step counter, the flat gradient buffers the fused backward writes and FlatAdam consumes in place (the critic's gradients of the
actor loss are dropped, not accumulated), the target after soft_update, workspaces reused by five forwards per step, the clip
coefficient left on the device, and the sum tree's leaves after update_priorities.

Every case is judged by the rule of sac_trajectory_ref (its docstring): |hip - ref64| per quantity against MARGIN = 4 times the distance of
the reference's own fp32 run from its fp64 run, computed here for the same case; nothing of the rule comes from the HIP side.  The N(0, 1)
draws are injected through sac_networks._standard_normal (two preallocated device buffers, refilled before each step); modules are in
eval mode (the embedding dropout's mask cannot be injected).  The defects this catches, and by how much: test_sac_trajectory_host.py.

Measured hip / yardstick on an MI355X (each case prints its table):
  case (largest ratio first)                        qf    pl    actor med / p99.9   critic med / p99.9   target med / p99.9
  1 shipped pairing, eager                          0.67  0.88  0.99 / 1.00         0.99 / 1.00          0.86 / 0.87
  2 transformer critic, eager                       1.33  0.96  1.00 / 1.00         1.10 / 1.00          0.99 / 0.86
  3 clipped                                         0.98  1.02  0.98 / 1.00         0.95 / 0.99          0.84 / 0.87
  4 captured from step 2                            1.53  0.60  1.01 / 1.00         1.14 / 0.99          0.93 / 0.86
  5 benchmarked step, captured from step 1          1.13  1.00  1.03 / 0.99         1.12 / 0.99          0.86 / 0.83
  6 prioritized, shifted (teacher-forced)           3.30  1.00  1.00 / 1.00         1.04 / 1.21          0.88 / 0.97
No element of any network is more than 0.1 lr from the fp64 run in any case (largest |delta| 7.1e-6).  Case 3: the gradient norms the
device leaves behind are within 4.4e-6 relative of the reference's.  Case 6: weights within 9.0e-7 relative (bound 1e-5), leaves within
0.036 of their bound.  The last-block fold is taken in every case (B = 37 at 50 tokens and B = 32 at 65 tokens, dim 64).

What the captured cases found: before the library's zero fills became a kernel (csrc/common.h zero_fill), cases 4 and 5
failed from the first replay on -- qf 7e4 and pl 2e5 times the yardstick, 66 % of the actor's and 58 % of the critic's elements more than
0.1 lr off, Adam moments of 1e10: hipMemsetAsync recorded into the graph did not clear the split-K arrival counters on replay, the
in-launch split-K GEMMs of the backward never wrote their tiles, and FlatAdam consumed uninitialised gradient memory.  Eager steps,
capturable or not, were exact throughout, also on deliberately dirtied allocator blocks.
"""
import contextlib
import copy
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O  # noqa: E402
import sac_trajectory_ref as T  # noqa: E402

CFG, B, K, LR, SEED, KW = T.BASE_CFG, T.BASE_B, T.BASE_K, T.BASE_LR, T.BASE_SEED, T.BASE_KW
# what bench.py's shipped_learn_step_ms.hip_graph times: GoTPolicy(2, 2, 4, 4, 64) on 128 x 160 frames with the CNN critic at batch 32
# (one 32-row block of the head kernels: the direct-write path); the same seed keeps the reference's fp32 run at rounding distance here too
SHIPPED_CFG, SHIPPED_B, SHIPPED_K = O.GoTConfig(image=(128, 160), patch=(16, 20), dim=64, depth=4, heads=4), 32, 4
PER = dict(alpha=0.6, eps=1e-4, beta=0.4, pad=4, size=100, stored=80)


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


_REFS, _HIP = {}, {}


def _reference(name, case, **kw):
    """(fp64 run, fp32 run, yardstick) of a case, computed once; the yardstick must meet the cap on its own"""
    if name not in _REFS:
        r64, r32 = T.run(case, torch.float64, **KW, **kw), T.run(case, torch.float32, **KW, **kw)
        _REFS[name] = (r64, r32, T.distance(r32, r64, LR))
    r64, r32, Y = _REFS[name]
    assert T.cap_violations(Y, len(case["steps"]), LR) == [], "the reference's own fp32 run breaks the cap: the case is ill-conditioned"
    return r64, r32, Y


def _case(critic="cnn"):
    key = ("case", critic)
    if key not in _REFS:
        _REFS[key] = T.make_case(CFG, B, K, SEED, critic)
    return _REFS[key]


def _load_state(module, params):
    module.load_state_dict(dict(params), strict=True)
    return module.cuda().eval()


class _Draws:
    """stands in for sac_networks._standard_normal: hands out two preallocated device buffers in turn (e1 for the next action, e2 for the
    actor sample), which the test refills before each step"""

    def __init__(self, batch):
        self.bufs = [torch.zeros(batch, 2, device="cuda") for _ in range(2)]
        self.calls = 0

    def __call__(self, like):
        buf = self.bufs[self.calls % 2]
        self.calls += 1
        assert like.shape == buf.shape and like.device == buf.device
        return buf


@contextlib.contextmanager
def _injected(batch):
    import dgvit_amd.sac_networks as S
    draws = _Draws(batch)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(S, "_standard_normal", draws)
        yield draws


def _folds(amd, pol, batch):
    from dgvit_amd._lib import dgvit_config
    return amd.load_library().dgvit_got_last_block_folds(ctypes.byref(dgvit_config(*pol.trans._cfg)), batch, 1.0, 0)


def _hip_run(amd, case, mode="eager", max_grad_norm=None, eager_steps=2, per=None, capturable=None, probe=None):
    """The K steps of ``case`` on the device, in bench.py's order.  mode "captured": FlatAdam(capturable=True); steps 0 .. eager_steps - 1 run
    eagerly, GraphedStep(fn, warmup=1) makes its warm-up call the next step and the rest are replays, the static inputs refilled before each.
    ``per``: the prioritized, shifted loop -- each step samples its batch from a PrioritizedDeviceReplayBuffer with uploaded uniforms, weighs
    the critic loss and writes |q1 - y|.mean(1) back; the indices, shifts and weights drawn and the leaves after each write-back are recorded
    into ``per`` / the result.  ``capturable`` overrides FlatAdam's flag (default: the mode's); ``probe(k, pol, crt, tgt, op, oc)`` is
    called after step k has finished -- for finding which component carries a difference.  Returns what sac_trajectory_ref.run returns,
    on the CPU."""
    from dgvit_amd.optim import FlatAdam, soft_update
    cfg, nsteps, batch = case["cfg"], len(case["steps"]), case["batch"]
    alpha, gamma, tau = KW["alpha"], KW["gamma"], KW["tau"]
    kw = dict(image_size=cfg.image, patch_size=cfg.patch)
    pol = _load_state(amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, **kw), case["actor"])
    crt = amd.QNetwork(2, 2) if case["critic"] == "cnn" else amd.GoTQNetwork(2, 2, cfg.depth, cfg.heads, cfg.dim, **kw)
    crt = _load_state(crt, case["critic_params"])
    tgt = copy.deepcopy(crt)
    captured = mode == "captured"
    capturable = captured if capturable is None else capturable
    mgn_a, mgn_c = (None, None) if max_grad_norm is None else max_grad_norm
    op = FlatAdam([pol], lr=LR, capturable=capturable, max_grad_norm=mgn_a)
    oc = FlatAdam([crt], lr=LR, capturable=capturable, max_grad_norm=mgn_c)
    fields = ("obs", "pobs", "act", "rew", "next_obs", "next_pobs")
    X = {f: torch.zeros_like(case["steps"][0][f], device="cuda") for f in fields}
    out = dict(qf=[], pl=[], td=[], weights=[], leaves=[], gnorm_actor=[], gnorm_critic=[], folds=_folds(amd, pol, batch))
    buf = None
    if per is not None:
        from dgvit_amd.replay import PrioritizedDeviceReplayBuffer
        buf = PrioritizedDeviceReplayBuffer(per["size"], obs_shape=cfg.image, seed=0, alpha=per["alpha"], eps=per["eps"])
        buf.add_batch(**per["store"])
        n = per["stored"]
        buf.update_priorities(torch.arange(n), torch.from_numpy(per["priorities"]).cuda())
        assert buf.get_stored_size() == n and len(buf._levels) == 2, "a two-level tree"
        uniforms = torch.zeros(batch, device="cuda")

    with _injected(batch) as draws:
        def fill(k):
            s = case["steps"][k]
            if per is None:
                for f in fields:
                    X[f].copy_(s[f])
            draws.bufs[0].copy_(s["e1"])
            draws.bufs[1].copy_(s["e2"])

        def learn():
            w, b = None, X
            if per is not None:
                b = buf.sample(batch, beta=per["beta"], random_shift=per["pad"], return_shifts=True, uniforms=uniforms)
                w = b["weights"]
            with torch.no_grad():
                na, nlogp, _ = pol.sample([b["next_obs"], b["next_pobs"]])
                q1n, q2n = tgt([b["next_obs"], b["next_pobs"], na])
                y = b["rew"] + gamma * (torch.min(q1n, q2n) - alpha * nlogp)
            q1, q2 = crt([b["obs"], b["pobs"], b["act"]])
            if w is None:
                qf = torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y)
            else:
                qf = (w * (q1 - y) ** 2).mean() + (w * (q2 - y) ** 2).mean()
            oc.zero_grad(); qf.backward(); oc.step()
            pi, logp, _ = pol.sample([b["obs"], b["pobs"]])
            q1p, q2p = crt([b["obs"], b["pobs"], pi])
            pl = (alpha * logp - torch.min(q1p, q2p)).mean()
            op.zero_grad(); oc.zero_grad(); pl.backward(); op.step()
            soft_update(tgt, crt, tau)
            td = (q1 - y).abs().detach()
            if per is not None:
                buf.update_priorities(b["indexes"], td.mean(1))
            return dict(qf=qf.detach(), pl=pl.detach(), td=td, batch=b if per is not None else None)

        def record(o):
            torch.cuda.synchronize()
            if probe is not None:
                probe(len(out["qf"]), pol, crt, tgt, op, oc)
            out["qf"].append(float(o["qf"].double())), out["pl"].append(float(o["pl"].double())), out["td"].append(o["td"].cpu().clone())
            for name, opt in (("gnorm_actor", op), ("gnorm_critic", oc)):
                out[name].append(None if opt.last_grad_norm is None else float(opt.last_grad_norm))
            if per is not None:
                b = o["batch"]
                per["idx"].append(b["indexes"].cpu().numpy()), per["obs_shift"].append(b["obs_shift"].cpu().numpy())
                per["next_obs_shift"].append(b["next_obs_shift"].cpu().numpy())
                out["weights"].append(b["weights"][:, 0].cpu().numpy().astype(np.float64))
                out["leaves"].append(buf.priorities().cpu().numpy().astype(np.float64))

        def before(k):
            fill(k)
            if per is not None:
                uniforms.copy_(torch.from_numpy(per["uniforms"][k]))
                torch.manual_seed(SEED + k)          # the seed of the step's shifts comes from torch's CPU generator

        if not captured:
            for k in range(nsteps):
                before(k)
                record(learn())
        else:
            for k in range(eager_steps):
                before(k)
                record(learn())
            calls = []
            before(eager_steps)
            graph = amd.GraphedStep(lambda: calls.append(learn()) or calls[-1], warmup=1)
            assert len(calls) == 2, "one warm-up call, which ran the step, and the capture, which ran nothing"
            record(calls[0])
            for k in range(eager_steps + 1, nsteps):
                before(k)
                record(graph())
        assert draws.calls > 0 and draws.calls % 2 == 0, "every step drew twice: e1 for the next action, e2 for the actor sample"
    for net, m in (("actor", pol), ("critic", crt), ("target", tgt)):
        out[net] = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return out


def _judge(title, hip, case, ref, margins=None):
    r64, r32, Y = ref
    nsteps = len(case["steps"])
    d = T.distance(hip, r64, LR)
    r, bad = T.check(d, Y, nsteps, LR, margins=margins)
    print(T.report(f"{title} (last-block fold taken: {hip['folds']})", d, Y, r))
    for name in ("qf", "pl"):
        print(f"  {name} per step, relative to the fp64 run:", " ".join(f"{abs(a - b) / abs(b):.2e}" for a, b in zip(hip[name], r64[name])))
    print("  |q1 - y|: largest difference from the fp64 run", max(float((a.double() - b).abs().max()) for a, b in zip(hip["td"], r64["td"])),
          "fp32 reference run's", max(float((a.double() - b).abs().max()) for a, b in zip(r32["td"], r64["td"])))
    assert not bad, "\n".join(bad)
    # parameters that never receive a gradient are untouched, bit for bit
    for net, init in (("actor", case["actor"]), ("critic", case["critic_params"])):
        assert r64["untouched"][net] or net == "critic"
        for k in r64["untouched"][net]:
            assert torch.equal(hip[net][k], init[k]), (net, k)
    return r


def _eager_base(amd):
    if "eager" not in _HIP:
        _HIP["eager"] = _hip_run(amd, _case())
    return _HIP["eager"]


def test_shipped_pairing_eager(amd):
    """GoTPolicy and the CNN QNetwork; B = 37 spans two 32-row blocks of the head kernels (the partial-sum path)"""
    case = _case()
    _judge("GoT actor + CNN critic, eager", _eager_base(amd), case, _reference("cnn", case))


def test_transformer_critic_eager(amd):
    """GoTPolicy and GoTQNetwork, the pairing bench.py's sac_step times; the critic's dead conv1-3 never move"""
    case = _case("got")
    _judge("GoT actor + GoT critic, eager", _hip_run(amd, case), case, _reference("got", case))


def test_clipped(amd):
    """FlatAdam(max_grad_norm=...) on both networks, each threshold half the smallest gradient norm of the unclipped fp64 run (the host test
    shows that this clips at every step); the norm the device leaves behind is the reference's"""
    case = _case()
    unclipped, _, _ = _reference("cnn", case)
    mgn = T.clip_norms(unclipped)
    ref = _reference("clipped", case, max_grad_norm=mgn)
    r64 = ref[0]
    assert all(c < 1 for c in r64["coef_actor"] + r64["coef_critic"])
    hip = _hip_run(amd, case, max_grad_norm=mgn)
    _judge("GoT actor + CNN critic, clipped", hip, case, ref)
    for name in ("gnorm_actor", "gnorm_critic"):
        print(f"  {name}: largest relative difference", max(abs(a / b - 1) for a, b in zip(hip[name], r64[name])))
        np.testing.assert_allclose(hip[name], r64[name], rtol=1e-4)     # (the parity tests' bound on outputs; here on a norm of gradients)


def test_captured(amd):
    """capturable=True: steps 0 and 1 eager, step 2 GraphedStep's warm-up call, steps 3 to 5 replays.  Against the reference as every case,
    and against the eager run at the bounds of test_gpu_parity.py::test_graphed_training_step."""
    case = _case()
    hip = _hip_run(amd, case, mode="captured")
    _judge("GoT actor + CNN critic, captured from step 2", hip, case, _reference("cnn", case))
    eager = _eager_base(amd)
    for name in ("qf", "pl"):
        for a, b in zip(hip[name], eager[name]):
            assert abs(a - b) <= 1e-6 * max(1.0, abs(b)), (name, hip[name], eager[name])
    for net in T.NETWORKS:
        for k in eager[net]:
            np.testing.assert_allclose(hip[net][k].numpy(), eager[net][k].numpy(), rtol=1e-5, atol=1e-7, err_msg=f"{net}.{k}")


def test_benchmarked_step_captured(amd):
    """the step shipped_learn_step_ms.hip_graph times, at its shapes: step 0 eager, step 1 the warm-up call, steps 2 and 3 replays"""
    if ("case", "shipped") not in _REFS:
        _REFS[("case", "shipped")] = T.make_case(SHIPPED_CFG, SHIPPED_B, SHIPPED_K, SEED, "cnn")
    case = _REFS[("case", "shipped")]
    hip = _hip_run(amd, case, mode="captured", eager_steps=1)
    _judge("shipped configuration, 128 x 160, B = 32, captured from step 1", hip, case, _reference("shipped", case))


def test_prioritized_shifted_loop(amd):
    """PrioritizedDeviceReplayBuffer(100, (84, 84)) holding 80 transitions (a two-level tree); each step samples with uploaded uniforms,
    beta 0.4 and random_shift 4, weighs the critic loss and writes |q1 - y|.mean(1) back.  The reference is teacher-forced with the indices
    and shifts the device drew, shifts its own copy of the frames and keeps its own fp64 leaves.  Besides the rule: the weights of every step
    at the bound of test_gpu_prioritized_replay.py::test_weights_equal_the_restatement (rtol 1e-5), and the leaves after every write-back at
    the bound of test_leaves_after_an_update (rtol 1e-5) widened by MARGIN times the reference's own fp32 error of a written-back priority,
    carried through (|p| + eps)^alpha."""
    case = _case()
    rng = np.random.default_rng(SEED)
    per = dict(PER, store=T.make_store(CFG, PER["stored"], SEED + 1000), priorities=(rng.random(PER["stored"]) * 5).astype(np.float32),
               uniforms=[rng.random(B).astype(np.float32) for _ in range(K)], idx=[], obs_shift=[], next_obs_shift=[])
    hip = _hip_run(amd, case, per=per)
    assert all(i.min() >= 0 and i.max() < PER["stored"] for i in per["idx"])
    assert all(np.abs(s).max() == PER["pad"] for s in per["obs_shift"] + per["next_obs_shift"]), "the shifts reach the pad"
    assert any(not np.array_equal(a, b) for a, b in zip(per["obs_shift"], per["next_obs_shift"]))
    print("  repeated indices per step:", [B - np.unique(i).size for i in per["idx"]])
    r64, r32, _ = ref = _reference("per", case, per=per)
    _judge("GoT actor + CNN critic, prioritized and shifted", hip, case, ref)
    slack = T.MARGIN * T.td_yardstick(r32, r64)
    wide = T.leaf_widening(per, r64, slack)
    for k in range(K):
        werr = np.abs(hip["weights"][k] / r64["weights"][k] - 1).max()
        bound = 1e-5 * r64["leaves"][k] + wide[k]
        lerr = np.abs(hip["leaves"][k] - r64["leaves"][k])
        print(f"  step {k}: weights off by {werr:.3g} relative (bound 1e-5; smallest weight {r64['weights'][k].min():.3f}); leaves at most "
              f"{(lerr / bound).max():.3g} of their bound (priority slack {slack:.3g})")
        np.testing.assert_allclose(hip["weights"][k], r64["weights"][k], rtol=1e-5, atol=0, err_msg=f"weights, step {k}")
        assert (lerr <= bound).all(), (k, float((lerr / bound).max()))
    assert r64["weights"][K - 1].min() < 0.9, "the weights are not all 1"


def test_cnn_actor_draws_through_the_same_hook(amd):
    """cnn_networks.GaussianPolicy.sample takes its N(0, 1) draw from sac_networks._standard_normal too: with the injected draw 0 the action
    is tanh(mean), and with the draw e it is tanh(mean + std e)"""
    m = _load_state(amd.GaussianPolicy(2, 2), O.make_params(O.cnn_policy_param_spec(), SEED))
    img, pstate, _, _ = (t.cuda() for t in O.make_inputs(CFG, 5, SEED))
    with _injected(5) as draws, torch.no_grad():
        a0, _, tmean = m.sample([img, pstate])
        assert draws.calls == 1 and torch.equal(a0, tmean)
        e = torch.tensor([[-1.5, 1.5]] * 5, device="cuda")
        draws.bufs[1].copy_(e)
        a1, logp, _ = m.sample([img, pstate])
        assert draws.calls == 2
        mean, log_std = m([img, pstate])
    ref_a = torch.tanh(mean.double().cpu() + log_std.double().cpu().exp() * e.double().cpu())
    np.testing.assert_allclose(a1.cpu().numpy(), ref_a.numpy(), rtol=0, atol=1e-6)
    assert logp.shape == (5, 1) and not torch.equal(a1, a0)
