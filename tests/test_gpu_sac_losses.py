"""GPU: the SAC loss head (dgvit_amd.sac_losses; csrc/sac_loss.hip) against its restatement tests/sac_losses_ref.py -- kernel parity, the
conditions that hold bit for bit, the autograd wiring, capture with a temperature that changes between replays, and learn() steps with a
learned temperature followed against the float64 learner.

The rule of the parity test is the project's trajectory rule: per output, max |hip - ref64| / max |ref64|, the largest over the cases,
against MARGIN times the same quantity of the restatement's own fp32 evaluation -- the yardstick, nothing of it comes from the HIP side.
MARGIN is 2 with a float alpha (the same arithmetic in another summation order) and 4 with log_alpha (the device's expf differs from
libm's, sac_trajectory_ref's margin).  Where the fp32 evaluation of a case is exact the output must be within 2^-23 relative.

Measured on an MI355X (largest relative error over the 5 shapes x {done} x {weights}; the test prints the table):
                 float alpha (margin 2)            log_alpha (margin 4)
  output         hip        yardstick  ratio       hip        yardstick  ratio
  target         5.400e-08  7.014e-08  0.77        4.416e-08  7.258e-08  0.61
  loss           4.845e-08  1.302e-07  0.37        5.185e-08  1.292e-07  0.40
  td             7.585e-08  7.634e-08  0.99        1.187e-07  8.259e-08  1.44
  dq1            6.570e-08  8.909e-08  0.74        7.402e-08  1.017e-07  0.73
  dq2            8.180e-08  1.109e-07  0.74        6.539e-08  1.073e-07  0.61
  policy_loss    4.450e-08  6.164e-08  0.72        3.478e-08  1.015e-07  0.34
  dlog_pi        4.568e-08  7.660e-08  0.60        3.760e-08  4.783e-08  0.79
  dq1_pi, dq2_pi 2.421e-08  2.421e-08  1.00        2.421e-08  2.421e-08  1.00
  alpha_loss                                       3.104e-08  1.642e-07  0.19
  dlog_alpha                                       2.606e-08  1.223e-07  0.21
Exact in fp32, and bit-exact on the device: dq1_pi / dq2_pi at (64, 2) and (1, 1).  td against torch's mean of the returned target: 0 ulp
at A = 2, 3, 7 and 16.  Trajectory (K = 6, hip / yardstick): eager qf 1.00, pl 0.39, al 0.75, parameters 0.16 to 1.00; captured from step
2 qf 1.00, pl 0.40, al 1.00, parameters 0.19 to 1.06; no element beyond 0.1 lr; log_alpha within 0.45 ulp of the fp64 run's at every step
(the fp32 reference run's own distance, to the digit).
"""
import contextlib
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O  # noqa: E402,F401
import sac_losses_ref as R  # noqa: E402
import sac_trajectory_ref as T  # noqa: E402

SHAPES = [(1, 1), (37, 2), (64, 2), (300, 3), (1025, 2)]     # less than a wave; a ragged wave; exact values (B A = 128); more than one pass of
#                                                              the 256 threads with A no power of two (b = i / A); a ragged last pass
GAMMA, ALPHA, TARGET_ENTROPY = 0.99, 0.2, -2.0
LOG_ALPHA = float(np.float32(-1.3))
CFG, B, K, LR, SEED = T.BASE_CFG, T.BASE_B, T.BASE_K, T.BASE_LR, T.BASE_SEED
TAU = T.BASE_KW["tau"]
CRITIC_OUT = ("target", "loss", "td", "dq1", "dq2")
ACTOR_OUT = ("policy_loss", "dlog_pi", "dq1_pi", "dq2_pi")
TEMP_OUT = ("alpha_loss", "dlog_alpha")


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


_CACHE = {}


def _inputs(Bn, A):
    """fp32 CPU tensors: N(0, 1) values, done at p = 0.25, weights in (0, 1]"""
    key = ("in", Bn, A)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * Bn + A)
        n = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)  # noqa: E731
        _CACHE[key] = dict(q1=n(Bn, A), q2=n(Bn, A), reward=n(Bn, 1), q1n=n(Bn, A), q2n=n(Bn, A), nlp=n(Bn, 1), lp=n(Bn, 1), q1p=n(Bn, A), q2p=n(Bn, A),
                           done=(torch.rand(Bn, 1, generator=g) < 0.25).float(), w=1 - torch.rand(Bn, 1, generator=g))
    return _CACHE[key]


def _reference(Bn, A, dtype, learned, use_done, use_w):
    """every output of both losses from the restatement in ``dtype``, as float64 tensors; computed once per case"""
    key = ("ref", Bn, A, dtype, learned, use_done, use_w)
    if key in _CACHE:
        return _CACHE[key]
    x = {k: v.to(dtype) for k, v in _inputs(Bn, A).items()}
    la = torch.tensor([LOG_ALPHA], dtype=dtype, requires_grad=True)
    alpha = la.detach().exp() if learned else ALPHA
    q1, q2 = x["q1"].clone().requires_grad_(True), x["q2"].clone().requires_grad_(True)
    y = R.target(x["reward"], x["q1n"], x["q2n"], x["nlp"], alpha, GAMMA, x["done"] if use_done else None)
    loss = R.critic_loss(q1, q2, y, x["w"] if use_w else None)
    loss.backward()
    out = dict(target=y, loss=loss.detach(), td=R.td(q1.detach(), y), dq1=q1.grad, dq2=q2.grad)
    lp, q1p, q2p = (x[k].clone().requires_grad_(True) for k in ("lp", "q1p", "q2p"))
    pl = R.actor_loss(alpha, lp, q1p, q2p)
    pl.backward()
    out.update(policy_loss=pl.detach(), dlog_pi=lp.grad, dq1_pi=q1p.grad, dq2_pi=q2p.grad)
    if learned:
        al = R.alpha_loss(la, x["lp"], TARGET_ENTROPY)
        al.backward()
        out.update(alpha_loss=al.detach(), dlog_alpha=la.grad)
    _CACHE[key] = {k: v.detach().double() for k, v in out.items()}
    return _CACHE[key]


def _device(amd, Bn, A, learned, use_done, use_w):
    """the same outputs from the device, through the public functions and autograd, on the CPU as float64"""
    S = amd.sac_losses
    x = {k: v.cuda() for k, v in _inputs(Bn, A).items()}
    la = torch.tensor([LOG_ALPHA], device="cuda", requires_grad=True)
    temp = dict(log_alpha=la) if learned else dict(alpha=ALPHA)
    q1, q2 = x["q1"].requires_grad_(True), x["q2"].requires_grad_(True)
    c = S.critic_loss(q1, q2, x["reward"], x["q1n"], x["q2n"], x["nlp"], gamma=GAMMA, done=x["done"] if use_done else None,
                      weights=x["w"] if use_w else None, **temp)
    c.loss.backward()
    assert c.loss.shape == () and c.td.shape == (Bn,) and c.target.shape == (Bn, A) and not c.td.requires_grad and not c.target.requires_grad
    out = dict(target=c.target, loss=c.loss, td=c.td, dq1=q1.grad, dq2=q2.grad)
    lp, q1p, q2p = (x[k].requires_grad_(True) for k in ("lp", "q1p", "q2p"))
    pl, al = S.actor_loss(lp, q1p, q2p, target_entropy=TARGET_ENTROPY if learned else None, **temp)
    pl.backward()
    assert la.grad is None, "nothing flows from the policy loss (or the critic loss) into log_alpha"
    out.update(policy_loss=pl, dlog_pi=lp.grad, dq1_pi=q1p.grad, dq2_pi=q2p.grad)
    if learned:
        lp.grad = None
        al.backward()
        assert lp.grad is None, "nothing flows from the temperature loss into log_pi"
        out.update(alpha_loss=al, dlog_alpha=la.grad)
    else:
        assert al is None
    return {k: v.detach().double().cpu() for k, v in out.items()}


def _rel(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------ kernel parity
@pytest.mark.parametrize("learned", [False, True], ids=["float_alpha", "log_alpha"])
def test_kernel_parity(amd, learned):
    margin = 4.0 if learned else 2.0
    names = CRITIC_OUT + ACTOR_OUT + (TEMP_OUT if learned else ())
    hip, yard, exact = {k: 0.0 for k in names}, {k: 0.0 for k in names}, []
    for Bn, A in SHAPES:
        for use_done in (False, True):
            for use_w in (False, True):
                r64, r32 = (_reference(Bn, A, dt, learned, use_done, use_w) for dt in (torch.float64, torch.float32))
                dev = _device(amd, Bn, A, learned, use_done, use_w)
                assert set(dev) == set(names) == set(r64)
                for k in names:
                    assert dev[k].shape == r64[k].shape, (k, dev[k].shape, r64[k].shape)
                    h, y = _rel(dev[k], r64[k]), _rel(r32[k], r64[k])
                    hip[k], yard[k] = max(hip[k], h), max(yard[k], y)
                    if y == 0.0:       # the fp32 evaluation is exact here (alpha / B at B = 64, 1 / (B A) at B A = 128, ...)
                        exact.append((k, Bn, A, h))
    print(f"\n{'log_alpha' if learned else 'float alpha'} (margin {margin}): output  hip  yardstick  hip/yardstick")
    for k in names:
        print(f"  {k:12s} {hip[k]:.3e}  {yard[k]:.3e}  {hip[k] / yard[k] if yard[k] > 0 else math.inf:.2f}")
    print("  outputs whose fp32 evaluation is exact, and the device's relative error there:", sorted(set((k, b, a) for k, b, a, _ in exact)),
          max((h for *_, h in exact), default=0.0))
    assert exact, "some case is exact in fp32"
    for k, Bn, A, h in exact:
        assert h <= 2.0 ** -23, (k, Bn, A, h)
    for k in names:
        assert yard[k] > 0, k
        assert hip[k] <= margin * yard[k], (k, hip[k], yard[k])


# ------------------------------------------------------------------------------------------------ exact conditions
def _call(amd, Bn, A, **kw):
    x = {k: v.cuda() for k, v in _inputs(Bn, A).items()}
    return x, amd.sac_losses.critic_loss(x["q1"], x["q2"], x["reward"], x["q1n"], x["q2n"], x["nlp"], gamma=GAMMA, **kw)


@pytest.mark.parametrize("Bn, A", [(37, 2), (300, 3), (33, 7), (5, 16)])      # td sums a row in another association at A = 2, 3, 7, 16
def test_exact_conditions_of_the_critic(amd, Bn, A):
    la = torch.tensor([LOG_ALPHA], device="cuda")
    x, c = _call(amd, Bn, A, log_alpha=la, done=_inputs(Bn, A)["done"].cuda(), weights=_inputs(Bn, A)["w"].cuda())
    rows = x["done"][:, 0] == 1
    assert rows.any() and not rows.all()
    assert torch.equal(c.target[rows], x["reward"][rows].expand(-1, A)), "a finished row's target is its reward"
    assert not torch.equal(c.target[~rows], x["reward"][~rows].expand(-1, A))
    # None is the neutral tensor, bit for bit; (B,) and (B, 1) are the same argument
    _, plain = _call(amd, Bn, A, alpha=ALPHA)
    _, ones = _call(amd, Bn, A, alpha=ALPHA, weights=torch.ones(Bn, 1, device="cuda"), done=torch.zeros(Bn, device="cuda"))
    for a, b in zip(plain, ones):
        assert torch.equal(a, b)
    # two calls give the same bits
    _, again = _call(amd, Bn, A, log_alpha=la, done=x["done"], weights=x["w"])
    for a, b in zip(c, again):
        assert torch.equal(a, b)
    # td is torch's (q1 - target).abs().mean(1) of the returned target, to 1 ulp (2^-23 of its magnitude)
    want = (x["q1"] - c.target).abs().mean(1)
    err = ((c.td - want).abs() / want).max().item()
    print(f"td against torch's mean of the returned target: {err / 2.0 ** -23:.2f} ulp")
    assert err <= 2.0 ** -23


def test_ties_get_half_each(amd):
    Bn, A = 300, 3
    x = {k: v.cuda() for k, v in _inputs(Bn, A).items()}
    q1p, q2p = x["q1p"].clone(), x["q2p"].clone()
    q2p[:, 0] = q1p[:, 0]
    q2p[:5] = q1p[:5]
    q1p.requires_grad_(True), q2p.requires_grad_(True)
    lp = x["lp"].requires_grad_(True)
    pl, al = amd.sac_losses.actor_loss(lp, q1p, q2p, alpha=ALPHA)
    pl.backward()
    tie, lt = (q1p == q2p).detach(), (q1p < q2p).detach()
    n = Bn * A
    for got, smaller in ((q1p.grad, lt), (q2p.grad, ~lt & ~tie)):
        want = torch.zeros(Bn, A, device="cuda")
        want[smaller], want[tie] = -1.0 / n, -0.5 / n
        assert torch.equal(got, want)
    assert tie.sum() >= Bn and torch.equal(lp.grad, torch.full_like(lp, np.float32(np.float64(np.float32(ALPHA)) / Bn)))
    pl2, _ = amd.sac_losses.actor_loss(lp, q1p, q2p, alpha=ALPHA)
    assert torch.equal(pl2, pl.detach())


# ------------------------------------------------------------------------------------------------ wiring
def test_backward_with_a_non_unit_upstream_gradient(amd):
    Bn, A = 37, 2
    x = {k: v.cuda() for k, v in _inputs(Bn, A).items()}
    q1, q2 = x["q1"].requires_grad_(True), x["q2"].requires_grad_(True)
    c = amd.sac_losses.critic_loss(q1, q2, x["reward"], x["q1n"], x["q2n"], x["nlp"], alpha=ALPHA, weights=x["w"])
    c.loss.backward(retain_graph=True)
    g1, g2 = q1.grad.clone(), q2.grad.clone()
    q1.grad = q2.grad = None
    (3 * c.loss).backward()
    assert torch.equal(q1.grad, 3 * g1) and torch.equal(q2.grad, 3 * g2) and g1.abs().max() > 0
    for t in (x["reward"], x["q1n"], x["q2n"], x["nlp"], x["w"]):
        assert t.grad is None


def test_inputs_that_need_no_gradient_get_none(amd):
    Bn, A = 37, 2
    x = {k: v.cuda() for k, v in _inputs(Bn, A).items()}
    q2 = x["q2"].requires_grad_(True)
    c = amd.sac_losses.critic_loss(x["q1"], q2, x["reward"], x["q1n"], x["q2n"], x["nlp"], alpha=ALPHA)
    c.loss.backward()
    assert x["q1"].grad is None and q2.grad is not None
    with torch.no_grad():
        c = amd.sac_losses.critic_loss(x["q1"], q2, x["reward"], x["q1n"], x["q2n"], x["nlp"], alpha=ALPHA)
    assert not c.loss.requires_grad
    la = torch.tensor([LOG_ALPHA], device="cuda")              # a constant temperature held on the device
    q1p = x["q1p"].requires_grad_(True)
    pl, al = amd.sac_losses.actor_loss(x["lp"], q1p, x["q2p"], log_alpha=la, target_entropy=TARGET_ENTROPY)
    assert pl.requires_grad and not al.requires_grad
    pl.backward()
    assert x["lp"].grad is None and x["q2p"].grad is None and q1p.grad is not None and la.grad is None


@pytest.mark.parametrize("order", ["policy_first", "alpha_first", "summed"])
def test_the_two_actor_losses_are_separate_nodes(amd, order):
    Bn, A = 300, 3
    x = {k: v.cuda() for k, v in _inputs(Bn, A).items()}
    r32 = _reference(Bn, A, torch.float32, True, False, False)
    la = torch.tensor([LOG_ALPHA], device="cuda", requires_grad=True)
    lp, q1p, q2p = (x[k].requires_grad_(True) for k in ("lp", "q1p", "q2p"))
    pl, al = amd.sac_losses.actor_loss(lp, q1p, q2p, log_alpha=la, target_entropy=TARGET_ENTROPY)
    if order == "summed":
        (pl + al).backward()
    else:
        first, second = (pl, al) if order == "policy_first" else (al, pl)
        first.backward()
        assert (la.grad is None) == (order == "policy_first") and (lp.grad is None) == (order == "alpha_first")
        second.backward()
    assert la.grad.shape == (1,) and la.grad.dtype == torch.float32 and lp.grad.shape == (Bn, 1)
    for got, name in ((la.grad, "dlog_alpha"), (lp.grad, "dlog_pi"), (q1p.grad, "dq1_pi"), (q2p.grad, "dq2_pi")):
        np.testing.assert_allclose(got.double().cpu().numpy(), r32[name].numpy(), rtol=1e-5, atol=0, err_msg=name)
    key = ("order", "grads")
    now = [t.grad.clone() for t in (la, lp, q1p, q2p)]
    if key in _CACHE:      # every order leaves the same bits
        assert all(torch.equal(a, b) for a, b in zip(now, _CACHE[key]))
    _CACHE[key] = now


def test_flat_adam_consumes_the_temperature_gradient(amd):
    from dgvit_amd.optim import FlatAdam
    x = {k: v.cuda() for k, v in _inputs(37, 2).items()}
    la = torch.tensor([LOG_ALPHA], device="cuda", requires_grad=True)
    opt = FlatAdam([la], lr=1e-2)
    _, al = amd.sac_losses.actor_loss(x["lp"], x["q1p"], x["q2p"], log_alpha=la, target_entropy=TARGET_ENTROPY)
    opt.zero_grad()
    al.backward()
    g = float(la.grad)
    opt.step()
    assert g != 0 and float(la.detach()) == pytest.approx(LOG_ALPHA - 1e-2 * math.copysign(1.0, g), rel=1e-6), "Adam's first step moves by lr against the sign"


# ------------------------------------------------------------------------------------------------ capture
def test_a_captured_step_reads_log_alpha_at_replay_time(amd):
    S = amd.sac_losses
    Bn, A = 37, 2
    x = {k: v.cuda() for k, v in _inputs(Bn, A).items()}
    la = torch.tensor([math.log(0.2)], device="cuda")
    q1 = x["q1"].requires_grad_(True)

    def fn():
        c = S.critic_loss(q1, x["q2"], x["reward"], x["q1n"], x["q2n"], x["nlp"], log_alpha=la, gamma=GAMMA, done=x["done"], weights=x["w"])
        q1.grad = None
        (2 * c.loss).backward()
        pl, al = S.actor_loss(x["lp"], x["q1p"], x["q2p"], log_alpha=la, target_entropy=TARGET_ENTROPY)
        return c.loss, c.target, c.td, q1.grad, pl, al

    graph = amd.GraphedStep(fn, warmup=1)
    seen = []
    for value in (math.log(0.2), math.log(0.5), -3.0):
        la.fill_(value)
        out = [t.clone() for t in graph()]
        eager = fn()
        for a, b in zip(out, eager):
            assert torch.equal(a, b), "a replay computes what an eager call computes with the log_alpha of that time"
        seen.append(out)
    assert not torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[1][1], seen[2][1]), "the target follows the temperature"
    alpha = math.exp(float(np.float32(-3.0)))
    want = x["reward"] + (1 - x["done"]) * GAMMA * (torch.minimum(x["q1n"], x["q2n"]) - alpha * x["nlp"])
    np.testing.assert_allclose(seen[2][1].cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------------------------ trajectory with a learned temperature
def _case():
    if "case" not in _CACHE:
        case, done = R.make_case(CFG, B, K, SEED), R.make_done(B, K, SEED)
        r64, r32 = R.run(case, torch.float64, done=done), R.run(case, torch.float32, done=done)
        _CACHE["case"] = (case, done, r64, r32, R.distance(r32, r64, LR))
    case, done, r64, r32, Y = _CACHE["case"]
    assert T.cap_violations(Y, K, LR) == [], "the reference's own fp32 run breaks the cap: the case is ill-conditioned"
    return _CACHE["case"]


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
    import dgvit_amd.sac_networks as N
    draws = _Draws(batch)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(N, "_standard_normal", draws)
        yield draws


def _hip_run(amd, case, done, captured, eager_steps=2):
    """The K steps on the device: sac_losses_ref.run's order with the fused losses, FlatAdam for actor, critic and [log_alpha].  Captured:
    FlatAdam(capturable=True), steps 0 .. eager_steps - 1 eager, the next GraphedStep's warm-up call, the rest replays."""
    from dgvit_amd.optim import FlatAdam, soft_update
    S = amd.sac_losses
    cfg, nsteps, batch = case["cfg"], len(case["steps"]), case["batch"]
    kw = dict(image_size=cfg.image, patch_size=cfg.patch)
    pol = _load_state(amd.GoTPolicy(2, 2, cfg.depth, cfg.heads, cfg.dim, **kw), case["actor"])
    crt = _load_state(amd.QNetwork(2, 2), case["critic_params"])
    tgt = copy.deepcopy(crt)
    log_alpha = torch.tensor([R.LOG_ALPHA0], device="cuda", requires_grad=True)
    op, oc = FlatAdam([pol], lr=LR, capturable=captured), FlatAdam([crt], lr=LR, capturable=captured)
    ot = FlatAdam([log_alpha], lr=R.ALPHA_LR, capturable=captured)
    fields = ("obs", "pobs", "act", "rew", "next_obs", "next_pobs")
    X = {f: torch.zeros_like(case["steps"][0][f], device="cuda") for f in fields}
    X["done"] = torch.zeros(batch, 1, device="cuda")
    out = dict(qf=[], pl=[], al=[], td=[], y=[], log_alpha=[])

    with _injected(batch) as draws:
        def fill(k):
            s = case["steps"][k]
            for f in fields:
                X[f].copy_(s[f])
            X["done"].copy_(done[k])
            draws.bufs[0].copy_(s["e1"])
            draws.bufs[1].copy_(s["e2"])

        def learn():
            with torch.no_grad():
                na, nlogp, _ = pol.sample([X["next_obs"], X["next_pobs"]])
                q1n, q2n = tgt([X["next_obs"], X["next_pobs"], na])
            q1, q2 = crt([X["obs"], X["pobs"], X["act"]])
            c = S.critic_loss(q1, q2, X["rew"], q1n, q2n, nlogp, log_alpha=log_alpha, gamma=GAMMA, done=X["done"])
            oc.zero_grad(); c.loss.backward(); oc.step()
            pi, logp, _ = pol.sample([X["obs"], X["pobs"]])
            q1p, q2p = crt([X["obs"], X["pobs"], pi])
            pl, al = S.actor_loss(logp, q1p, q2p, log_alpha=log_alpha, target_entropy=R.TARGET_ENTROPY)
            op.zero_grad(); oc.zero_grad(); ot.zero_grad()
            pl.backward(); op.step()
            al.backward(); ot.step()
            soft_update(tgt, crt, TAU)
            return dict(qf=c.loss.detach(), pl=pl.detach(), al=al.detach(), td=c.td, y=c.target, log_alpha=log_alpha.detach().clone())

        def record(o):
            torch.cuda.synchronize()
            for name in ("qf", "pl", "al", "log_alpha"):
                out[name].append(float(o[name].double()))
            out["td"].append(o["td"].cpu().clone()), out["y"].append(o["y"].cpu().clone())

        if not captured:
            for k in range(nsteps):
                fill(k)
                record(learn())
        else:
            for k in range(eager_steps):
                fill(k)
                record(learn())
            calls = []
            fill(eager_steps)
            graph = amd.GraphedStep(lambda: calls.append(learn()) or calls[-1], warmup=1)
            assert len(calls) == 2, "one warm-up call, which ran the step, and the capture, which ran nothing"
            record(calls[0])
            for k in range(eager_steps + 1, nsteps):
                fill(k)
                record(graph())
        assert draws.calls > 0 and draws.calls % 2 == 0
    for net, m in (("actor", pol), ("critic", crt), ("target", tgt)):
        out[net] = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return out


@pytest.mark.parametrize("mode", ["eager", "captured"])
def test_trajectory_with_a_learned_temperature(amd, mode):
    """GoTPolicy + CNN QNetwork at sac_trajectory_ref's base case with done ~ Bernoulli(0.25), log_alpha from log 0.2, target_entropy -2,
    alpha_lr 1e-2: six steps, eager or captured from step 2, under sac_trajectory_ref.check (MARGIN 4) with the temperature loss as one
    more loss quantity; log_alpha after each step within K ulps of the fp64 run's."""
    case, done, r64, r32, Y = _case()
    hip = _hip_run(amd, case, done, captured=mode == "captured")
    d = R.distance(hip, r64, LR)
    r, bad = R.check(d, Y, K, LR)
    print(T.report(f"learned temperature, {mode}", d, Y, r))
    print(f"  al             {d['al']:.3e}  {Y['al']:.3e}  {r['al']:.2f}")
    ulps = R.log_alpha_ulps(hip, r64)
    print("  log_alpha per step:", hip["log_alpha"], "ulps from the fp64 run:", [f"{u:.2f}" for u in ulps], "fp32 reference run's:",
          [f"{u:.2f}" for u in R.log_alpha_ulps(r32, r64)])
    print("  target: largest difference from the fp64 run", max(float((a.double() - b).abs().max()) for a, b in zip(hip["y"], r64["y"])),
          "fp32 reference run's", max(float((a.double() - b).abs().max()) for a, b in zip(r32["y"], r64["y"])))
    assert not bad, "\n".join(bad)
    assert max(ulps) <= K, ulps
    assert all(abs(a - b) > 0.5 * R.ALPHA_LR for a, b in zip([R.LOG_ALPHA0] + hip["log_alpha"], hip["log_alpha"])), "the temperature moves every step"
    rows = done[K - 1][:, 0] == 1
    assert torch.equal(hip["y"][K - 1][rows], case["steps"][K - 1]["rew"][rows].expand(-1, 2))
