"""CPU (no GPU): keeps the fp32 attention matrix of tests/attention_fp32_cases.py honest.

The GPU file (tests/test_gpu_attention_fp32_matrix.py) holds the kernels of attention.hip and attention_long.hip to an fp64 reference
under a rule whose every number comes from here.  Without a device: the reference agrees with autograd on an independent formulation,
with and without the dropout mask; the restatement meets the rule against itself in every order it has, and its yardstick
stays under the cap; the builders of the exact classes keep their promises and the restatement reproduces them bit for bit;
kernel_reached is a literal transcription of the dispatch and the table covers every kernel and every listed token count; every seeded
defect breaks the rule or an exact promise on every small problem of the table it applies to (the many-item problems of the pipelined
kernel differ from these in their item count only); the dropped restatement uses the masks of layer_dropout_ref; and the library
refuses the illegal calls before it touches a device.
"""
import ctypes

import pytest
import torch

import attention_fp32_cases as A
import layer_dropout_ref as LD

CASES = A.all_cases()
# everything but the pipelined kernel's item counts; of the one-query kernels' 130-item problems those at 50 tokens
SMALL = sorted({A.problem(c) for c in CASES if c.B * c.H <= 9 or (c.B * c.H == 130 and c.N == 50)})
ERR_ARG, ERR_WORKSPACE = -1, -4


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_tensors():
    yield
    A.clear_caches()


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("dh", A.DHS)
@pytest.mark.parametrize("cls,keep,nq", [("gauss", 1.0, 45), ("moving-max", 1.0, 45), ("offset-v", 1.0, 45), ("token0", 1.0, 45), ("gauss", 0.5, 45),
                                         ("gauss", 0.9, 33), ("gauss", 1.0, 1)])
def test_reference_is_autograds_softmax_attention(cls, keep, nq, dh):
    """out, lse and the gradient against torch.softmax / logsumexp per head under autograd (another formulation: no explicit maximum,
    no explicit dS; the mask applied to the probabilities as GoalFormer.py:78 does)"""
    p = A.Problem("bwd", cls, 2, 45, 3, dh, nq, keep)
    ops, ref = A.operands(p), A.cpu_reference(p)
    x = ops.qkv.double().requires_grad_(True)
    I = p.H * dh
    outs, lses = [], []
    for h in range(p.H):
        q, k, v = (x[..., j * I + h * dh: j * I + (h + 1) * dh] for j in range(3))
        dots = torch.einsum("bid,bjd->bij", q, k) * A.scale32(dh)
        attn = torch.softmax(dots, -1)
        if keep < 1:
            attn = attn * ops.meta["mask"][:, h] / float(torch.tensor(keep, dtype=torch.float32))
        outs.append(attn @ v)
        lses.append(torch.logsumexp(dots, -1) / A.LN2)
    out = torch.cat(outs, -1)
    (out * ops.dout.double()).sum().backward()              # dout rows >= nq are zero
    torch.testing.assert_close(ref["out"][0], out.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["lse"][0], torch.stack(lses, 1).detach(), rtol=1e-12, atol=1e-12)
    for k, g in A.split_dqkv(x.grad, p.H).items():
        torch.testing.assert_close(ref[k][0], g, rtol=1e-10, atol=1e-12 * float(g.abs().max()))
    for k, (r, m) in ref.items():
        assert bool((m >= 0).all()) and bool(torch.isfinite(m).all()) and float(m.max()) > 0, k


def test_ulp_helper_and_constants():
    x = torch.tensor([1.0, 1.99, 2.0, 100.0, -0.75, 0.0], dtype=torch.float64)
    assert A.ulp_f32(x).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -17, 2.0 ** -24, 0.0]
    assert A.scale32(64) == 0.125 and abs(A.scale32(32) - 32 ** -0.5) < 2.0 ** -26
    assert A.select_lse(64) == 4096.0 * float(torch.tensor(A.LOG2E, dtype=torch.float32))
    assert A.n_codes(32) >= max(A.TILED_N) and A.MARGIN == 2.0 and A.Y_CAP == 8.0 and A.LSE_FLOOR_ULPS == 4


# ------------------------------------------------------------------------------------------------ the restatement against itself
Y_SEEN = {}


@pytest.mark.parametrize("p", SMALL, ids=A.problem_id)
def test_restatement_meets_the_rule_and_every_defect_breaks_it(p):
    Y = A.yardsticks(p)
    for k, y in Y.items():
        assert 0.0 <= y <= A.Y_CAP, f"yardstick of {k} outside [0, {A.Y_CAP}] masses: {Y}"
        zero_ref = p.cls in A.EXACT_CLASSES or (k != "lse" and p.N == 1)      # nothing to round: p = 1 exactly, dq = dk = 0 up to luck
        assert y > 0.0 or zero_ref, f"{k}: the restatement is the fp64 reference: the yardstick measures nothing"
        key = (p.op, p.cls, k, p.keep < 1)
        Y_SEEN[key] = (min(y, Y_SEEN.get(key, (9.0, 0.0))[0]), max(y, Y_SEEN.get(key, (9.0, 0.0))[1]))
    forms = A.forms_of(p)
    for name, got in forms.items():
        j = A.judge(p, got, Y=Y)
        assert all(t <= 1.0 for t, _, _ in j.values()), f"{name}: {j}"
        assert not A.exact_violations(p, got), f"{name} breaks the exact promises of {p.cls}: {A.exact_violations(p, got)}"
    for d in A.DEFECTS:
        if not A.defect_applies(d, p):
            continue
        got = A.restated(p, d.name, d.online)
        worst = max(t for t, _, _ in A.judge(p, got, Y=Y).values())
        assert worst > 1.0 or A.exact_violations(p, got), f"defect {d.name} passes: tightness {worst:.3f}"
        if d.name == "swap_tiles":
            assert A.exact_violations(p, got), f"{d.name} must break an exact promise of {p.cls}"


def test_zz_yardsticks_seen():
    """the table of DESIGN: smallest and largest Y per class and output over the small problems (run after the test above)"""
    print()
    for key in sorted(Y_SEEN):
        print("attention fp32 Y:", *key, "min %.3f max %.3f" % Y_SEEN[key])
    assert all(hi <= A.Y_CAP for _, hi in Y_SEEN.values())


def test_every_defect_is_tried_on_every_class_it_names():
    for d in A.DEFECTS:
        hit = {p.cls for p in SMALL if A.defect_applies(d, p)}
        assert hit == set(d.classes), (d.name, d.op, sorted(set(d.classes) - hit))
    assert {d.name for d in A.DEFECTS} >= {"drop_last", "bwd_drop_last", "pad_key", "no_log2e", "no_rescale", "swap_tiles", "head_v", "frame_k", "stale_k",
                                           "lse_nat", "lse_nomax", "no_delta", "no_scale_dk", "dq_scaled_twice", "no_inv_keep", "mask_transposed",
                                           "mask_stride", "mask_other_layer", "bwd_mask_differs", "lse_dropped"}


def test_a_row_past_nq_written_is_caught():
    """the structural defect: rows >= nq must keep the bits they held"""
    before = torch.full((2, 40, 192), float("nan"))
    after = before.clone()
    after[:, :33] = 1.0
    assert A.rows_kept(after, before, 33, "out") and A.rows_kept(after, before, 33, "dq")
    after[1, 33, 5] = 1.0
    assert not A.rows_kept(after, before, 33, "out")
    lb = torch.full((2, 3, 40), float("nan"))
    la = lb.clone()
    la[..., :1] = 0.5
    assert A.rows_kept(la, lb, 1, "lse")
    la[0, 2, 1] = 0.5
    assert not A.rows_kept(la, lb, 1, "lse")


def test_an_unwritten_or_poisoned_element_is_rejected():
    p = A.Problem("fwd", "gauss", 2, 33, 3, 64, 33, 1.0)
    got = A.restated(p)
    got["out"] = got["out"].clone()
    got["out"][1, 32, 191] = float("nan")
    assert A.judge(p, got)["out"][0] == A.INF


def test_one_token_gradients_are_noise_below_the_floor():
    """N = 1: dq = dk = 0 in exact arithmetic (dP and delta are the same number); in fp32 they are two sums of the same dh products in
    two orders.  The floor at a zero reference is the mass, and the restatement's noise is below it."""
    for dh in A.DHS:
        p = A.Problem("bwd", "gauss", 2, 1, 3, dh, 1, 1.0)
        ref, got = A.cpu_reference(p), A.restated(p)
        for k in ("dq", "dk"):
            assert bool((ref[k][0].abs() <= 1e-13).all()) and bool((got[k].double().abs() <= ref[k][1]).all()), k      # (fp64's own noise)


# ------------------------------------------------------------------------------------------------ the exact classes
@pytest.mark.parametrize("dh", A.DHS)
@pytest.mark.parametrize("N", [1, 2, 33, 288, 513])
def test_select_and_tie_builders_keep_their_promises(N, dh):
    """the builders assert the lead themselves; here: the promised outputs are what fp64 gives, to fp64's own accuracy (lse: to the one
    fp32 rounding of qscale), and tie's average is in general not representable"""
    for cls in ("select", "tie"):
        if cls == "tie" and N < 2:
            continue
        for op in ("fwd", "bwd"):
            p = A.Problem(op, cls, 2, N, 3, dh, N, 1.0)
            ops, ref = A.operands(p), A.reference(A.operands(p))
            for k, e in A.select_expect(ops, p).items():
                err = (e.double() - ref[k][0]).abs()
                assert bool((err <= 2.0 ** -23 * ref[k][0].abs() + 1e-30).all()), (cls, op, k, float(err.max()))
            if cls == "tie" and op == "fwd" and N >= 33:
                v = A.split(ops.qkv, 3)[2].double()
                pi, npair = ops.meta["pi"], ops.meta["npair"]
                idx = pi[..., None].expand(2, 3, N, dh)
                s = torch.gather(v, 2, idx) + torch.gather(v, 2, idx + npair)
                assert bool((s.float().double() != s).any()), "every tie sum is representable: nothing to round"


# ------------------------------------------------------------------------------------------------ the table and the dispatch
def _dispatch_transcribed(op, entry, B, N, H, dh, nq, keep, g_attn_q1, g_attn_bwd64):
    """attention.hip (attention_fwd, attention_bwd, ATTN_DISPATCH) and attention_long.hip (attention_fwd_tiled, attention_bwd_tiled),
    condition by condition"""
    drop = keep is not None
    if entry == "tiled":
        if drop and keep < 1.0:
            return "tiled_drop"
        return "tiled"
    nt = (N + 31) // 32

    def attn_dispatch():
        if nt == 1:
            return 1
        if nt == 2:
            return 2
        return 4

    if op == "fwd":
        if drop and keep < 1.0:
            return "drop"
        if g_attn_q1 and nq == 1 and N <= 64:
            return "q1"
        if nq == N and N > 32 and N <= 64 and B * H >= 2048:
            return "pipe"
        return f"tile{attn_dispatch()}"
    if drop and keep < 1.0:
        return "drop"
    if g_attn_q1 and nq == 1 and N <= 64:
        return "q1"
    if g_attn_bwd64 and nq == N and N > 32 and N <= 64:
        return "bwd64"
    return f"two-phase{attn_dispatch()}"


def test_kernel_reached_restates_the_dispatch():
    for c in CASES:
        want = _dispatch_transcribed(c.op, c.entry, c.B, c.N, c.H, c.dh, c.nq, c.keep if c.keep < 1 else None,
                                     1 if c.q1 is None else c.q1, 1 if c.bwd64 is None else c.bwd64)
        assert A.kernel_reached(c) == want, A.case_id(c)
    for N in range(1, 289):
        for nq in {1, min(33, N), N}:
            for B, H in ((2, 3), (89, 23), (512, 4)):
                for q1 in (None, 0, 1):
                    for b64 in (None, 0, 1):
                        for keep in (1.0, 0.5):
                            for op in ("fwd", "bwd"):
                                c = A.Case(op, "fused", "gauss", B, N, H, 64, nq, True, q1, b64, keep)
                                want = _dispatch_transcribed(op, "fused", B, N, H, 64, nq, keep if keep < 1 else None, 1 if q1 is None else q1,
                                                             1 if b64 is None else b64)
                                assert A.kernel_reached(c) == want, A.case_id(c)

    def c(N=50, nq=None, **kw):
        return A.Case(**{**dict(op="fwd", entry="fused", cls="gauss", B=2, N=N, H=3, dh=64, nq=N if nq is None else nq, lse=True, q1=None,
                                bwd64=None, keep=1.0), **kw})

    assert [A.kernel_reached(c(N=n)) for n in (32, 33, 64, 65, 288)] == ["tile1", "tile2", "tile2", "tile4", "tile4"]
    assert A.kernel_reached(c(B=512, H=4)) == "pipe" and A.kernel_reached(c(B=89, H=23)) == "tile2" and A.kernel_reached(c(B=512, H=4, N=32)) == "tile1"
    assert A.kernel_reached(c(B=512, H=4, nq=33)) == "tile2" and A.kernel_reached(c(B=512, H=4, N=65)) == "tile4"
    assert A.kernel_reached(c(nq=1)) == "q1" and A.kernel_reached(c(nq=1, q1=0)) == "tile2" and A.kernel_reached(c(N=65, nq=1)) == "tile4"
    assert A.kernel_reached(c(nq=1, keep=0.5)) == "drop" and A.kernel_reached(c(entry="tiled", keep=0.9)) == "tiled_drop"
    assert A.kernel_reached(c(op="bwd")) == "bwd64" and A.kernel_reached(c(op="bwd", bwd64=0)) == "two-phase2"
    assert A.kernel_reached(c(op="bwd", nq=33)) == "two-phase2" and A.kernel_reached(c(op="bwd", nq=1)) == "q1"
    assert A.kernel_reached(c(op="bwd", N=32)) == "two-phase1" and A.kernel_reached(c(op="bwd", N=65)) == "two-phase4"
    assert A.kernel_reached(c(op="bwd", entry="tiled", N=513)) == "tiled"


def test_table_reaches_every_kernel_at_every_listed_token_count():
    for dh in A.DHS:
        cases = [c for c in CASES if c.dh == dh]
        dense = {}
        for c in cases:
            if c.nq == c.N or A.kernel_reached(c) == "q1":
                dense.setdefault((c.op, A.kernel_reached(c)), set()).add(c.N)
        for op, names in (("fwd", A.FWD_KERNELS), ("bwd", A.BWD_KERNELS)):
            for k in names:
                assert (op, k) in dense, f"{op} {k}: not reached at dim_head {dh}"
                assert set(A.LISTED_N[(op, k)]) <= dense[(op, k)], (op, k, dh, sorted(set(A.LISTED_N[(op, k)]) - dense[(op, k)]))
        fwd = [c for c in cases if c.op == "fwd"]
        # nq in {1, 33} wherever the entry takes nq
        for op in ("fwd", "bwd"):
            for k in ("tile2", "tile4", "tiled", "drop", "tiled_drop") if op == "fwd" else ("two-phase2", "two-phase4", "tiled", "drop", "tiled_drop"):
                assert {1, 33} <= {c.nq for c in cases if c.op == op and A.kernel_reached(c) == k and c.nq < c.N}, (op, k)
        for k in A.FWD_KERNELS:                                                      # lse NULL and non-NULL on every forward path
            assert {True, False} <= {c.lse for c in fwd if A.kernel_reached(c) == k}, k
        # the pipelined kernel: 2048, 2049 and 3071 items; a workgroup walks two, two or three, and three items; 2047 items fall to tile2
        pipe = [c for c in fwd if A.kernel_reached(c) == "pipe"]
        assert {c.B * c.H for c in pipe} == {2048, 2049, 3071}
        assert [A.items_per_workgroup(n) for n in (2048, 2049, 3071)] == [(2, 2), (2, 3), (2, 3)] and 3071 - 2 * 1024 == 1023
        assert {c.N for c in pipe if c.B * c.H == 2048} == set(A.TILE2_N) and {c.N for c in pipe if c.B * c.H == 3071} >= {33, 50, 64}
        assert any(c.B * c.H == 2047 and A.kernel_reached(c) == "tile2" for c in fwd)
        # the one-query kernels: every N at 1, 3, 4, 5 and 130 items, and the same cases on the tile kernels
        for op in ("fwd", "bwd"):
            q1 = [c for c in cases if c.op == op and A.kernel_reached(c) == "q1"]
            assert {(c.N, c.B * c.H) for c in q1} >= {(n, i) for n in A.Q1_N for i in (1, 3, 4, 5, 130)}
            off = {c._replace(q1=None) for c in cases if c.op == op and c.q1 == 0}
            assert off and off <= set(q1) and all(A.kernel_reached(c._replace(q1=0)).startswith(("tile", "two-phase")) for c in off)
        # every class on every kernel (dropout: the numeric classes; the exact ones need every probability)
        for op, names, classes in (("fwd", A.FWD_KERNELS, A.FWD_CLASSES), ("bwd", A.BWD_KERNELS, A.BWD_CLASSES)):
            for k in names:
                seen = {c.cls for c in cases if c.op == op and A.kernel_reached(c) == k}
                want = set(A.NUMERIC) if k in ("drop", "tiled_drop") else set(classes)
                assert want <= seen, (op, k, dh, sorted(want - seen))
        for keep in A.DROP_KEEPS:
            assert {c.N for c in cases if c.keep == keep and c.entry == "fused"} >= set(A.DROP_N)
            assert {c.N for c in cases if c.keep == keep and c.entry == "tiled"} >= set(A.DROP_TILED_N)
    for c in CASES:
        assert c.entry != "fused" or c.N <= 288
        assert 1 <= c.nq <= c.N and c.cls in (A.FWD_CLASSES if c.op == "fwd" else A.BWD_CLASSES) and c.B * c.H * c.N * 3 * c.H * c.dh < 2 ** 31
    assert any(n % 4 for n in A.DROP_N) and {2, 3} <= {c.B for c in CASES} and {2, 3} <= {c.H for c in CASES}
    assert [A.moving_max_tile(197, i) for i in range(4)] == [0, 3, 5, 6] and [A.moving_max_tile(288, i) for i in range(4)] == [0, 4, 8, 8]


# ------------------------------------------------------------------------------------------------ the masks
@pytest.mark.parametrize("N", [7, 50, 65])
def test_dropped_restatement_uses_the_masks_of_layer_dropout_ref(N):
    """the mask in the operands is layer_dropout_ref.mask(0, layer, (B, H, N, N), seed, keep); the restatement's out is the masked
    product; the defects' masks differ from it"""
    for keep in A.DROP_KEEPS:
        p = A.Problem("fwd", "gauss", 2, N, 3, 64, N, keep)
        ops = A.operands(p)
        m = LD.mask(0, A.DROP_LAYER, (2, 3, N, N), A.DROP_SEED, keep)
        assert torch.equal(ops.meta["mask"], m) and set(m.unique().tolist()) == {0.0, 1.0}
        assert abs(float(m.mean()) - keep) < 0.1
        q, k, v = A.split(ops.qkv, 3)
        pr = torch.softmax((q.double() @ k.double().transpose(-1, -2)) * A.scale32(64), -1)
        want = A.unheads((pr * m / float(torch.tensor(keep, dtype=torch.float32))) @ v.double())
        torch.testing.assert_close(A.restate_fwd(ops)[0].double(), want, rtol=1e-4, atol=1e-5)
        assert torch.equal(A.attention_mask(2, 3, N, keep, row_stride=(N + 3) // 4), m)
        assert not torch.equal(A.attention_mask(2, 3, N, keep, row_stride=N // 4), m)
        assert not torch.equal(A.attention_mask(2, 3, N, keep, layer=A.DROP_LAYER + 1), m) and not torch.equal(m.transpose(-1, -2), m)
        assert not torch.equal(A.attention_mask(2, 3, N, keep, seed=A.DROP_SEED + 1), m)
        assert torch.equal(A.attention_mask(2, 3, N, keep, frames=[1]), m[1:2])


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def libs():
    import __graft_entry__
    __graft_entry__.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    import dgvit_amd
    return dgvit_amd


FUSED = ("fwd", "bwd", "fwd_queries", "bwd_queries", "fwd_drop", "bwd_drop")
TILED = ("fwd_tiled", "bwd_tiled", "fwd_tiled_drop", "bwd_tiled_drop")
DROPS = ("fwd_drop", "bwd_drop", "fwd_tiled_drop", "bwd_tiled_drop")
TAKES_NQ = tuple(e for e in FUSED + TILED if e not in ("fwd", "bwd"))
Refusal = __import__("collections").namedtuple("Refusal", "entry what B N H dh nq keep layer null scratch code")


def refusals():
    """every call the fp32 attention entry points must turn away, with the code they return"""
    out = []

    def add(entry, what, N=33, dh=64, nq=None, keep=0.5, layer=3, null=None, scratch=None, code=ERR_ARG):
        out.append(Refusal(entry, what, 2, N, 3, dh, N if nq is None else nq, keep, layer, null, scratch, code))

    for e in FUSED:
        add(e, "N = 289", N=289)
    for e in FUSED + TILED:
        add(e, "dh = 48", dh=48)
        add(e, "N = 0", N=0, nq=0)
        for ptr in ("qkv", "out") + (("dout", "lse", "dqkv") if e.startswith("bwd") else ()) + (("scratch",) if e.startswith("bwd_tiled") else ()):
            add(e, f"NULL {ptr}", null=ptr)
    for e in TAKES_NQ:
        add(e, "nq = 0", nq=0)
        add(e, "nq = N + 1", nq=34)
    for e in DROPS:
        add(e, "keep = 0", keep=0.0)
        add(e, "keep < 0", keep=-0.5)
        add(e, "layer = -1", layer=-1)
        add(e, "layer = 2^22", layer=1 << 22)
    for e in ("bwd_tiled", "bwd_tiled_drop"):
        add(e, "short scratch", scratch=2 * 3 * 33 - 1, code=ERR_WORKSPACE)
    return out


def call_refused(lib, r, ptr, stream=None):
    """issue the refused call; ptr(name) -> address of qkv / out / lse / dout / dqkv / scratch"""
    a = lambda n: ctypes.c_void_p(0 if n == r.null else ptr(n))
    st = ctypes.c_void_p(stream or 0)
    dims = (r.B, r.N, r.H, r.dh)
    drop = (r.keep, A.DROP_SEED, None, r.layer)
    floats = 2 * 3 * 289 if r.scratch is None else r.scratch
    fwd, bwd = (a("qkv"), a("out"), a("lse")), (a("qkv"), a("out"), a("dout"), a("lse"), a("dqkv"))
    if r.entry == "fwd":
        return lib.dgvit_attention_forward(*fwd, *dims, st)
    if r.entry == "bwd":
        return lib.dgvit_attention_backward(*bwd, *dims, st)
    if r.entry == "fwd_queries":
        return lib.dgvit_attention_forward_queries(*fwd, *dims, r.nq, st)
    if r.entry == "bwd_queries":
        return lib.dgvit_attention_backward_queries(*bwd, *dims, r.nq, st)
    if r.entry == "fwd_drop":
        return lib.dgvit_attention_forward_drop(*fwd, *dims, r.nq, *drop, st)
    if r.entry == "bwd_drop":
        return lib.dgvit_attention_backward_drop(*bwd, *dims, r.nq, *drop, st)
    if r.entry == "fwd_tiled":
        return lib.dgvit_attention_forward_tiled(*fwd, *dims, r.nq, st)
    if r.entry == "bwd_tiled":
        return lib.dgvit_attention_backward_tiled(*bwd, a("scratch"), floats, *dims, r.nq, st)
    if r.entry == "fwd_tiled_drop":
        return lib.dgvit_attention_forward_tiled_drop(*fwd, *dims, r.nq, *drop, st)
    assert r.entry == "bwd_tiled_drop"
    return lib.dgvit_attention_backward_tiled_drop(*bwd, a("scratch"), floats, *dims, r.nq, *drop, st)


def test_illegal_calls_are_refused_before_any_device_call(libs):
    """every argument check of the fp32 attention entry points runs before the first device call: without a device the pointers are
    placeholders (a refused call dereferences nothing)"""
    names = ("qkv", "out", "lse", "dout", "dqkv", "scratch")
    with libs.diagnostic_library() as lib:
        for r in refusals():
            rc = call_refused(lib, r, lambda n: 0x10000 * (names.index(n) + 1))
            assert rc == r.code, f"{r.entry} {r.what}: returned {rc}"
            assert lib.dgvit_last_error(), r
    assert len(refusals()) >= 80 and {r.entry for r in refusals()} == set(FUSED + TILED)


def test_the_drop_entry_points_are_diagnostic_only(libs):
    from dgvit_amd import _lib
    for name in ("dgvit_attention_forward_drop", "dgvit_attention_backward_drop", "dgvit_attention_forward_tiled_drop", "dgvit_attention_backward_tiled_drop"):
        assert name in _lib.DIAG_SIGNATURES and name not in _lib.SIGNATURES
        assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), name), "the product library exports a test entry point"
