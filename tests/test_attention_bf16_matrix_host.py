"""CPU (no GPU): keeps the bf16 attention matrix of tests/attention_bf16_cases.py honest.

The GPU file (tests/test_gpu_attention_bf16_matrix.py) holds the kernels of attention_bf16.hip and attention_bf16_long.hip to an fp64
reference under a rule whose every number comes from here.  Without a device: the reference agrees with autograd on an independent
formulation; the restatement meets the rule against itself, whole-row and online; the builders of the exact classes keep their
promises and the restatement reproduces them bit for bit; kernel_reached covers every kernel and every listed token count; every
seeded defect breaks the rule or an exact promise on every small problem of the table it applies to (the many-item problems differ
from these in their item count only); and the library refuses the illegal calls before it touches a device.
"""
import ctypes

import pytest
import torch

import attention_bf16_cases as A

CASES = A.all_cases()
SMALL = sorted({A.problem(c) for c in CASES if c.B * c.H <= 9})         # the item and the tiled problems: every class at every N


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_tensors():
    yield
    A.clear_caches()


def _restated(p, defect=None, online=False):
    ops = A.operands(p)
    if p.op == "fwd":
        return dict(zip(A.FWD_OUTPUTS, (A.restate_fwd_online if online else A.restate_fwd)(ops, defect)))
    return A.split_dqkv(A.restate_bwd(ops, *A.backward_inputs(p), defect)[0], p.H)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("cls", ["gauss", "moving-max", "offset-v", "token0"])
def test_reference_is_autograds_softmax_attention(cls):
    """out, lse and the gradient against torch.softmax / logsumexp per head under autograd (another formulation: no explicit
    maximum, no explicit dS)"""
    p = A.Problem("bwd", cls, 2, 45, 3)
    ops, ref = A.operands(p), A.cpu_reference(p)
    x = ops.qkv.double().requires_grad_(True)
    I = p.H * A.DH
    outs, lses = [], []
    for h in range(p.H):
        q, k, v = (x[..., j * I + h * A.DH: j * I + (h + 1) * A.DH] for j in range(3))
        dots = torch.einsum("bid,bjd->bij", q, k) / 8.0
        outs.append(torch.softmax(dots, -1) @ v)
        lses.append(torch.logsumexp(dots, -1) / A.LN2)
    out = torch.cat(outs, -1)
    (out * ops.dout.double()).sum().backward()
    torch.testing.assert_close(ref["out"][0], out.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref["lse"][0], torch.stack(lses, 1).detach(), rtol=1e-12, atol=1e-12)
    for k, g in A.split_dqkv(x.grad, p.H).items():
        torch.testing.assert_close(ref[k][0], g, rtol=1e-10, atol=1e-12 * float(g.abs().max()))
    for k, (r, m, m32) in ref.items():
        assert bool((m >= 0).all()) and bool(torch.isfinite(m).all()) and bool((m32 >= 0).all()), k


def test_masses_are_never_below_their_floors():
    """the floor is the cost of one rounding flip of the stored value; the mass counts that rounding among others"""
    for p in (A.Problem("bwd", "gauss", 2, 65, 3), A.Problem("bwd", "offset-v", 2, 33, 3), A.Problem("fwd", "moving-max", 2, 197, 3)):
        for k, (r, m, m32) in A.cpu_reference(p).items():
            if k != "delta":
                assert bool((m >= (A.ulp_f32(r) if k == "lse" else A.floor_of(k, r, m32))).all()) and bool((m32 <= m).all()), (p, k)
                assert k == "lse" or float((m32 / m).max()) < 2.0 ** -7, (p, k)        # the fp32 part is a sliver of the mass


def test_ulp_helpers():
    x = torch.tensor([1.0, 1.99, 2.0, 100.0, -0.75, 0.0], dtype=torch.float64)
    assert A.ulp_bf16(x).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 0.5, 2.0 ** -8, 0.0]
    assert A.ulp_f32(x).tolist() == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22, 2.0 ** -17, 2.0 ** -24, 0.0]
    t = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -10, -3.3])
    assert A._trunc_bf16(t).tolist() == [1.0, -3.296875] and A._rn_bf16(t).tolist() == [1.0078125, -3.296875]


# ------------------------------------------------------------------------------------------------ the restatement against itself
@pytest.mark.parametrize("p", SMALL, ids=lambda p: f"{p.op}-{p.cls}-B{p.B}H{p.H}N{p.N}")
def test_restatement_meets_the_rule_and_every_defect_breaks_it(p):
    Y = A.yardsticks(p)
    assert all(0.0 <= y < 1.0 for y in Y.values()), f"a yardstick outside [0, 1) masses: {Y}"
    forms = [("restatement", _restated(p))] + ([("online restatement", _restated(p, online=True))] if p.op == "fwd" else [])
    for name, got in forms:
        j = A.judge(p, got, Y=Y)
        assert all(t <= 1.0 for t, _, _ in j.values()), f"{name}: {j}"
        assert not A.exact_violations(p, got), f"{name} breaks the exact promises of {p.cls}: {A.exact_violations(p, got)}"
    for d in A.DEFECTS:
        if not A.defect_applies(d, p):
            continue
        got = _restated(p, d.name, d.online)
        worst = max(t for t, _, _ in A.judge(p, got, Y=Y).values())
        assert worst > 1.0 or A.exact_violations(p, got), f"defect {d.name} passes: tightness {worst:.3f}"
        if d.name in ("swap_tiles", "out_trunc"):
            assert A.exact_violations(p, got), f"{d.name} must break an exact promise of {p.cls}"


def test_every_defect_is_tried_on_every_class_it_names():
    for d in A.DEFECTS:
        hit = {p.cls for p in SMALL if A.defect_applies(d, p)}
        assert hit == set(d.classes), (d.name, sorted(set(d.classes) - hit))
    assert {d.name for d in A.DEFECTS} >= {"drop_last", "pad_key", "no_log2e", "p_trunc", "out_trunc", "no_rescale", "swap_tiles", "head_v",
                                           "frame_k", "stale_k", "lse_nat", "lse_nomax", "no_delta", "no_scale_dk"}


def test_a_row_past_nq_written_is_caught():
    """the fifteenth defect is structural: rows >= nq must keep the bits they held"""
    before = torch.full((2, 40, 192), float("nan"), dtype=torch.bfloat16)
    after = before.clone()
    after[:, :33] = 1.0
    assert A.rows_kept(after, before, 33, "out")
    after[1, 33, 5] = 1.0
    assert not A.rows_kept(after, before, 33, "out")
    lb = torch.full((2, 3, 40), float("nan"))
    la = lb.clone()
    la[..., :1] = 0.5
    assert A.rows_kept(la, lb, 1, "lse")
    la[0, 2, 1] = 0.5
    assert not A.rows_kept(la, lb, 1, "lse")


def test_one_token_gradients_are_zero_only_up_to_the_order_of_two_fp32_sums():
    """N = 1: dq = dk = 0 in exact arithmetic, because dP = dout . V and delta = rowsum(dout o out) are the same number.  The kernels
    form them as two fp32 sums of the same 64 products in two orders (four 16-deep matrix-core steps; one lane-sequential chain folded
    across the two halves of a wave), and two such orders do not give the same bits: exact zeros cannot be promised outside the integer
    classes.  What holds is the rule, whose floor at a zero reference is the fp32 part of the mass; here the difference of the two
    orders stays below a tenth of it."""
    import numpy as np
    p = A.Problem("bwd", "gauss", 2, 1, 3)
    ops, ref = A.operands(p), A.cpu_reference(p)
    do, v = A.heads(ops.dout.float(), 3).numpy().reshape(-1, 64), A.split(ops.qkv.float(), 3)[2].numpy().reshape(-1, 64)
    prod = (do * v).astype(np.float32)                 # exact: products of bf16 pairs
    worst, differ = 0.0, 0
    for it in range(prod.shape[0]):
        seq = np.float32(0)
        for x in prod[it]:
            seq = np.float32(seq + x)
        blocked = np.float32(0)
        for s in range(4):
            blocked = np.float32(blocked + np.float32(np.sum(prod[it, 16 * s:16 * s + 16].astype(np.float64))))
        differ += int(seq != blocked)
        worst = max(worst, abs(float(seq) - float(blocked)) / (float(np.abs(prod[it]).sum()) * A.V32))
    assert differ > 0, "the two orders agree on every item: pick other operands"
    assert worst < 8.0                                 # in units of 2^-24 of the sum of absolute products
    got = A.split_dqkv(A.restate_bwd(ops, *A.backward_inputs(p))[0], 3)
    for k in ("dq", "dk"):
        assert bool((ref[k][0] == 0).all()) and bool((got[k].double().abs() <= 0.25 * ref[k][2]).all()), k


def test_an_unwritten_or_poisoned_element_is_rejected():
    p = A.Problem("fwd", "gauss", 2, 33, 3)
    got = _restated(p)
    got["out"] = got["out"].clone()
    got["out"][1, 32, 191] = float("nan")
    assert A.judge(p, got)["out"][0] == A.INF


# ------------------------------------------------------------------------------------------------ the exact classes
@pytest.mark.parametrize("N", [1, 2, 33, 288, 545])
def test_select_and_tie_builders_keep_their_promises(N):
    """the builders assert the 2^-200 margin themselves; here: the promised outputs are what fp64 gives, to fp64's own accuracy"""
    for cls in ("select", "tie"):
        if cls == "tie" and N < 2:
            continue
        for op in ("fwd", "bwd"):
            p = A.Problem(op, cls, 2, N, 3)
            ops, ref = A.operands(p), A.reference(A.operands(p))
            exp = A.select_expect(ops, p)
            for k, e in exp.items():
                rel = 2.0 ** -8 if cls == "tie" else 2.0 ** -23          # the tie's average is rounded once to bf16; SELECT_LSE once to fp32
                err = (e.double() - ref[k][0]).abs()
                assert bool((err <= rel * ref[k][0].abs() + 1e-30).all()), (cls, op, k, float(err.max()))
            if cls == "tie" and op == "fwd" and N >= 33:
                avg = ref["out"][0].float()                               # (V_a + V_b) / 2 is exact in fp32
                assert bool((avg.to(torch.bfloat16).float() != avg).any()), "every tie average is representable: nothing to round"


# ------------------------------------------------------------------------------------------------ the table and the dispatch
def test_kernel_reached_restates_the_dispatch():
    def c(N=197, nq=None, **kw):
        return A.Case(**{**dict(op="fwd", entry="short", cls="gauss", B=2, N=N, H=3, nq=N if nq is None else nq, lse=True, long=None, waves=None), **kw})

    assert A.kernel_reached(c(N=128)) == "item4" and A.kernel_reached(c(N=129)) == "item8" and A.kernel_reached(c(N=129, nq=128)) == "item4"
    assert A.kernel_reached(c(N=257, nq=257)) == "item9" and A.kernel_reached(c(N=257, nq=257, long=1)) == "item8"
    assert A.kernel_reached(c(N=257, nq=256)) == "item8"
    assert A.kernel_reached(c(B=128, H=4, N=128, nq=128)) == "item4" and A.kernel_reached(c(B=128, H=4, N=129, nq=1)) == "stream"
    assert A.kernel_reached(c(B=128, H=4, N=224, nq=224)) == "stream" and A.kernel_reached(c(B=128, H=4, N=225, nq=225)) == "stream288"
    assert A.kernel_reached(c(B=128, H=4, N=225, nq=225, long=2)) == "item8" and A.kernel_reached(c(B=128, H=4, N=288, nq=288, long=2)) == "item9"
    assert A.kernel_reached(c(B=73, H=7, N=224, nq=224)) == "item8" and A.kernel_reached(c(B=73, H=7, N=288, nq=288)) == "item9"
    assert A.kernel_reached(c(op="bwd", N=256, nq=256)) == "dq8+dkv" and A.kernel_reached(c(op="bwd", N=257, nq=257)) == "dq9+dkv"
    assert A.kernel_reached(c(op="bwd", N=257, nq=257, long=1)) == "dq8+dkv"
    assert A.kernel_reached(c(entry="tiled")) == "tiled8" and A.kernel_reached(c(entry="tiled", waves=4)) == "tiled4"
    assert A.kernel_reached(c(entry="tiled", waves=-1)) == "tiled8" and A.kernel_reached(c(entry="tiled_drop")) == "tiled_drop"


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_table_reaches_every_kernel_at_every_listed_token_count(cus):
    cases = A.all_cases(cus)
    dense = {}
    for c in cases:
        if c.nq == c.N:
            dense.setdefault((c.op, A.kernel_reached(c)), set()).add(c.N)
    for op, names in (("fwd", A.FWD_KERNELS), ("bwd", A.BWD_KERNELS)):
        for k in names:
            assert (op, k) in dense, f"{op} {k}: not reached"
            assert set(A.LISTED_N[(op, k)]) <= dense[(op, k)], (op, k, sorted(set(A.LISTED_N[(op, k)]) - dense[(op, k)]))
    fwd = [c for c in cases if c.op == "fwd"]
    for fam in ("item4", "item8", "stream", "stream288"):                       # nq in {1, 33, N} where N alone would reach the kernel
        dense_kernel = lambda c: A.kernel_reached(c._replace(nq=c.N))
        assert {1, 33} <= {c.nq for c in fwd if c.entry == "short" and dense_kernel(c) == fam and c.nq < c.N}, fam
    for w in (4, 8):
        assert {1, 33} <= {c.nq for c in fwd if c.entry == "tiled" and c.waves == w and c.nq < c.N}
    for k in A.FWD_KERNELS:                                                      # lse NULL and non-NULL on every forward path
        assert {True, False} <= {c.lse for c in fwd if A.kernel_reached(c) == k}, k
    # the persistent kernels' item counts: exactly 512; 511 falls to the per-item kernels; 2 C + 1 and 3 C - 1 give workgroups 2 and 3 items
    for k, ns in (("stream", A.STREAM_N), ("stream288", A.STREAM288_N)):
        mine = [c for c in fwd if A.kernel_reached(c) == k]
        assert {c.N for c in mine if c.B * c.H == 512 and (c.B, c.H) == (128, 4)} == set(ns)
        counts = {c.B * c.H for c in mine}
        assert 512 in counts and min(counts) >= 512, counts
        for n in (2 * cus + 1, 3 * cus - 1):
            if n >= 512:                 # (a small device: the item kernels take these counts)
                assert n in counts and {A.items_per_workgroup(c, cus) for c in mine if c.B * c.H == n} == {(2, 3)}
                assert {c.N for c in mine if c.B * c.H == n} == set(ns)
        assert {c.N for c in fwd if (c.B, c.H) == (73, 7) and c.N in ns and A.kernel_reached(c) in ("item8", "item9")} == {ns[0], ns[-1]}
    for c in cases:
        assert c.entry != "short" or c.N <= 288
        assert 1 <= c.nq <= c.N and (c.op == "fwd" or c.nq == c.N)
        assert c.cls in (A.FWD_CLASSES if c.op == "fwd" else A.BWD_CLASSES)
    # every class on every kernel, and moving-max reaches each of its four tile positions there
    for op, names, classes in (("fwd", A.FWD_KERNELS, A.FWD_CLASSES), ("bwd", A.BWD_KERNELS, A.BWD_CLASSES)):
        for k in names:
            seen = {c.cls for c in cases if c.op == op and A.kernel_reached(c) == k}
            want = {"gauss", "select"} if k == "tiled_drop" else set(classes)
            assert want <= seen, (op, k, sorted(want - seen))
    assert all(c.B * c.H >= 4 for c in cases if c.cls == "moving-max")
    assert [A.moving_max_tile(197, i) for i in range(4)] == [0, 3, 5, 6] and [A.moving_max_tile(288, i) for i in range(4)] == [0, 4, 8, 8]


def test_many_item_shapes():
    assert A.factor_items(513) == (171, 3) and A.factor_items(767) == (59, 13) and A.factor_items(607) == (607, 1)
    for cus in (64, 256, 304):
        for n in (2 * cus + 1, 3 * cus - 1):
            B, H = A.factor_items(n)
            assert B * H == n and 3 * H * 64 * 2 * 288 < 2 ** 31


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def libs():
    import __graft_entry__
    __graft_entry__.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    import dgvit_amd
    return dgvit_amd


def refusals():
    """(entry, what, B, N, H, dh, nq, keep, null) of every call the entry points must turn away with DGVIT_ERR_ARG"""
    out = []
    for entry in ("fwd", "fwd_queries", "bwd"):
        out += [(entry, "N = 0", 2, 0, 3, 64, 0, 1.0, None), (entry, "N = 289", 2, 289, 3, 64, 289, 1.0, None)]
    for entry in ("fwd", "fwd_queries", "bwd", "fwd_tiled", "bwd_tiled", "fwd_tiled_drop", "bwd_tiled_drop"):
        out += [(entry, "dh = 32", 2, 33, 3, 32, 33, 1.0, None), (entry, "NULL qkv", 2, 33, 3, 64, 33, 1.0, "qkv"),
                (entry, "NULL out", 2, 33, 3, 64, 33, 1.0, "out")]
    for entry in ("fwd_queries", "fwd_tiled", "fwd_tiled_drop"):
        out += [(entry, "nq = 0", 2, 33, 3, 64, 0, 1.0, None), (entry, "nq = N + 1", 2, 33, 3, 64, 34, 1.0, None)]
    for entry in ("fwd_tiled", "bwd_tiled"):
        out += [(entry, "N = 0", 2, 0, 3, 64, 0, 1.0, None)]
    for entry in ("fwd_tiled_drop", "bwd_tiled_drop"):
        out += [(entry, "keep = 0", 2, 33, 3, 64, 33, 0.0, None)]
    return out


def call_refused(lib, r, ptr, stream=None):
    """issue the refused call; ptr(name) -> address of qkv / out / lse / dout / dqkv / delta"""
    entry, _, B, N, H, dh, nq, keep, null = r
    a = lambda n: ctypes.c_void_p(0 if n == null else ptr(n))
    st = ctypes.c_void_p(stream or 0)
    if entry == "fwd":
        return lib.dgvit_attention_forward_bf16(a("qkv"), a("out"), a("lse"), B, N, H, dh, st)
    if entry == "fwd_queries":
        return lib.dgvit_attention_forward_bf16_queries(a("qkv"), a("out"), a("lse"), B, N, H, dh, nq, st)
    if entry == "bwd":
        return lib.dgvit_attention_backward_bf16(a("qkv"), a("out"), a("dout"), a("lse"), a("dqkv"), a("delta"), B, N, H, dh, st)
    if entry == "fwd_tiled":
        return lib.dgvit_attention_forward_bf16_tiled(a("qkv"), a("out"), a("lse"), B, N, H, dh, nq, st)
    if entry == "bwd_tiled":
        return lib.dgvit_attention_backward_bf16_tiled(a("qkv"), a("out"), a("dout"), a("lse"), a("dqkv"), a("delta"), B, N, H, dh, st)
    if entry == "fwd_tiled_drop":
        return lib.dgvit_attention_forward_bf16_tiled_drop(a("qkv"), a("out"), a("lse"), B, N, H, dh, nq, keep, 1, None, 0, st)
    assert entry == "bwd_tiled_drop"
    return lib.dgvit_attention_backward_bf16_tiled_drop(a("qkv"), a("out"), a("dout"), a("lse"), a("dqkv"), a("delta"), B, N, H, dh, keep, 1,
                                                        None, 0, st)


def test_illegal_calls_are_refused_before_any_device_call(libs):
    """every argument check of the bf16 attention entry points runs before the first device call: without a device the pointers are
    placeholders (a refused call dereferences nothing)"""
    names = ("qkv", "out", "lse", "dout", "dqkv", "delta")
    with libs.diagnostic_library() as lib:
        for r in refusals():
            rc = call_refused(lib, r, lambda n: 0x10000 * (names.index(n) + 1))
            assert rc == -1, f"{r[0]} {r[1]}: returned {rc}"                      # DGVIT_ERR_ARG
            assert lib.dgvit_last_error(), r
    assert len(refusals()) >= 30


def test_the_queries_entry_point_is_diagnostic_only(libs):
    from dgvit_amd import _lib
    assert "dgvit_attention_forward_bf16_queries" in _lib.DIAG_SIGNATURES and "dgvit_attention_forward_bf16_queries" not in _lib.SIGNATURES
    assert not hasattr(ctypes.CDLL(_lib.LIB_PATH), "dgvit_attention_forward_bf16_queries"), "the product library exports the test entry point"
    assert callable(libs.functional.op_attention_bf16_queries)
