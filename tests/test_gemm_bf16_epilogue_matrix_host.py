"""CPU (no GPU): keeps the bf16 GEMM epilogue matrix of tests/gemm_bf16_epilogue_cases.py honest.

The GPU file (tests/test_gpu_gemm_bf16_epilogues.py) compares dgvit_gemm_bf16 with an fp64 reference, bit for bit on small-integer
operands and under helpers.bf16_epilogue_bound on Gaussian ones.  Here, without a device: the reference agrees with autograd; every
partial sum of an int case is below 2^24; a plain emulation (bf16 operands, fp32 accumulation, fp32 epilogue, one bf16 rounding) equals
the int reference and stays inside the gauss bounds; eight deliberately wrong evaluations are each rejected; the table reaches every
kernel with every epilogue that kernel takes, according to a restatement of dispatch<EPI> and gemm_bf16_stream_supports; and the
library refuses the illegal calls before it touches a device.
"""
import pytest
import torch

import gemm_bf16_epilogue_cases as G
from helpers import bf16_epilogue_bound, knobs

CASES = G.all_cases()
AUTO_CASES = [c for name in G.AUTO_SHAPES for c in G.auto_cases(name)]
PROBLEMS = list(dict.fromkeys(G.problem(c) for c in CASES))            # cases that differ in path only share operands and reference


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_tensors():
    """The operands and references are computed once and shared by the tests of this file; nothing of them outlives it."""
    yield
    G.clear_caches()


# ------------------------------------------------------------------------------------------------ the reference
def test_reference_gelu_and_its_derivative_are_autograds_erf_form():
    t = torch.linspace(-12, 12, 4801, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.gelu(t)
    assert torch.allclose(G.gelu(t.detach()), y.detach(), rtol=0, atol=1e-15)
    (dy,) = torch.autograd.grad(y.sum(), t)
    assert float((G.gelu_grad(t.detach()) - dy).abs().max()) <= 1e-14


def test_reference_epilogue_5_keeps_the_pre_activation_of_its_c():
    c = [p for p in PROBLEMS if p.cls == "ragged" and p.epi == 5 and p.variant == "b" and p.regime == "gauss"][0]
    ops, ref = G.operands(c), G.reference(c)
    pre = ops["A"].double() @ ops["B"].double().T + ops["bias"].double()
    assert torch.equal(ref["C2"], pre) and float((ref["C"] - torch.nn.functional.gelu(pre)).abs().max()) <= 1e-13


def test_store_helpers_round_to_nearest_even_and_truncate():
    x = torch.tensor([257.0, 259.0, 258.0, -257.0, -259.0, 1.00390625, 1.01171875])     # ties and the values between two bf16 numbers
    assert G.round_bf16(x).tolist() == [256.0, 260.0, 258.0, -256.0, -260.0, 1.0, 1.015625]
    assert G.truncate_bf16(x).tolist() == [256.0, 258.0, 258.0, -256.0, -258.0, 1.0, 1.0078125]


# ------------------------------------------------------------------------------------------------ the int regime
def test_int_operands_keep_every_partial_sum_exact_in_fp32():
    """|sum_k a b| + |bias| + |res| < 2^24 with integer terms: fp32 accumulation is exact in any order, on any path."""
    n = 0
    for p in PROBLEMS:
        if p.regime != "int":
            continue
        ops = G.operands(p)
        assert float(ops["A"].abs().max()) <= 3 and float(ops["B"].abs().max()) <= 3
        for k in ("A", "B", "bias", "res"):
            if k in ops:
                assert torch.equal(ops[k], ops[k].round()) and float(ops[k].abs().max()) <= (3 if k in "AB" else 8)
        assert G.partial_sum_limit(p, ops) < 2 ** 24, p
        n += 1
    assert n >= 40
    assert all(p.epi in G.INT_EPILOGUES for p in PROBLEMS if p.regime == "int")


def test_int_references_have_values_only_rounding_gets_right():
    """From K = 72 the planted rows give integers above 256 that are not bf16 values: the exact comparison sees the rounding mode."""
    for p in PROBLEMS:
        if p.regime == "int" and p.epi in (0, 5) and p.K >= 72 and p.M >= 2:
            ops = G.operands(p)
            pre = ops["A"].double() @ ops["B"].double().T + (ops["bias"].double() if "bias" in ops else 0.0)
            inexact = pre != G.round_bf16(pre)
            assert int(inexact[0].sum()) >= 8 and int(inexact[p.M - 1].sum()) >= 8, p
            assert int((pre[inexact] < 0).sum()) >= 8 and int((pre[inexact] > 0).sum()) >= 8, p


# ------------------------------------------------------------------------------------------------ the bounds
def test_bounds_are_the_projects_own():
    r = torch.tensor([0.0, 1.0, -4.0], dtype=torch.float64)
    assert torch.equal(G.bf16_epilogue_bound("bf16", r, 72), bf16_epilogue_bound("bf16", r, 72))
    assert torch.equal(bf16_epilogue_bound("bf16", r, 72), 2 ** -8 * r.abs() + 1e-5)
    assert torch.equal(bf16_epilogue_bound("f32", r, 72), torch.full_like(r, 2e-5 * 72 ** 0.5))
    assert all(G.outputs(c) == {"C": "f32"} for c in CASES if c.epi in (2, 4))          # epilogue 2 with scaled B: the "f32" bound


def test_emulation_equals_the_int_reference_and_stays_inside_the_gauss_bounds():
    """bf16 operands, fp32 accumulation, the epilogue in fp32 and one bf16 rounding, on the CPU.  Int: equal.  Gauss: a bf16 store alone
    reaches 2^-8 |ref| just above a power of two, so a bf16 output can come close to its bound by nature (the absolute term and the
    distance to the power of two are the headroom); the fp32 outputs stay under a quarter of theirs."""
    worst = {}
    for p in PROBLEMS:
        ops, ref = G.operands(p), G.reference(p)
        got = G.evaluate(p, ops, mode="emul")
        if p.regime == "int":
            assert G.exact_mismatches(p, got, ref) == 0, p
            continue
        key = (p.cls, "f32" if G.out_f32(p) else "bf16")
        worst[key] = max(worst.get(key, 0.0), G.worst_ratio(p, got, ref))
    per_epi = {}
    for p in PROBLEMS:
        if p.regime == "gauss" and p.cls != "persistent":
            r = G.worst_ratio(p, G.evaluate(p, G.operands(p), mode="emul"), G.reference(p))
            per_epi[p.epi] = max(per_epi.get(p.epi, 0.0), r)
    print("bf16 CPU emulation, worst error / bound per (class, output type):", {k: round(v, 4) for k, v in sorted(worst.items())})
    print("bf16 CPU emulation, worst error / bound per epilogue:", {k: round(v, 4) for k, v in sorted(per_epi.items())})
    for (cls, kind), v in worst.items():
        assert v <= (0.25 if kind == "f32" else 1.0), (cls, kind, v)


@pytest.mark.parametrize("mutant", sorted(G.MUTANTS))
def test_comparison_rejects_a_wrong_evaluation(mutant):
    """Each deliberately wrong evaluation (wrong arithmetic on the CPU, in fp64) is over the bound on every gauss case it applies to and
    unequal on every int case it applies to."""
    applies = [p for p in PROBLEMS if G.mutant_applies(mutant, p)]
    assert applies, mutant
    survived = [p for p in applies if not G.rejected(p, G.evaluate(p, G.operands(p), mutant=mutant), G.reference(p))]
    assert not survived, f"{mutant} is accepted on {survived}"
    got = {(p.epi, p.regime) for p in applies}
    both = lambda epis: {(e, r) for e in epis for r in G.regimes(e)}
    want = {"k_chunk_dropped": both(G.EPILOGUES), "bias_shifted_4": both((0, 1, 2, 5)), "res_next_row": both((2,)), "dgelu_at_acc": both((3,)),
            "c2_activation": both((5,)), "c2_with_ldc": both((5,)), "aux_with_ldc": both((3,)), "bf16_store_truncates": both((0, 1, 3, 5))}[mutant]
    assert got == want, (mutant, got ^ want)


def test_an_unwritten_or_poisoned_element_is_rejected():
    for p in PROBLEMS:
        if p.cls == "ragged" and p.variant == G.VARIANTS[p.epi][0]:
            got = {k: v.clone() for k, v in G.reference(p).items()}
            name = (G.exact_outputs(p) or ("C",))[0]
            got[name][p.M - 1, p.N - 1] = float("nan")
            assert G.rejected(p, got, G.reference(p)), p


# ------------------------------------------------------------------------------------------------ the table reaches the kernels it claims
def test_every_epilogue_variant_and_regime_has_a_case_on_every_kernel_that_takes_it():
    """Per kernel and shape class: the set of (epilogue, variant, regime) whose cases reach that kernel.  The per-tile and ring kernels
    take everything; the stream kernel what gemm_bf16_stream_supports says, and every such epilogue has a case that really reaches it."""
    everything = {(e, v, r) for (e, v) in G.EPI_VARIANTS for r in G.regimes(e)}
    stream_takes = {(e, v, r) for (e, v, r) in everything if e in (0, 1, 4, 5)}
    persistent = {(e, v, r) for (e, v) in G.class_epi_variants("persistent") for r in G.regimes(e)}
    reach = {}
    for c in CASES:
        reach.setdefault((G.kernel_reached(c), c.cls), set()).add((c.epi, c.variant, c.regime))
    for kernel in G.KERNELS:
        for cls in G.CLASSES:
            got = reach.get((kernel, cls), set())
            if cls == "persistent":
                want = set() if kernel in ("tile64", "tile128") else persistent - ({k for k in persistent if k[0] == 2} if kernel == "stream" else set())
            elif kernel != "stream":
                want = everything            # (the ring256 kernels also take what hint 256257 hands back: a superset is the same set)
            elif cls == "n4":
                want = {k for k in stream_takes if k[0] == 4}          # N % 8 == 4: the fp32 output only
            else:
                want = stream_takes
            assert got == want, (kernel, cls, got ^ want)
    # the fallbacks of hint 256257 land on the 256 x 256 ring kernel
    back = {(c.epi, c.variant) for c in CASES if c.path.name == "stream" and G.kernel_reached(c) == "ring256"}
    assert {(2, "br"), (2, "b"), (2, "r"), (2, ""), (3, "")} <= back and (0, "b") in back      # (0, "b"): the n4 class
    # tiny: N = 4 reaches the stream kernel through epilogue 4 only
    assert {c.epi for c in CASES if c.N == 4 and G.kernel_reached(c) == "stream"} == {4}


def test_shape_classes_are_the_ones_the_kernels_can_go_wrong_at():
    shapes = {cls: G.class_shapes(cls) for cls in G.CLASSES}
    assert shapes["ragged"] == [(300, 264, 72)] and shapes["pad"] == shapes["ragged"]
    (M, N, K), = shapes["ragged"]
    assert (-(-M // 256), -(-N // 256)) == (2, 2) and M % 64 and N % 64 and K % 32 == 8 and K % 64 == 8     # ragged both ways, k-tail of 8
    assert shapes["n4"][0][1] % 8 == 4
    assert shapes["tiny"] == [(1, 8, 8), (1, 4, 128)]
    assert [s[2] for s in shapes["short-k"]] == [8, 40] and shapes["long-k"] == [(70, 72, 520)]
    (M, N, K), = shapes["persistent"]
    assert -(-M // 256) * -(-N // 256) == 306 > 256            # more 256 x 256 tiles than the chip has compute units
    # pad: every stride distinct where the launch checks allow, ldc2 == ldc where the ring and stream kernels insist
    for path in G.PATHS:
        c = [c for c in G.class_cases("pad", path) if c.epi == 5][0]
        assert (c.lda, c.ldb, c.ldc, c.ldr, c.ldaux) == (c.K + 8, c.K + 16, c.N + 16, c.N + 4, c.N + 8)
        assert (c.ldc2 != c.ldc) == G.ldc2_may_differ(path) == (path.name in ("tile64", "tile128"))
        assert len({c.lda, c.ldb, c.ldc, c.ldr, c.ldaux, c.N, c.K}) == 7
        p = [c for c in G.class_cases("persistent", path)]
        assert all(q.ldc == q.N + 16 and q.lda == q.K + 8 for q in p)


def test_every_arm_of_the_automatic_dispatch_has_a_case():
    arms = {}
    for c in AUTO_CASES:
        arms.setdefault(c.cls, set()).add(G.auto_path(c.epi, c))
    assert arms == {"auto-" + k: v for k, v in G.AUTO_ARMS.items()}
    assert set().union(*arms.values()) == {64064, 128128, 256256, 256257}
    c = G.auto_cases("mid")[0]
    assert (G.tiles(c, 128), G.tiles(c, 256)) == (156, 42)
    large = G.auto_cases("large")
    assert G.tiles(large[0], 256) == 552
    assert {c.epi for c in large if G.auto_path(c.epi, c) == 256257} == {0, 1, 4, 5}
    assert {(c.epi, c.variant) for c in large if G.auto_path(c.epi, c) == 256256} == {(2, "br"), (3, "")}
    # the thresholds themselves: 512 tiles of 256, 128 tiles of 128
    mk = lambda M, N: G._case("t", G.AUTO, "gauss", 3, "", M, N, 8)
    assert G.auto_path(3, mk(256 * 32, 256 * 16)) == 256256 and G.auto_path(3, mk(256 * 32, 256 * 16 - 256)) == 128128
    assert G.auto_path(3, mk(255, 256 * 600)) == 128128
    assert G.auto_path(3, mk(128 * 16, 128 * 8)) == 128128 and G.auto_path(3, mk(128 * 16, 128 * 8 - 128)) == 64064


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    import dgvit_amd
    return dgvit_amd.load_library()


def test_illegal_calls_are_refused_before_any_device_call(lib):
    """Every refusal of the table returns DGVIT_ERR_ARG with its message.  Without a device the pointers are placeholders (a refused
    call dereferences nothing); with one they are real buffers that cover the whole problem, so a regressed check gives a wrong return
    code, never a stray access.  The ldc2 != ldc refusals of the ring and stream kernels need their tile hint: diagnostic library."""
    names = ("A", "B", "C", "bias", "res", "C2", "aux")
    if torch.cuda.is_available():
        bufs = {n: torch.zeros(1 << 16, device="cuda") for n in names}
        ptr = lambda n: bufs[n].data_ptr()
    else:
        ptr = lambda n: 0x10000 * (names.index(n) + 1)
    seen = 0
    for r in G.refusals():
        with knobs(gemm_bf16_tile=r.hint) as active:
            rc = active.dgvit_gemm_bf16(*G.refusal_arguments(r, ptr))
            msg = active.dgvit_last_error()
        assert rc == -1, f"{r.what}: returned {rc}"                     # DGVIT_ERR_ARG
        assert msg and r.msg.encode() in msg, f"{r.what}: {msg}"
        seen += 1
    assert seen == len(G.refusals()) >= 22
