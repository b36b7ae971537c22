"""CPU (no GPU): keeps the fp32 GEMM epilogue matrix of tests/gemm_epilogue_cases.py honest.

The GPU file (tests/test_gpu_gemm_epilogues.py) compares dgvit_gemm with an fp64 reference under a bound taken from the existing
tests.  Here, without a device: the reference agrees with autograd; the bound admits a plain fp32 evaluation with a factor of two
to spare and rejects eight deliberately wrong evaluations; and the case table reaches every dispatch path it claims, according to a
restatement of gemm_f32 / pick_tile / auto_tile / split_plan that is compared with the library's own host entry point.
"""
import math

import pytest
import torch

import gemm_epilogue_cases as G

CASES = G.all_cases()


# ------------------------------------------------------------------------------------------------ the reference against autograd
def test_reference_gelu_grad_is_autograds_derivative_of_the_erf_gelu():
    t = torch.linspace(-12, 12, 4801, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.gelu(t)                     # approximate="none": the erf form
    assert torch.allclose(G.gelu(t.detach()), y.detach(), rtol=0, atol=1e-15)
    (dy,) = torch.autograd.grad(y.sum(), t)
    assert float((G.gelu_grad(t.detach()) - dy).abs().max()) <= 1e-14


def test_reference_epilogue_6_is_the_derivative_at_the_pre_activation_of_its_c2():
    c = G.class_cases("vec", G.NT, 6)[0]
    ops = G.operands(c)
    t = (ops["A"].double() @ ops["B"].double().T + ops["bias"].double()).requires_grad_(True)
    y = torch.nn.functional.gelu(t)
    (dy,) = torch.autograd.grad(y.sum(), t)
    ref = G.reference(c)
    assert float((ref["C2"] - y.detach()).abs().max()) <= 1e-13
    assert float((ref["C"] - dy).abs().max()) <= 1e-13
    # ... and epilogue 1 stores that pre-activation itself beside the same C2
    c1 = G.class_cases("vec", G.NT, 1)[0]
    o1, r1 = G.operands(c1), G.reference(c1)
    t1 = o1["A"].double() @ o1["B"].double().T + o1["bias"].double()
    assert torch.equal(r1["C"], t1) and float((r1["C2"] - torch.nn.functional.gelu(t1)).abs().max()) <= 1e-13


def test_reference_epilogue_4_is_relus_derivative_and_masks_both_zeros():
    for c in G.class_cases("vec", G.NN, 4) + G.class_cases("tiny", G.NN, 4):
        ops = G.operands(c)
        aux = ops["aux"]
        sites = G.zero_sites(c)
        signs = [math.copysign(1.0, float(aux[m, n])) for (m, n) in sites]
        assert all(float(aux[m, n]) == 0.0 for (m, n) in sites)
        assert -1.0 in signs and (len(sites) < 2 or 1.0 in signs), "both 0.0 and -0.0 are planted"
        a = aux.double().clone().requires_grad_(True)
        (mask,) = torch.autograd.grad(torch.relu(a).sum(), a)          # relu'(0) = relu'(-0) = 0
        acc = ops["A"].double() @ ops["B"].double()
        ref = G.reference(c)["C"]
        assert torch.equal(ref, acc * mask)
        for (m, n) in sites:
            assert float(ref[m, n]) == 0.0
    # no denormal aux anywhere (the kernels' handling of them is not a stated semantic)
    tiny = torch.finfo(torch.float32).tiny
    for c in CASES:
        if G.has_aux(c):
            a = G.operands(c)["aux"].abs()
            assert not ((a > 0) & (a < tiny)).any()


def test_operands_are_in_the_stated_regime():
    for c in CASES:
        ops = G.operands(c)
        if c.M * c.N >= 4096 and c.layout != G.TN:
            acc = ops["A"].double() @ (ops["B"].double().T if c.layout == G.NT else ops["B"].double())
            assert 2.5 < float(acc.std()) < 3.5, (c, float(acc.std()))
        if G.has_bias(c):
            assert float(ops["bias"][c.N - 1]) == 8.0 and float(ops["bias"][(c.N - 1) // 2]) == -8.0


# ------------------------------------------------------------------------------------------------ the bound
def test_bound_is_the_one_the_suite_already_uses():
    assert G.tol(72) == 1e-4 and G.tol(256) == 1e-4            # test_gemm_epilogues: 1e-4 absolute up to K = 256
    assert G.tol(520) == pytest.approx(1e-4 * math.sqrt(520 / 256))
    assert G.tol(1024) == pytest.approx(2e-4)
    c = G.class_cases("vec", G.NN, 7)[0]
    b, aux = G.bound(c, G.operands(c)), G.operands(c)["aux"].double().abs()
    assert torch.equal(b, G.tol(c.K) * aux.clamp_min(1.0))      # no relative term: the factor is the epilogue's own multiplier


def test_bound_admits_a_plain_fp32_evaluation_with_headroom():
    """fp32 matmul and fp32 epilogue on the CPU stay within half the bound on every case: the GPU's headroom comes from the
    reference and the number format, not from the kernel under test."""
    worst = {}
    for c in CASES:
        ops = G.operands(c)
        r = G.worst_ratio(c, ops, G.evaluate(c, ops, torch.float32), G.reference(c))
        worst[c.cls] = max(worst.get(c.cls, 0.0), r)
    print("fp32 CPU evaluation, worst error / bound per class:", {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst


@pytest.mark.parametrize("mutant", sorted(G.MUTANTS))
def test_bound_rejects_a_wrong_evaluation(mutant):
    """Each deliberately wrong evaluation (wrong arithmetic on the CPU, in fp64) violates the bound on every case it applies to."""
    applies = [c for c in CASES if G.MUTANTS[mutant](c)]
    assert applies, mutant
    survived = []
    for c in applies:
        ops = G.operands(c)
        if G.worst_ratio(c, ops, G.evaluate(c, ops, mutant=mutant), G.reference(c)) <= 1.0:
            survived.append(c)
    assert not survived, f"{mutant} stays inside the bound on {survived}"
    # every pair the mutant can touch is among them
    pairs = {(c.layout, c.epi) for c in applies}
    want = {"tanh_gelu": {(0, 1), (0, 6), (0, 8), (1, 2)}, "bias_dropped": {(0, 0), (0, 1), (0, 6), (0, 8), (0, 3), (1, 0)},
            "bias_after_activation": {(0, 1), (0, 6), (0, 8), (0, 3)}, "side_from_next_row": {(0, 0), (1, 0), (1, 2), (1, 7), (1, 4)},
            "aux_stride_n": {(1, 2), (1, 7), (1, 4)}, "c2_with_ldc": {(0, 1), (0, 6)}, "aux_ge_zero": {(1, 4)},
            "split_drops_last_slice": set(G.PAIRS)}[mutant]
    assert pairs == want


# ------------------------------------------------------------------------------------------------ the table reaches the paths it claims
def test_every_pair_has_a_case_on_every_path():
    """float4 loader + vector epilogue, float4 loader + element-wise epilogue, scalar loader, full split on the 64 x 64 x 32 tile and
    full split on the wide 64 x 128 x 16 tile: each of the nine pairs has a case in each, in the class that names it."""
    want = {"vec": ("float4", "vector", False, (64, 64, 32)), "pad": ("float4", "vector", False, (64, 64, 32)),
            "elem": ("float4", "element", False, (64, 64, 32)), "scalar": ("scalar", "element", False, (64, 64, 32)),
            "split": ("float4", "vector", True, (64, 64, 32)), "split-wide": ("float4", "vector", True, (64, 128, 16))}
    listing = []
    for (layout, epi) in G.PAIRS:
        for cls in G.CLASSES:
            cases = G.class_cases(cls, layout, epi)
            assert len(cases) == len(G.pair_variants(layout, epi)) * {"scalar": 2, "tiny": 2, "split": 2}.get(cls, 1)
            paths = {G.path(c) for c in cases}
            if cls == "tiny":      # one partial tile, element-wise (N = 2) and vector (N = 4)
                assert all(-(-c.M // 64) * -(-c.N // 64) == 1 and not G.takes_split(c) for c in cases)
            else:
                assert paths == {want[cls]}, (layout, epi, cls, paths)
            listing.append((("NT", "NN")[layout], epi, cls, sorted(paths)))
    assert len(listing) == 9 * len(G.CLASSES)
    for row in listing:
        print(*row)
    # the split class cuts 17 k-tiles into slices of 5, 5, 5 and 2; every stride of the pad class is distinct
    for c in G.class_cases("split", G.NT, 1) + G.class_cases("split", G.NN, 2):
        pl = G.gemm_split_plan(c.layout, c.M, c.N, c.K)
        assert (pl.tiles, pl.nsplit, pl.split_from, pl.kchunk) == (4, 4, 0, 160)
    c = G.class_cases("pad", G.NT, 1)[0]
    assert len({c.lda, c.ldb, c.ldc, c.ldr, c.ldc2, c.ldaux, c.N, c.K}) == 8
    # the scalar class: K % 4 = 2 and N % 4 = 2; TN: the float4 loader, then the scalar one
    assert all(c.K % 4 == 2 and c.N % 4 == 2 for c in G.class_cases("scalar", G.NT, 0))
    assert [G.vec4(c) for c in G.tn_cases()] == [True, False]
    # a shape that plans a split also takes it: no case of the table has strides that veto the split its scratch query announces
    for c in CASES:
        if c.layout != G.TN:
            assert G.takes_split(c) == (G.scratch_floats(c.layout, c.M, c.N, c.K) > 0), c


def test_tile_sweep_reaches_both_vector_epilogue_forms_and_the_split():
    """The eight tiles on "vec" and "split": the split class splits on every tile given room for its slabs, the vec class on none."""
    for t in G.TILES:
        for c in G.class_cases("vec", G.NT, 0)[:1] + G.class_cases("vec", G.NN, 0)[:1]:
            assert G.path(c, t) == ("float4", "vector", False, t)
        for c in G.class_cases("split", G.NT, 0)[:1] + G.class_cases("split", G.NN, 0)[:1]:
            assert G.takes_split(c, t, scratch=1 << 20), (t, c)


# ------------------------------------------------------------------------------------------------ the restatement against the library
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    import dgvit_amd
    return dgvit_amd.load_library()


def test_restated_split_plan_is_the_librarys(lib):
    """dgvit_gemm_scratch_floats is a pure host function: the Python restatement of auto_tile / split_plan gives its value for
    every case of the table and for a sweep of shapes around the policy's thresholds."""
    shapes = {(c.layout, c.M, c.N, c.K) for c in CASES if c.layout != G.TN}
    for layout in (G.NT, G.NN):
        for M in (1, 64, 65, 130, 2080, 8192, 16400, 25600):
            for N in (2, 64, 68, 256, 511, 512, 1023, 1024, 2048):
                for K in (4, 255, 256, 257, 304, 520, 1024, 2048):
                    shapes.add((layout, M, N, K))
    split = 0
    for (layout, M, N, K) in sorted(shapes):
        got = lib.dgvit_gemm_scratch_floats(layout, M, N, K)
        assert got == G.scratch_floats(layout, M, N, K), (layout, M, N, K)
        split += got > 0
    assert 100 < split < len(shapes) - 100
