"""CPU (no GPU): the row-kernel matrix of tests/row_kernel_cases.py checked against itself -- the fp64 references against torch
autograd, the yardsticks against the cap, every defect against the rule, the case tables against the branch predicates restated from
csrc/norm.hip and csrc/misc_bf16.hip.  tests/test_gpu_row_kernels.py runs the same tables through the kernels."""
import os
import re

import numpy as np
import pytest
import torch

import row_kernel_cases as R
from helpers import ROOT

CSRC = os.path.join(ROOT, "dgvit-depth-goal-guided-vision-transformer-_amd", "csrc")


def _close64(a, b, what, rtol=1e-10, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    scale = max(float(np.abs(b).max()), 1e-300) if scale is None else scale
    assert float(np.abs(a - b).max()) <= rtol * scale, f"{what}: {float(np.abs(a - b).max()):.3e} against a scale of {scale:.3e}"


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("cls", R.LN_CLASSES)
def test_layernorm_reference_agrees_with_torch_autograd(cls):
    for (T, D) in ((5, 4), (5, 260), (37, 768)):
        i = R.ln_inputs(cls, T, D)
        ref = R.ln_ref64(i["x"], i["gamma"], i["beta"], i["dy"], i["dres"])
        x = torch.from_numpy(np.array(i["x"])).double().requires_grad_(True)
        g = torch.from_numpy(np.array(i["gamma"])).double().requires_grad_(True)
        b = torch.from_numpy(np.array(i["beta"])).double().requires_grad_(True)
        y = torch.nn.functional.layer_norm(x, (D,), g, b, R.EPS_LN)
        y.backward(torch.from_numpy(np.array(i["dy"])).double())
        _close64(ref["y"], y.detach().numpy(), f"y {cls} {T}x{D}")
        _close64(ref["dx"] - i["dres"].astype(np.float64), x.grad.numpy(), f"dx {cls} {T}x{D}", rtol=1e-9)
        # the gradient of constant rows with respect to gamma is exactly zero in the reference, rounding noise in torch
        _close64(ref["dgamma"] + ref["_mass_dbeta"], g.grad.numpy() + ref["_mass_dbeta"], f"dgamma {cls} {T}x{D}")
        _close64(ref["dbeta"], b.grad.numpy(), f"dbeta {cls} {T}x{D}")
        _close64(ref["mean"], x.detach().mean(1).numpy(), "mean")
        _close64(ref["rstd"], (x.detach().var(1, unbiased=False) + R.EPS_LN).rsqrt().numpy(), "rstd", rtol=1e-9)


@pytest.mark.parametrize("cls", R.RMS_CLASSES)
def test_rmsnorm_reference_agrees_with_torch_autograd(cls):
    """fp64 torch of GoalFormer.py's RMSNorm, F.normalize(x, dim=-1) * sqrt(D) * g; zero rows take torch's subgradient 0 of the norm,
    the reference's clamp branch"""
    for (B, D) in ((3, 1), (3, 3), (7, 65), (5, 768)):
        i = R.rms_inputs(cls, B, D)
        ref = R.rms_ref64(i["x"], i["g"], i["dy"])
        x = torch.from_numpy(np.array(i["x"])).double().requires_grad_(True)
        g = torch.from_numpy(np.array(i["g"])).double().requires_grad_(True)
        y = torch.nn.functional.normalize(x, dim=-1, eps=R.EPS_RMS) * float(np.sqrt(R.F32(D))) * g
        y.backward(torch.from_numpy(np.array(i["dy"])).double())
        _close64(ref["y"], y.detach().numpy(), f"y {cls} {B}x{D}")
        # (dx of a one-element row cancels to zero: compare on the scale of the terms that cancel)
        scale = ref["_umax"][:, None]
        _close64(ref["dx"] / scale, x.grad.numpy() / scale, f"dx {cls} {B}x{D}", rtol=1e-9, scale=1.0)
        _close64(ref["dg"], g.grad.numpy(), f"dg {cls} {B}x{D}", rtol=1e-9)
    if cls in ("tiny", "zero_rows"):
        assert R.rms_ref64(**{k: R.rms_inputs(cls, 3, 65)[k] for k in ("x", "g", "dy")})["_clamped"].any()


def test_colsum_reference_and_row_map():
    for c in R.col_cases():
        i = R.col_inputs(c)
        m = i["buf"][c.off:].reshape(-1, c.lda)
        live = np.zeros(m.shape, dtype=bool)
        live[[R.colsum_row(t, c.rgrp) for t in range(c.T)], :c.N] = True
        assert not np.isnan(m[live]).any() and np.isnan(m[~live]).all() and np.isnan(i["buf"][:c.off]).all()
        if c.rgrp:
            skipped = sorted(set(range(m.shape[0])) - {R.colsum_row(t, c.rgrp) for t in range(c.T)})
            assert skipped == list(range(0, m.shape[0], c.rgrp + 1)), "the map skips token 0 of every frame of rgrp + 1 rows"
        np.testing.assert_array_equal(R.col_ref64(c)["sum"], torch.from_numpy(np.array(i["rows"])).double().sum(0).numpy())


# ------------------------------------------------------------------------------------------------ the yardsticks
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_every_class_meets_the_cap(fam):
    """Every Y that enters a bound is at most Y_CAP, every class keeps cases of every branch after the admission, and the shapes turned
    away are exactly the four the module names."""
    for cls in R.family_classes(fam):
        Y = R.yardsticks(fam, cls)
        assert Y and all(0.0 <= v <= R.Y_CAP for v in Y.values()), (fam, cls, Y)
        print(f"row kernels yardstick: {fam} {cls}: " + ", ".join(f"{k} {v:.2e}" for k, v in Y.items()))
    away = {(fam, c.cls, R.case_rows(fam, c), c.D) for cls in R.family_classes(fam) if fam != "colsum"
            for c in R.family_cases(fam, cls) if not R.admitted(fam, c)}
    assert away == {t for t in R.NOT_ADMITTED if t[0] == fam}


def test_bf16_half_ulp():
    ref = np.array([0.0, 1.0, 1.5, 1.9999, 2.0, -3.0, 1e-3, 255.0, 256.0])
    want = [0.0, 2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -18, 2.0 ** -1, 1.0]
    np.testing.assert_array_equal(R.bf16_half_ulp(ref), want)
    x = torch.linspace(0.5, 4.0, 10001, dtype=torch.float64)
    err = (x.float().to(torch.bfloat16).double() - x).abs().numpy()
    assert (err <= R.bf16_half_ulp(x.numpy()) * (1 + 1e-6)).all() and err.max() > 2.0 ** -8


def test_distances_treat_nan_and_zero_rows():
    ref = np.array([[1.0, -2.0], [0.0, 0.0]])
    assert R.row_dist(ref.astype(R.F32), ref) == 0.0
    assert R.row_dist(np.array([[1.0, -2.0], [0.0, 1e-30]]), ref) == float("inf")       # an all-zero reference row: exact or nothing
    assert R.row_dist(np.array([[np.nan, -2.0], [0.0, 0.0]]), ref) == float("inf")
    assert R.row_dist(np.array([[1.0, -2.5], [0.0, 0.0]]), ref) == 0.25
    assert R.col_dist(np.array([1.0, np.nan]), np.array([1.0, 2.0]), np.array([4.0, 4.0])) == float("inf")
    assert R.col_dist(np.array([1.0, 3.0]), np.array([1.0, 2.0]), np.array([4.0, 2.0])) == 0.25
    assert R.col_dist(np.array([0.5]), np.array([0.0]), np.array([0.0]), np.array([2.0])) == 0.25
    assert R.bound(1e-7, R.ROW_FLOOR) == R.ROW_FLOOR and R.bound(1e-5, R.ROW_FLOOR) == 2e-5
    assert R.floor_of("dx", 5) == 8 * 2.0 ** -24 and R.floor_of("dbeta", 2051) == 2059 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the defects
def _cases_broken(fam, defect):
    hit = {}
    for cls in R.family_classes(fam):
        for c in R.family_cases(fam, cls):
            if R.admitted(fam, c) and R.violations(fam, c, R.fp32_evaluations(fam, c, defect)[0]):
                hit[cls] = hit.get(cls, 0) + 1
    return hit


def test_honest_fp32_passes_the_rule():
    """the rule turns away no honest evaluation (by construction of Y; this guards the plumbing of violations())"""
    for fam in R.FAMILIES:
        for cls in R.family_classes(fam):
            for c in R.family_cases(fam, cls):
                if R.admitted(fam, c):
                    for ev in R.fp32_evaluations(fam, c):
                        assert not R.violations(fam, c, ev), (fam, c)


@pytest.mark.parametrize("defect", R.LN_DEFECTS)
def test_layernorm_defects_break_the_rule(defect):
    hit = _cases_broken("ln", defect)
    print(f"row kernels defect: ln {defect}: cases that break the rule, by class: {hit}")
    assert hit, f"no case sees the defect {defect}"
    if defect == "one_pass_variance":
        # N(0, 1)-like rows cannot see it (the reason for the classes); rows with a large mean must
        assert "normal" not in hit and hit.get("offset", 0) >= 10 and hit.get("tight", 0) >= 10
    if defect in ("drop_c2", "c1_without_gamma"):
        assert all(hit.get(cls, 0) >= 10 for cls in ("normal", "offset", "tight", "spike", "scaled"))
    if defect == "padded_mean":
        assert all(hit.get(cls, 0) >= 10 for cls in R.LN_CLASSES)
    if defect == "neighbour_rstd":
        assert hit.get("scaled", 0) >= 10 and "const" not in hit       # (constant rows all have the same rstd)


@pytest.mark.parametrize("defect", R.RMS_DEFECTS)
def test_rmsnorm_defects_break_the_rule(defect):
    hit = _cases_broken("rms", defect)
    print(f"row kernels defect: rms {defect}: cases that break the rule, by class: {hit}")
    assert hit
    if defect == "drop_projection":
        assert all(hit.get(cls, 0) >= 10 for cls in ("normal", "scaled", "spike", "huge")) and "tiny" not in hit
    if defect == "clamp_keeps_projection":
        assert hit.get("tiny", 0) >= 10 and "normal" not in hit and "huge" not in hit
    if defect == "n_cubed":
        # the kernel as it was: norm^3 past the fp32 range drops the projection term; moderate norms are fine
        assert hit.get("huge", 0) >= 20 and "normal" not in hit and "tiny" not in hit


def test_colsum_defect_breaks_the_rule():
    hit = _cases_broken("colsum", "rgrp_without_plus_one")
    assert hit == {"normal": sum(1 for c in R.col_cases() if c.rgrp)}


def test_n_cubed_error_is_the_missing_projection():
    """What the repaired kernel was doing on rows with a norm above 7e12: dx without its projection term, 0.08 - 0.12 of |dx| at D = 256."""
    c = R.RmsCase("huge", 255, 256)
    i = R.rms_inputs(c.cls, c.B, c.D)
    ref = R.reference("rms", c)
    old, new = R.rms_f32(i["x"], i["g"], i["dy"], defect="n_cubed"), R.rms_f32(i["x"], i["g"], i["dy"])
    rel = lambda got: float(np.abs(got - ref["dx"]).max() / np.abs(ref["dx"]).max())
    assert rel(old["dx"]) > 0.05 and rel(new["dx"]) < 1e-6
    n =np.sqrt((i["x"].astype(np.float64) ** 2).sum(1))
    assert n.min() > 7e12 and float(np.float32(n.max()) * np.float32(n.max())) < np.finfo(np.float32).max


# ------------------------------------------------------------------------------------------------ the table reaches every branch
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_restated_predicates_match_the_sources():
    norm, misc = _src("norm.hip"), _src("misc_bf16.hip")
    assert "int layernorm_bwd_blocks(int T) { return T < 2048 ? (T + 3) / 4 : (T < 16384 ? 512 : 2048); }" in norm
    assert "static int layernorm_bwd_blocks_f32(int T) { return T < 2048 ? (T + 3) / 4 : 512; }" in norm
    assert "int rmsnorm_bwd_blocks(int B) { return B < 256 ? (B + 3) / 4 : 64; }" in norm
    assert "int colsum_blocks(int T) { return T < 64 ? 1 : (T < 16384 ? 16 : 64); }" in norm
    assert "int colsum_bf16_blocks(int rows) { return rows < 4096 ? 1 : (rows < 16384 ? 64 : 256); }" in misc
    assert "const int nch = (D + 255) / 256;" in norm
    assert len(re.findall(r"D % 4 == 0 && D <= 1024", norm)) == 2 and "D > 0 && D <= 4096, \"rmsnorm_bwd" in norm
    assert "rgrp > 0 ? (long long)t + t / rgrp + 1 : (long long)t" in norm
    assert "N % 4 == 0 && lda % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 15) == 0" in norm
    assert "nr < 1e-12f" in norm and "n * n * n" not in norm
    for T in (1, 2047, 2048, 16383, 16384):
        assert R.ln_bwd_blocks_bf16(T) == ((T + 3) // 4 if T < 2048 else 512 if T < 16384 else 2048)


def test_layernorm_table_reaches_every_branch():
    cases = [c for cls in R.LN_CLASSES for c in R.ln_cases(cls)]
    for cls in R.LN_CLASSES:
        cs = [c for c in R.ln_cases(cls) if R.admitted("ln", c)]
        assert {R.ln_nch(c.D) for c in cs} == {1, 2, 3, 4}
        assert {c.D for c in cs if R.ln_last_chunk_lanes(c.D) == 1} >= {260, 516, 772} - ({4} if cls == "offset" else set())
        assert any(R.ln_last_chunk_lanes(c.D) == 64 for c in cs)                       # 256, 768, 1024: full last chunk
        assert {c.rs for c in cs} == {1, 5}
        blocks = {(R.ln_bwd_blocks_f32(c.T), R.ln_bwd_grid_strides(c.T, R.ln_bwd_blocks_f32(c.T))) for c in cs}
        assert {(1, False), (2, False), (512, False), (512, True)} <= blocks          # T = 1, 5, 2047, 2051
        assert any(c.T % 4 for c in cs)                                                # a ragged last workgroup
    assert {c.T for c in cases} == {1, 5, 2047, 2051} and {c.D for c in cases} == set(R.LN_D)
    assert all(R.ln_bwd_accepts(D) for D in R.LN_D) and not R.ln_bwd_accepts(R.LN_D_FWD_ONLY) and R.LN_D_FWD_ONLY % 4 == 0
    # the strided long case survives the admission in every class but "offset"
    assert all(any(c.T == 2051 and c.rs == 5 and R.admitted("ln", c) for c in R.ln_cases(cls)) for cls in R.LN_CLASSES if cls != "offset")


def test_bf16_layernorm_tables_reach_every_branch():
    for cls in R.LN_CLASSES:
        fwd = R.lnb_fwd_cases(cls)
        assert all(R.admitted("lnb_fwd", c) for c in fwd)
        for D in R.LN_D:
            got = {(R.lnb_add(c.variant),) + R.LNB_VARIANTS[c.variant][1:] for c in fwd if c.D == D}
            # ADD 0 with and without statistics; ADD 1 with xout + statistics and with neither; ADD 2 with and without xout
            assert got == {(0, False, True), (0, False, False), (1, True, True), (1, False, False), (2, True, False), (2, False, False)}
            assert {c.variant for c in fwd if c.D == D and c.rs == 5} == set(R.LNB_STRIDED)
        bwd = [c for c in R.lnb_bwd_cases(cls) if R.admitted("lnb_bwd", c)]
        assert {R.ln_nch(c.D) for c in bwd} == {1, 2, 3, 4} and {c.rs for c in bwd} == {1, 5}
        blocks = {(R.ln_bwd_blocks_bf16(c.T), R.ln_bwd_grid_strides(c.T, R.ln_bwd_blocks_bf16(c.T))) for c in bwd}
        assert blocks == {(2, False), (512, True), (2048, True)}
        assert all(c.D == 64 for c in bwd if c.T > 5)
    # the joint form has contiguous rows and no statistics (add2_layernorm_fwd_bf16 passes rs = 1 and NULL)
    assert all(not R.LNB_VARIANTS[v][2] for v in R.LNB_VARIANTS if v not in R.LNB_STRIDED and R.lnb_add(v))


def test_rmsnorm_table_reaches_every_branch():
    for cls in R.RMS_CLASSES:
        cs = R.rms_cases(cls)
        assert all(R.admitted("rms", c) for c in cs)
        assert {(c.B, c.D) for c in cs} == {(B, D) for B in R.RMS_B for D in R.RMS_D}
        assert {R.rms_bwd_blocks(c.B) for c in cs} == {1, 64}
        assert any(c.B > 4 * R.rms_bwd_blocks(c.B) for c in cs), "a wave takes a second row"
        assert any(c.D % 64 for c in cs) and any(c.D < 64 for c in cs) and max(c.D for c in cs) == 4096
    assert all(R.rms_bwd_accepts(D) for D in R.RMS_D) and not R.rms_bwd_accepts(4097)
    clamped = lambda cls, B, D: R.reference("rms", R.RmsCase(cls, B, D))["_clamped"]
    assert clamped("tiny", 259, 768).all() and not clamped("normal", 259, 768).any() and not clamped("huge", 259, 768).any()
    z = clamped("zero_rows", 259, 768)
    assert z[::3].all() and not z[1::3].any() and not z[2::3].any()
    # "tiny" rows are clamped with x != 0: the branch in which a kept projection term would show
    assert np.abs(R.rms_inputs("tiny", 259, 768)["x"]).min() > 0
    n = np.sqrt((R.rms_inputs("scaled", 259, 768)["x"].astype(np.float64) ** 2).sum(1))
    assert n.min() < 1e-9 and n.max() > 1e9


def test_colsum_table_reaches_every_branch():
    cs = R.col_cases()
    assert {R.colsum_blocks(c.T) for c in cs} == {1, 16, 64} and {c.T for c in cs} == set(R.COL_T)
    for T in R.COL_T:
        at = [c for c in cs if c.T == T]
        assert {R.colsum_takes_vec(c) for c in at} == {True, False} and {c.rgrp for c in at} == {0, 4}
        scalar = [c for c in at if not R.colsum_takes_vec(c)]
        assert any(c.N % 4 for c in scalar) and any(c.lda % 2 and c.lda > c.N for c in scalar) and any(c.off % 4 for c in scalar)
        assert any(c.lda > c.N for c in at if R.colsum_takes_vec(c))
    trips = {T: R.colsum4_trips(T) for T in R.COL_T}
    assert trips[1] == (0, 1) and trips[63][0] > 0 and trips[63][1] > 0            # 63 rows, one block: rows 0..30 full, then ragged
    assert trips[64] == (0, 64) and trips[515] == (64, 3) and trips[16387][0] > 0 and trips[16387][1] > 0
    # which block counts of colsum_bf16 the existing operator test reaches (tests/test_gpu_bf16.py::test_wgrad_bf16): all three
    assert {R.colsum_bf16_blocks(T) for T in (394, 4000, 9001, 64, 20000, 33, 1)} == {1, 64, 256}


def test_helper_tables():
    assert any(r % 64 or c % 64 for r, c in R.TRANSPOSE_SHAPES) and (64, 64) in R.TRANSPOSE_SHAPES
    assert all(r % 8 == 0 and c % 8 == 0 for r, c in R.TRANSPOSE_SHAPES)
    assert {rs for _, _, rs in R.RESIDUAL_CASES} == {1, 5} and any(rows * D // 4 > 256 for rows, D, _ in R.RESIDUAL_CASES)
