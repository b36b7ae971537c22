"""Shared test helpers: fixture loading, input regeneration, gradient digests."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import dgvit_oracle as O  # noqa: E402  (tests are allowed to import the oracle)

GOLDEN = os.path.join(ROOT, "tests", "golden")

import contextlib  # noqa: E402

# A/B knobs of libdgvit_hip_diag.so (include/dgvit_hip_diag.h): name -> (setter, default arguments)
_KNOBS = {
    "gemm_tile": ("dgvit_set_gemm_tile", (0,)), "gemm_split": ("dgvit_set_gemm_split", (1,)), "ln_fusion": ("dgvit_set_ln_fusion", (1,)),
    "conv_gather": ("dgvit_set_conv_gather", (1,)), "grouped_reduce": ("dgvit_set_grouped_reduce", (1,)),
    "gemm_diagnostics": ("dgvit_set_gemm_diagnostics", (0,)), "gemm_persistent": ("dgvit_set_gemm_persistent", (0, 0)),
    "small_batch_path": ("dgvit_set_small_batch_path", (0, 0)), "block_path": ("dgvit_set_block_path", (1, 4160)), "gelu_grad_store": ("dgvit_set_gelu_grad_store", (1,)), "block_fuse": ("dgvit_set_block_fuse", (2,)), "gemm_bf16_tile": ("dgvit_set_gemm_bf16_tile", (0,)),
    "gemm_bf16_mfma16": ("dgvit_set_gemm_bf16_mfma16", (1,)), "gemm_bf16_group_m": ("dgvit_set_gemm_bf16_group_m", (8,)),
    "gemm_bf16_l2_budget_kb": ("dgvit_set_gemm_bf16_l2_budget_kb", (2048,)),
    "attention_bwd_single_pass": ("dgvit_set_attention_bwd_single_pass", (1,)), "attention_single_query": ("dgvit_set_attention_single_query", (1,)), "gemm_wgrad_slice_major": ("dgvit_set_gemm_wgrad_slice_major", (1,)), "gemm_lds_pad": ("dgvit_set_gemm_lds_pad", (0,)),
}


@contextlib.contextmanager
def knobs(force_diag=False, **kw):
    """Run a block with A/B knobs set.  The product library has no knobs: when every requested value is the shipped default the
    block runs on libdgvit_hip.so itself; otherwise the package is routed through libdgvit_hip_diag.so (same sources, -DDGVIT_DIAG)
    for the duration, the knobs are set there and put back afterwards.  Yields the active library."""
    import dgvit_amd
    want = {k: (v if isinstance(v, tuple) else (v,)) for k, v in kw.items()}
    for k in want:
        assert k in _KNOBS, k
    changed = {k: v for k, v in want.items() if tuple(int(x) for x in v) != _KNOBS[k][1]}
    if not changed and not force_diag:
        yield dgvit_amd.load_library()
        return
    with dgvit_amd.diagnostic_library() as lib:
        try:
            for k, v in changed.items():
                getattr(lib, _KNOBS[k][0])(*v)
            yield lib
        finally:
            for k in changed:
                getattr(lib, _KNOBS[k][0])(*_KNOBS[k][1])


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


def fixture_cfg(fx):
    d = fx["meta/dims"]
    return O.GoTConfig(image=tuple(int(v) for v in fx["meta/image"]), patch=tuple(int(v) for v in fx["meta/patch"]),
                       dim=int(d[0]), depth=int(d[1]), heads=int(d[2]), dim_head=int(d[3]), mlp_dim=int(d[4]))


def got_case_inputs(fx, cfg, with_mask):
    """Regenerate exactly what make_golden.case_got fed the reference."""
    batch, seed = int(fx["meta/batch"]), int(fx["meta/seed"])
    img, _, _, _ = O.make_inputs(cfg, batch, seed)
    rs = np.random.RandomState(seed + 7)
    goal = torch.from_numpy(rs.standard_normal((batch, cfg.dim))).float()
    wout = torch.from_numpy(rs.standard_normal((batch, cfg.dim))).float()
    mask = None
    if with_mask:
        mask = torch.from_numpy((rs.random_sample((batch, cfg.tokens, cfg.dim)) < 0.9).astype(np.float32))
    return img, goal, wout, mask


def grad_digest(named_grads):
    """Same digest as make_golden.grad_summary, from a dict name -> grad tensor (or None)."""
    out = {}
    for k, g in named_grads.items():
        if g is None:
            out[("none", k)] = None
            continue
        g = g.detach().double().flatten().cpu()
        out[("norm", k)] = g.norm().item()
        out[("sum", k)] = g.sum().item()
        out[("head", k)] = g[:16].float().numpy()
    return out


def check_grad_digest(fx, tag, named_grads, rtol, atol, strip=""):
    """Compare gradients with the reference digest stored under ``tag`` in fixture ``fx``."""
    dig = grad_digest(named_grads)
    n_checked = 0
    for key in fx:
        if not key.startswith(tag + "/"):
            continue
        _, kind, pname = key.split("/", 2)
        ours = dig.get((kind, pname[len(strip):] if strip and pname.startswith(strip) else pname), "missing")
        assert not isinstance(ours, str), f"no gradient entry for {pname}"
        if kind == "none":
            assert ours is None or float(np.abs(named_grads[pname]).max()) == 0.0, f"{pname} should have no grad"
            continue
        assert ours is not None, f"{pname}: reference has a gradient, we have none"
        ref = fx[key]
        scale = float(fx[f"{tag}/norm/{pname}"])
        if kind == "head":
            np.testing.assert_allclose(ours, ref, rtol=rtol, atol=atol * max(1.0, scale), err_msg=key)
        elif kind == "norm":
            np.testing.assert_allclose(ours, ref, rtol=rtol, atol=atol, err_msg=key)
        else:  # sum: cancellation-prone, scale tolerance by the norm and sqrt(numel)
            np.testing.assert_allclose(ours, ref, rtol=rtol, atol=atol * max(1.0, scale) * 64, err_msg=key)
        n_checked += 1
    assert n_checked > 0
    return n_checked


# ------------------------------------------------------------------------------------------------ bf16 GEMM checks on sampled rows
# The batch bench.py's c5_bf16 times (checked against bench.py by tests/test_c5_bench_batch_host.py).
C5_BENCH_BATCH = 440

# Element bounds of the bf16 GEMM epilogues, |got - ref| <= rel * |ref| + abs, for the operand scaling of tests/test_gpu_bf16.py: A ~ N(0, 1),
# B ~ N(0, 1) / sqrt(K) (unit-variance outputs), fp32 bias ~ N(0, 1).  A bf16 output carries one rounding (half an ulp: at most 2^-8 of
# |ref|, reached just above a power of two) plus fp32 accumulation error, which the absolute term covers; fp32 outputs carry accumulation
# error only, which grows like sqrt(K).  These are the bounds tests/test_gpu_bf16.py uses for the same epilogues.
def bf16_epilogue_bound(kind, ref, K):
    if kind == "bf16":            # epilogue 0, and the pre-activation copy of epilogue 5
        return 2 ** -8 * ref.abs() + 1e-5
    if kind == "gelu":            # epilogues 1 and 5 (sigmoid form of GELU: within 2.6e-5 of the erf form)
        return 2 ** -8 * ref.abs() + 5e-5
    if kind == "dgelu":           # epilogue 3
        return 2 ** -8 * ref.abs() + 3e-5
    if kind == "f32":             # epilogue 4
        return torch.full_like(ref, 2e-5 * K ** 0.5)
    if kind == "f32_res":         # epilogue 2 with bias and residual, for UNSCALED B ~ N(0, 1) (outputs ~ sqrt(K)), as in test_gpu_bf16.py
        return torch.full_like(ref, 1e-4 * K ** 0.5)
    raise ValueError(kind)


def sampled_rows(M, extra=300, seed=0, more=()):
    """Rows of an M-row GEMM output to check against a CPU reference: every row of the first and of the last (ragged) 256-row panel,
    the rows in ``more``, and a seeded random sample of ``extra`` others.  Sorted int64 tensor."""
    rows = set(range(min(256, M))) | set(range((M - 1) // 256 * 256, M)) | {r for r in more if 0 <= r < M}
    rng = np.random.RandomState(seed)
    rows |= set(int(r) for r in rng.randint(0, M, size=extra))
    return torch.tensor(sorted(rows), dtype=torch.int64)


def gemm_ref_rows(a, b64, rows, bias=None):
    """fp64 CPU reference of rows ``rows`` of A B^T (+ bias): A is the bf16 device operand (M, >= K), b64 the CPU float64 copy of B."""
    K = b64.shape[1]
    ar = a[rows.to(a.device), :K].double().cpu()
    h = ar @ b64.T
    return h if bias is None else h + bias.double().cpu()


# ------------------------------------------------------------------------------------------------ operands past 2 GiB / 4 GiB / 2^31 elements
GIB = 1 << 30


def boundary_rows(n_rows, row_elems, itemsize=4):
    """Rows on each side of every 2^31-byte, 2^32-byte and 2^31-element offset of an (n_rows, row_elems) operand whose rows are
    row_elems elements apart (the leading dimension): for a boundary at element e, the row that holds element e - 1 and the row that
    holds element e, plus one neighbour on each side.  Boundaries the operand does not reach give nothing."""
    rows = set()
    for e in ((1 << 31) // itemsize, (1 << 32) // itemsize, 1 << 31):
        r = e // row_elems
        rows |= {q for q in (r - 2, r - 1, r, r + 1) if 0 <= q < n_rows and r < n_rows}
    return sorted(rows)


def large_rows(n_rows, row_elems, itemsize=4, extra=64, seed=0):
    """sampled_rows for a large operand: first and last panel, the rows around every byte / element boundary, a seeded sample."""
    return sampled_rows(n_rows, extra=extra, seed=seed, more=boundary_rows(n_rows, row_elems, itemsize))


def need_device_memory(nbytes):
    """Skip (with the numbers) when the device has less than ``nbytes`` free; the large-operand tests stay under 48 GiB each."""
    import pytest
    assert nbytes <= 48 * GIB, f"a large-operand test may use at most 48 GiB, this one asks for {nbytes / GIB:.1f}"
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    if free < nbytes + GIB:
        pytest.skip(f"needs {nbytes / GIB:.1f} GiB (+1 GiB slack) of device memory, {free / GIB:.1f} of {total / GIB:.1f} GiB free")
