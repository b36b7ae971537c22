"""GPU: every kernel family driven with ONE operand past 2 GiB, 4 GiB or 2^31 elements, against fp64 arithmetic on sampled rows.

Method.  Operands are generated on the device and never copied whole to the host.  The fp64 reference is formed for the first and last
256-row panel, the rows on each side of every 2^31-byte, 2^32-byte and 2^31-element offset of the large operand (helpers.boundary_rows)
and a seeded random sample.  Reductions over a huge K (TN weight gradient, LayerNorm dgamma / dbeta, RMSNorm dg) are checked with probe
rows: the large operand is zero except for random data in a few dozen k-rows at those same positions, so the exact answer comes from
those rows alone and any mis-addressed read shows up as a missing term; one dense run is compared with the sum of the kernel's own
results on chunks below 2 GiB.  Tolerances are those of tests/test_gpu_ops.py for the same operator and data scale (K there = the number
of non-zero terms of a sum).  Every test states its need, skips (with the numbers) if the device has less free, stays under 48 GiB and
frees its tensors; each prints its peak allocation and wall time.

Boundary branches reached (shape in each test's docstring): gemm_tile.h Fetch::plan per-workgroup descriptor rebase and num_records clamp, the
direct C / residual / aux stores' clamp, the `lda*512` and `kchunk*ld*4` refusals and the new output-leading-dimension refusal; the
int-row / widened-offset arithmetic of norm.hip; gather_rows_kernel's source index; dropout / cast with n > 2^31; the fused and tiled
fp32 attention kernels' frame offsets past element 2^31 of qkv; the bf16 stream / ring GEMM, weight gradient, LayerNorm and the
persistent bf16 attention past 4 GiB; the CNN stack on both sides of its implicit-GEMM -> im2col fallbacks (cnn_api.hip:93-94); the fp32 encoder with an fc1 output past
4 GiB and on both sides of the patch-gather fallback (encoder.hip:235)."""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import GIB, O, boundary_rows, knobs, large_rows, need_device_memory  # noqa: E402
from layer_dropout_ref import _keep_words  # noqa: E402


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd


@pytest.fixture(autouse=True)
def _report_and_free():
    """Prints the peak device allocation and the wall time of each test, and hands the memory back."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    print(f"\n[large-operands] peak {torch.cuda.max_memory_allocated() / GIB:.2f} GiB, {time.time() - t0:.1f} s", flush=True)
    torch.cuda.empty_cache()


def _p(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from dgvit_amd import _lib as L
    return L.load()


def _ok(rc, what):
    from dgvit_amd import _lib as L
    L.check(rc, what)


def _randn_(t, seed, scale=1.0, shift=0.0):
    """N(shift, scale) into a contiguous device tensor of any size, 2^28 elements at a time (seeded, reproducible)."""
    g = torch.Generator(device=t.device).manual_seed(seed)
    flat = t.view(-1)
    for a in range(0, flat.numel(), 1 << 28):
        part = flat[a:a + (1 << 28)]
        part.normal_(shift, scale, generator=g)
    return t


def _rows(t, rows):
    """fp64 host copy of the first-axis entries `rows` (sorted) of a device tensor: one slice per run of consecutive rows, so every
    read is a plain view at a 64-bit storage offset."""
    rows = [int(r) for r in rows]
    out, a = [], 0
    while a < len(rows):
        b = a
        while b + 1 < len(rows) and rows[b + 1] == rows[b] + 1:
            b += 1
        out.append(t[rows[a]:rows[b] + 1].cpu())
        a = b + 1
    return torch.cat(out).double()


def _zero_rows(t, rows):
    """t[rows] = 0, one slice per row (plain views; no 64-bit index arithmetic of torch's own in the way)."""
    for r in rows:
        t[int(r)].zero_()


def _groups(x, groups):
    """(len(groups), 4) device tensor of the float4 groups `groups` of a flat tensor, read through 4-element views."""
    return torch.stack([x[4 * int(g):4 * int(g) + 4] for g in groups])


def _maxerr(got, ref):
    return float((got.double() - ref.double()).abs().max())


def _gemm(layout, epi, A, lda, B, ldb, C, ldc, M, N, K, bias=None, res=None, ldr=0, aux=None, ldaux=0, check=True):
    lib = _lib()
    nsc = max(int(lib.dgvit_gemm_scratch_floats(layout, M, N, K)), 4)
    sc = torch.empty(nsc, dtype=torch.float32, device="cuda")
    rc = lib.dgvit_gemm(layout, epi, _p(A), lda, _p(B), ldb, _p(C), ldc, M, N, K, _p(bias), _p(res), ldr, None, 0, _p(aux), ldaux,
                        _p(sc), nsc, _st())
    if check:
        _ok(rc, "dgvit_gemm")
    return rc


# ------------------------------------------------------------------------------------------------ elementwise (smallest first)
def test_dropout_and_cast_past_2_31_elements(amd):
    """dgvit_dropout and dgvit_cast_f32_bf16 (`long long n`) at n = 2^31 + 2^20: float4 groups around element 2^31 and the tail past it.
    The mask is compared with the Philox restatement of tests/layer_dropout_ref.py, the cast with torch's rounding (bit exact); kept values equal 1/keep to 1e-6 as in test_gpu_ops."""
    n = (1 << 31) + (1 << 20)
    need_device_memory(n * 4 + n * 2 + (1 << 28))
    from dgvit_amd import functional as F
    x = torch.ones(n, dtype=torch.float32, device="cuda")
    seed, keep = 0x1234ABCD5678, 0.9
    F.op_dropout_(x, seed, keep)
    n4 = n // 4
    rng = np.random.RandomState(5)
    g = np.unique(np.concatenate([np.arange(64), np.arange(n4 - 64, n4), np.arange((1 << 29) - 64, (1 << 29) + 64),
                                  rng.randint(0, n4, size=4096), rng.randint(1 << 29, n4, size=1024)])).astype(np.int64)
    got = _groups(x, g).cpu().numpy()
    kept = _keep_words(g, 0, seed, keep)
    assert np.array_equal(got != 0, kept), f"{int(((got != 0) != kept).sum())} of {kept.size} sampled elements differ from the Philox restatement"
    np.testing.assert_allclose(got[kept], 1.0 / 0.9, rtol=1e-6)        # kept values are scaled by 1/keep (as test_dropout_statistics_and_replay)
    tail_kept = float((x[1 << 31:] != 0).float().mean())
    assert abs(tail_kept - keep) < 5e-3, tail_kept          # the tail past 2^31 was masked at all (2^20 draws: sigma 3e-4)
    # cast: the same buffer refilled with values whose bf16 rounding is not trivial
    _randn_(x, 11)
    y = F.cast_bf16(x)
    for a, b in ((0, 1 << 20), ((1 << 31) - (1 << 20), n)):                         # head, and everything around and past element 2^31
        assert torch.equal(y[a:b], x[a:b].to(torch.bfloat16)), f"cast differs from torch's rounding in [{a}, {b})"
    assert torch.equal(_groups(y, g), _groups(x, g).to(torch.bfloat16))
    del x, y


# ------------------------------------------------------------------------------------------------ replay gather
def test_gather_rows_from_a_ring_past_2_31_floats(amd):
    """dgvit_gather_rows from 104 960 rows of 20 480 floats (2.15e9 floats, 8.6 GB): gather_rows_kernel's `s * row4 + c` source index
    for rows around element 2^31 (rows 104 857 / 104 858) and byte offsets 2^31 and 2^32, the last row, and out-of-range indices on
    both sides (these clamp).  Row r holds (7919 r + c) mod 2^24, exact in fp32; results are bit exact."""
    nrows, row = 104960, 20480
    need_device_memory(nrows * row * 4 + 3 * GIB)
    src = torch.empty(nrows, row, dtype=torch.float32, device="cuda")
    c = torch.arange(row, dtype=torch.int64, device="cuda")
    for a in range(0, nrows, 8192):
        r = torch.arange(a, min(a + 8192, nrows), dtype=torch.int64, device="cuda")
        src[a:a + 8192] = ((r[:, None] * 7919 + c[None, :]) % (1 << 24)).float()
    rng = np.random.RandomState(3)
    idx = np.concatenate([[0, nrows - 1], boundary_rows(nrows, row), [-1, -(1 << 40), nrows, nrows + 5, 1 << 40],
                          rng.randint(0, nrows, size=512)]).astype(np.int64)
    assert {104857, 104858} <= set(idx.tolist())
    out = torch.empty(len(idx), row, dtype=torch.float32, device="cuda")
    idx_d = torch.from_numpy(idx).cuda()
    _ok(_lib().dgvit_gather_rows(_p(src), _p(idx_d), _p(out), len(idx), row, nrows, _st()), "dgvit_gather_rows")
    want = ((np.clip(idx, 0, nrows - 1)[:, None] * 7919 + np.arange(row)[None, :]) % (1 << 24)).astype(np.float32)
    assert np.array_equal(out.cpu().numpy(), want)
    del src, out


def test_replay_buffer_round_trip_at_the_end_of_a_large_ring(amd):
    """DeviceReplayBuffer(size=104960): obs and next_obs are 8.6 GB each.  add_batch writes the last 110 slots (rows 104 850 ..
    104 959, across element 2^31 of the field matrix) and wraps to slots 0 and 1; sample(indices=...) returns them bit exact."""
    size = 104960
    need_device_memory(2 * size * 20480 * 4 + 2 * GIB)
    from dgvit_amd.replay import DeviceReplayBuffer
    buf = DeviceReplayBuffer(size=size, seed=1)
    rng = np.random.RandomState(8)
    n = 112
    data = {"obs": rng.standard_normal((n, 128, 160)).astype(np.float32), "next_obs": rng.standard_normal((n, 128, 160)).astype(np.float32),
            "pobs": rng.standard_normal((n, 2)).astype(np.float32), "next_pobs": rng.standard_normal((n, 2)).astype(np.float32),
            "act": rng.standard_normal((n, 2)).astype(np.float32), "rew": rng.standard_normal((n, 1)).astype(np.float32),
            "done": (rng.random_sample((n, 1)) < 0.5).astype(np.float32)}
    buf.next_index = size - 110          # the ring's write position after size - 110 earlier transitions
    buf.stored = size - 110
    buf.add_batch(**data)
    assert buf.next_index == 2 and buf.stored == size
    slots = np.concatenate([np.arange(size - 110, size), [0, 1]])
    pick = np.array([0, 1, 6, 7, 8, 9, 108, 109, 110, 111, 50])       # transitions 7 / 8 sit in slots 104 857 / 104 858
    assert slots[7] == 104857
    got = buf.sample(len(pick), indices=torch.from_numpy(slots[pick]))
    for k, v in data.items():
        assert np.array_equal(got[k].cpu().numpy(), v[pick]), k
    del buf, got


# ------------------------------------------------------------------------------------------------ norms
def test_layernorm_past_2_31_elements(amd):
    """LayerNorm forward and backward at rows = 8 400 000, D = 256 (2.15e9 elements): norm.hip's `int row = blockIdx.x * 4 + ...`
    widened per use; rows around byte offsets 2^31 (row 2^21), 2^32 (row 2^22) and element 2^31 (row 2^23).  Forward on sampled rows
    (2e-5); backward with dy non-zero in those rows only: dx there against fp64 (5e-5), dx == dres bit exact everywhere else, and
    dgamma / dbeta exact from the probe rows (1e-4 sqrt(rows that contribute)).  Then one dense backward against the sum of the
    kernel's own results on five chunks below 2 GiB."""
    T, D = 8400000, 256
    need_device_memory(4 * T * D * 4 + 2 * GIB)
    lib = _lib()
    rows = large_rows(T, D, extra=64, seed=1).tolist()
    assert {(1 << 21) - 1, 1 << 21, (1 << 22) - 1, 1 << 22, (1 << 23) - 1, 1 << 23} <= set(rows)
    x = _randn_(torch.empty(T, D, device="cuda"), 1, scale=2.0, shift=0.5)
    y = torch.empty(T, D, device="cuda")
    gam = (1 + 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(2), dtype=torch.float64))
    bet = 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    g_d, b_d = gam.float().cuda(), bet.float().cuda()
    mean, rstd = torch.empty(T, device="cuda"), torch.empty(T, device="cuda")
    _ok(lib.dgvit_layernorm_forward(_p(x), _p(g_d), _p(b_d), _p(y), _p(mean), _p(rstd), T, D, _st()), "dgvit_layernorm_forward")
    xr = _rows(x, rows).requires_grad_(True)
    gr, br = g_d.double().cpu().requires_grad_(True), b_d.double().cpu().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (D,), gr, br, 1e-5)
    e = _maxerr(_rows(y, rows), ref.detach())
    print(f"layernorm fwd max err {e:.3e} on {len(rows)} rows")
    assert e <= 2e-5
    mu = xr.detach().mean(1)
    assert _maxerr(_rows(mean, rows), mu) <= 2e-5
    assert _maxerr(_rows(rstd, rows), (xr.detach().var(1, unbiased=False) + 1e-5).rsqrt()) <= 2e-5
    # backward, probe rows: dy lives in the buffer of y
    dy = y.zero_()
    dy_rows = torch.randn(len(rows), D, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    for i, r in enumerate(rows):
        dy[r] = dy_rows[i].float().cuda()
    dres = _randn_(torch.empty(T, D, device="cuda"), 5)
    dx = torch.empty(T, D, device="cuda")
    dg, db = torch.empty(D, device="cuda"), torch.empty(D, device="cuda")
    nsc = int(lib.dgvit_layernorm_backward_scratch_floats(T, D))
    sc = torch.empty(nsc, device="cuda")

    def bwd(r0, r1):
        n = r1 - r0
        _ok(lib.dgvit_layernorm_backward(_p(dy[r0:r1]), _p(x[r0:r1]), _p(mean[r0:r1]), _p(rstd[r0:r1]), _p(g_d), _p(dres[r0:r1]), _p(dx[r0:r1]),
                                         _p(dg), _p(db), _p(sc), nsc, n, D, _st()), "dgvit_layernorm_backward")
    bwd(0, T)
    ref.backward(dy_rows.float().double())
    e = _maxerr(_rows(dx, rows), xr.grad + _rows(dres, rows))
    eg, eb = _maxerr(dg.cpu(), gr.grad), _maxerr(db.cpu(), br.grad)
    print(f"layernorm bwd: dx {e:.3e}, dgamma {eg:.3e}, dbeta {eb:.3e} ({len(rows)} probe rows)")
    assert e <= 5e-5
    tol = 1e-4 * math.sqrt(len(rows))
    assert eg <= tol and eb <= tol
    dx.sub_(dres)
    _zero_rows(dx, rows)
    assert float(dx.abs().max()) == 0.0, "a row with dy == 0 must return dres unchanged"
    # dense: the whole reduction against the sum over chunks of 2 000 000 rows (2.05 GB each: below 2 GiB)
    _randn_(dy, 6)
    bwd(0, T)
    dg_big, db_big = dg.clone(), db.clone()
    acc_g, acc_b = torch.zeros(D, dtype=torch.float64, device="cuda"), torch.zeros(D, dtype=torch.float64, device="cuda")
    for r0 in range(0, T, 2000000):
        bwd(r0, min(r0 + 2000000, T))
        acc_g += dg.double()
        acc_b += db.double()
    assert float((acc_g - dg_big).abs().max()) <= 2e-3 * float(dg_big.abs().max()) + 1e-8
    assert float((acc_b - db_big).abs().max()) <= 2e-3 * float(db_big.abs().max()) + 1e-8
    del x, y, dy, dres, dx


def test_rmsnorm_past_2_31_elements_with_padded_rows(amd):
    """RMSNorm forward and backward at rows = 8 400 000, D = 256 with ldx = lddx = 260 > D (x spans 2.18e9 elements): the
    `row * ldx` / `row * lddx` products of rmsnorm_fwd_kernel / rmsnorm_bwd_kernel.  Tolerances of test_rmsnorm_fwd_bwd: 1e-5 forward,
    2e-5 dx, 1e-4 sqrt(contributing rows) dg (probe rows)."""
    T, D, ld = 8400000, 256, 260
    need_device_memory((2 * T * ld + 2 * T * D) * 4 + 2 * GIB)
    lib = _lib()
    rows = sorted(set(large_rows(T, ld, extra=64, seed=2).tolist()) | set(boundary_rows(T, D)))
    x = _randn_(torch.empty(T, ld, device="cuda"), 1)
    x[:, D:] = float("nan")                       # the padding must never be read
    g = 1 + 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    g_d = g.float().cuda()
    y = torch.empty(T, D, device="cuda")
    _ok(lib.dgvit_rmsnorm_forward(_p(x), ld, _p(g_d), _p(y), T, D, _st()), "dgvit_rmsnorm_forward")
    xr = _rows(x, rows)[:, :D].clone().requires_grad_(True)
    gr = g_d.double().cpu().requires_grad_(True)
    ref = torch.nn.functional.normalize(xr, dim=-1) * math.sqrt(D) * gr
    e = _maxerr(_rows(y, rows), ref.detach())
    print(f"rmsnorm fwd max err {e:.3e} on {len(rows)} rows")
    assert e <= 1e-5
    dy = y.zero_()
    dy_rows = torch.randn(len(rows), D, generator=torch.Generator().manual_seed(4), dtype=torch.float64).float()
    for i, r in enumerate(rows):
        dy[r] = dy_rows[i].cuda()
    dx = torch.full((T, ld), float("nan"), device="cuda")
    dg = torch.empty(D, device="cuda")
    nsc = int(lib.dgvit_rmsnorm_backward_scratch_floats(T, D))
    sc = torch.empty(nsc, device="cuda")
    _ok(lib.dgvit_rmsnorm_backward(_p(dy), _p(x), ld, _p(g_d), _p(dx), ld, _p(dg), _p(sc), nsc, T, D, _st()), "dgvit_rmsnorm_backward")
    ref.backward(dy_rows.double())
    got = _rows(dx, rows)
    e, eg = _maxerr(got[:, :D], xr.grad), _maxerr(dg.cpu(), gr.grad)
    print(f"rmsnorm bwd: dx {e:.3e}, dg {eg:.3e}")
    assert e <= 2e-5 and eg <= 1e-4 * math.sqrt(len(rows))
    assert bool(torch.isnan(got[:, D:]).all()), "the padding of dx must not be written"
    _zero_rows(dx, rows)
    assert float(dx[:, :D].abs().max()) == 0.0, "a row with dy == 0 has no gradient"
    del x, y, dx


# ------------------------------------------------------------------------------------------------ fp32 GEMM
@pytest.mark.parametrize("tile", [0, 64])
def test_gemm_nt_a_past_4_gib(amd, tile):
    """dgvit_gemm NT, epilogue 0 with bias and residual, M = 4 200 000, K = 256, N = 64: A is 4.3 GB.  Fetch::plan() rebases the A
    descriptor per workgroup and clamps num_records to 0x7FFFFFFF (all tiles before row 2 102 848 see the clamp); rows around byte
    offsets 2^31 and 2^32 of A (rows 2^21, 2^22).  gemm_tile knob 0 and 64.  2e-4 sqrt(K)."""
    M, K, N = 4200000, 256, 64
    need_device_memory((M * K + 2 * M * N) * 4 + GIB)
    rows = large_rows(M, K, extra=64, seed=3).tolist()
    assert {(1 << 21) - 1, 1 << 21, (1 << 22) - 1, 1 << 22} <= set(rows)
    A = _randn_(torch.empty(M, K, device="cuda"), 1)
    res = _randn_(torch.empty(M, N, device="cuda"), 2)
    W = torch.randn(N, K, generator=torch.Generator().manual_seed(3)).cuda()
    b = torch.randn(N, generator=torch.Generator().manual_seed(4)).cuda()
    C = torch.empty(M, N, device="cuda")
    with knobs(gemm_tile=tile):
        _gemm(0, 0, A, K, W, K, C, N, M, N, K, bias=b, res=res, ldr=N)
    ref = _rows(A, rows) @ W.double().cpu().T + b.double().cpu() + _rows(res, rows)
    e = _maxerr(_rows(C, rows), ref)
    print(f"gemm NT tile {tile}: max err {e:.3e} on {len(rows)} rows")
    assert e <= 2e-4 * math.sqrt(K)
    del A, res, C


def test_gemm_nn_c_and_aux_past_4_gib(amd):
    """dgvit_gemm NN, epilogue 2 (C = acc * gelu'(aux)), M = 4 200 000, N = 256, K = 64: C and aux are 4.3 GB each, written and read
    through the direct epilogue's per-tile descriptors (tile_rsrc: rebased to the tile origin, clamped to 0x7FFFFFFF).  Rows around
    byte offsets 2^31 and 2^32 of C / aux.  2e-4 sqrt(K)."""
    M, N, K = 4200000, 256, 64
    need_device_memory((M * K + 2 * M * N) * 4 + GIB)
    rows = large_rows(M, N, extra=64, seed=4).tolist()
    A = _randn_(torch.empty(M, K, device="cuda"), 1)
    aux = _randn_(torch.empty(M, N, device="cuda"), 2)
    Bm = torch.randn(K, N, generator=torch.Generator().manual_seed(3)).cuda()
    C = torch.empty(M, N, device="cuda")
    _gemm(1, 2, A, K, Bm, N, C, N, M, N, K, aux=aux, ldaux=N)
    u = _rows(aux, rows)
    gp = 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    ref = (_rows(A, rows) @ Bm.double().cpu()) * gp
    e = _maxerr(_rows(C, rows), ref)
    print(f"gemm NN dgelu: max err {e:.3e} on {len(rows)} rows")
    assert e <= 2e-4 * math.sqrt(K)
    del A, aux, C


def test_gemm_nt_padded_lda_spans_past_4_gib(amd):
    """dgvit_gemm NT with M = 2304 rows 1 048 576 floats apart (lda*512 = 2^29, under the refusal): the A buffer spans 9.7 GB while
    M stays small, so every 64-row tile's rebased window is 256 MiB wide and rows 512 / 1024 / 2048 start at byte 2^31 / 2^32 /
    element 2^31.  The padding is NaN: a read past K poisons the row.  Every row is checked.  2e-4 sqrt(K)."""
    M, K, N, lda = 2304, 256, 64, 1 << 20
    need_device_memory(M * lda * 4 + GIB)
    A = torch.full((M, lda), float("nan"), device="cuda")
    a = torch.randn(M, K, generator=torch.Generator().manual_seed(1))
    A[:, :K] = a.cuda()
    W = torch.randn(N, K, generator=torch.Generator().manual_seed(2))
    b = torch.randn(N, generator=torch.Generator().manual_seed(3))
    C = torch.empty(M, N, device="cuda")
    _gemm(0, 0, A, lda, W.cuda(), K, C, N, M, N, K, bias=b.cuda())
    e = _maxerr(C.cpu(), a.double() @ W.double().T + b.double())
    print(f"gemm NT padded lda: max err {e:.3e}")
    assert e <= 2e-4 * math.sqrt(K)
    del A, C


def test_gemm_tn_split_k_over_4_2_million_rows(amd):
    """dgvit_gemm TN (split-K weight gradient), K = 4 200 000, M = 256, N = 64: A (K x M) is 4.3 GB; each of the 128 k-slices rebases
    its descriptor at `kbeg * lda` (Fetch::plan, MC form).  Probe rows: A is zero except ~80 k-rows (first, last, around byte offsets
    2^31 and 2^32 = k-rows 2^21 and 2^22, random), B is dense: C = A[probe]^T B[probe] exactly, 2e-4 sqrt(probe rows).  Then one
    dense run against the sum of the kernel's own results on three chunks of 1 400 000 k-rows (1.4 GB)."""
    K, M, N = 4200000, 256, 64
    need_device_memory((K * M + K * N) * 4 + GIB)
    A = torch.zeros(K, M, device="cuda")
    Bm = _randn_(torch.empty(K, N, device="cuda"), 2)
    rng = np.random.RandomState(6)
    probe = sorted(set([0, 1, K - 2, K - 1] + boundary_rows(K, M) + [int(v) for v in rng.randint(0, K, size=64)]))
    assert {(1 << 21) - 1, 1 << 21, (1 << 22) - 1, 1 << 22} <= set(probe)
    a_rows = torch.randn(len(probe), M, generator=torch.Generator().manual_seed(1))
    for i, r in enumerate(probe):
        A[r] = a_rows[i].cuda()
    C = torch.empty(M, N, device="cuda")
    _gemm(2, 0, A, M, Bm, N, C, N, M, N, K)
    ref = a_rows.double().T @ _rows(Bm, probe)
    e = _maxerr(C.cpu(), ref)
    print(f"gemm TN probe rows: max err {e:.3e} ({len(probe)} rows)")
    assert e <= 2e-4 * math.sqrt(len(probe))
    _randn_(A, 3)
    _gemm(2, 0, A, M, Bm, N, C, N, M, N, K)
    big = C.double()
    acc = torch.zeros_like(big)
    part = torch.empty(M, N, device="cuda")
    for k0 in range(0, K, 1400000):
        _gemm(2, 0, A[k0:k0 + 1400000], M, Bm[k0:k0 + 1400000], N, part, N, M, N, 1400000)
        acc += part.double()
    assert float((acc - big).abs().max()) <= 2e-3 * float(big.abs().max()) + 1e-8
    del A, Bm


def test_gemm_refuses_what_its_descriptors_cannot_address(amd):
    """The launch checks of gemm_f32: `lda*512 >= 2^31` ("leading dimension too large"), `kchunk * ldb * 4 >= 2 GiB` for an NN
    B operand ("k-chunk x ldb"), and an output leading dimension whose 128-row tile would leave the direct epilogue's 2 GiB window
    ("output leading dimension too large").  Each returns DGVIT_ERR_ARG with a message; the buffers are real and cover everything the
    refused problem would touch."""
    lib = _lib()
    need_device_memory(3 * GIB)
    a = torch.zeros(64, device="cuda")
    w = torch.zeros(4, 32, device="cuda")
    c = torch.zeros(64, device="cuda")
    assert _gemm(0, 0, a, 1 << 22, w, 32, c, 4, 1, 4, 32, check=False) == -1            # M = 1: only row 0 exists
    assert b"leading dimension too large" in lib.dgvit_last_error()
    assert _gemm(0, 0, a, 32, w, 32, c, 1 << 22, 1, 4, 32, check=False) == -1
    assert b"output leading dimension too large" in lib.dgvit_last_error()
    K, ldb = 160, 4000000                                                                # ldb*512 < 2^31, K*ldb*4 = 2.56e9
    bm = torch.zeros(K, ldb, device="cuda")
    a2 = torch.zeros(4, K, device="cuda")
    c2 = torch.zeros(4, 8, device="cuda")
    assert _gemm(1, 0, a2, K, bm, ldb, c2, 8, 4, 8, K, check=False) == -1
    assert b"k-chunk x ldb" in lib.dgvit_last_error()
    del bm


# ------------------------------------------------------------------------------------------------ fp32 attention
def _attn_ref(qkv, H, dh):
    B, N, _ = qkv.shape
    inner = H * dh
    q, k, v = (qkv[..., j * inner:(j + 1) * inner].reshape(B, N, H, dh).permute(0, 2, 1, 3) for j in range(3))
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, N, inner), torch.logsumexp(s, -1) / math.log(2.0)


def test_attention_qkv_past_2_31_elements(amd):
    """dgvit_attention_forward / _backward at B = 28 000, N = 50, H = 8, dh = 64: qkv and dqkv are 2.150e9 floats (8.6 GB), and
    B*H = 224 000 takes the pipelined forward.  Frame offsets `(long long)b * N * ld` past element 2^31 (inside frame 27 962) and byte
    offsets 2^31 / 2^32 (frames 6 990 / 13 981).  out and lse (2e-5) and dqkv (1e-4) of frames 0, 27 999, those around the
    boundaries and 16 random ones against fp64."""
    B, N, H, dh = 28000, 50, 8, 64
    inner = H * dh
    need_device_memory((2 * B * N * 3 * inner + 2 * B * N * inner) * 4 + GIB)
    from dgvit_amd import functional as F
    rng = np.random.RandomState(9)
    frames = sorted(set([0, B - 1] + boundary_rows(B, N * 3 * inner) + [int(v) for v in rng.randint(0, B, size=16)]))
    assert {27961, 27962, 6990, 13981} <= set(frames)
    qkv = _randn_(torch.empty(B, N, 3 * inner, device="cuda"), 1)
    dout = _randn_(torch.empty(B, N, inner, device="cuda"), 2)
    out, lse = F.op_attention_fwd(qkv, H, dh)
    dqkv = F.op_attention_bwd(qkv, out, dout, lse, H, dh)
    qr = _rows(qkv, frames).requires_grad_(True)
    ref, lse_ref = _attn_ref(qr, H, dh)
    ref.backward(_rows(dout, frames))
    eo, el, eg = _maxerr(_rows(out, frames), ref.detach()), _maxerr(_rows(lse, frames), lse_ref.detach()), _maxerr(_rows(dqkv, frames), qr.grad)
    print(f"attention B={B}: out {eo:.3e}, lse {el:.3e}, dqkv {eg:.3e} on {len(frames)} frames")
    assert eo <= 2e-5 and el <= 2e-5
    assert eg <= 1e-4
    del qkv, dout, out, dqkv


def test_tiled_attention_qkv_past_2_gib_below_the_grid_guard(amd):
    """dgvit_attention_forward_tiled / _backward_tiled (attention_long.hip) at B = 7 000, N = 50, H = 8, dh = 64: qkv is 2.15 GB
    (frame 6 990 holds byte 2^31) and B*H*ceil(N/64) = 56 000 stays below the 2^24 guard of check_tiled (the refusal above it is in
    tests/test_large_operands_host.py).  out, lse (2e-5) and dqkv (1e-4) of frames 0, 6 999, those around byte 2^31 and 16 random."""
    B, N, H, dh = 7000, 50, 8, 64
    inner = H * dh
    assert B * N * 3 * inner * 4 > 1 << 31 and B * H < 1 << 24
    need_device_memory((2 * B * N * 3 * inner + 2 * B * N * inner) * 4 + GIB)
    from dgvit_amd import functional as F
    rng = np.random.RandomState(10)
    frames = sorted(set([0, B - 1] + boundary_rows(B, N * 3 * inner) + [int(v) for v in rng.randint(0, B, size=16)]))
    assert {6989, 6990, 6991} <= set(frames)
    qkv = _randn_(torch.empty(B, N, 3 * inner, device="cuda"), 1)
    dout = _randn_(torch.empty(B, N, inner, device="cuda"), 2)
    out, lse = F.op_attention_fwd_tiled(qkv, H, dh)
    dqkv = F.op_attention_bwd_tiled(qkv, out, dout, lse, H, dh)
    qr = _rows(qkv, frames).requires_grad_(True)
    ref, lse_ref = _attn_ref(qr, H, dh)
    ref.backward(_rows(dout, frames))
    eo, el, eg = _maxerr(_rows(out, frames), ref.detach()), _maxerr(_rows(lse, frames), lse_ref.detach()), _maxerr(_rows(dqkv, frames), qr.grad)
    print(f"tiled attention B={B}: out {eo:.3e}, lse {el:.3e}, dqkv {eg:.3e} on {len(frames)} frames")
    assert eo <= 2e-5 and el <= 2e-5
    assert eg <= 1e-4
    del qkv, dout, out, dqkv


# ------------------------------------------------------------------------------------------------ bf16 kernels
def _randn_bf16(shape, seed, scale=1.0):
    """bf16 N(0, scale) device tensor of any size, generated 2^27 elements at a time (the fp32 draw of a chunk is 512 MB)."""
    t = torch.empty(shape, dtype=torch.bfloat16, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    flat = t.view(-1)
    for a in range(0, flat.numel(), 1 << 27):
        n = min(1 << 27, flat.numel() - a)
        flat[a:a + n] = (torch.randn(n, device="cuda", generator=g) * scale).to(torch.bfloat16)
    return t


def _within(what, got, ref, bound):
    frac = float(((got.double() - ref.double()).abs() / bound.double()).max())
    print(f"{what}: max error / bound = {frac:.3f}")
    assert frac <= 1.0, f"{what}: error reaches {frac:.2f} x the bound"


@pytest.mark.parametrize("tile", [0, 256256], ids=["stream", "ring"])
def test_gemm_bf16_a_past_4_gib(amd, tile):
    """dgvit_gemm_bf16 at M = 700 000, K = 3072, N = 768: A is 4.3 GB of bf16 and the fp32 C of epilogue 4 is 2.15 GB.  The stream
    kernel (gemm_bf16_stream.hip: per-tile A / C descriptors rebased at `m0 * lda`, clamped to 0x7FFFFFF0) and, under the
    gemm_bf16_tile knob, the 256 x 256 ring kernel (gemm_bf16.hip).  Epilogues 0 (bf16 + bias), 4 (plain fp32) and 5 (GELU and the
    pre-activation copy) on rows around byte offsets 2^31 and 2^32 of A (rows 349 525 / 699 050) and of C (row 699 050 of the fp32
    output), bounds of helpers.bf16_epilogue_bound."""
    from helpers import bf16_epilogue_bound
    M, K, N = 700000, 3072, 768
    need_device_memory(M * K * 2 + M * N * 4 + M * N * 2 + 2 * GIB)
    lib0 = _lib()
    a = _randn_bf16((M, K), 1)
    b = _randn_bf16((N, K), 2, K ** -0.5)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3)).cuda()
    rows = sampled_rows_for(M, [K * 2, N * 4, N * 2], seed=5)
    assert {349525, 699050} <= set(rows.tolist())
    h = _rows(a, rows) @ b.double().cpu().T
    hb = h + bias.double().cpu()
    with knobs(gemm_bf16_tile=tile):
        lib = _lib()
        for epi in (0, 4, 5):
            c = torch.full((M, N), float("nan"), dtype=torch.float32 if epi == 4 else torch.bfloat16, device="cuda")
            c2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda") if epi == 5 else None
            _ok(lib.dgvit_gemm_bf16(epi, _p(a), K, _p(b), K, _p(c), N, M, N, K, _p(None if epi == 4 else bias), None, 0, _p(c2), N, None, 0,
                                    _st()), "dgvit_gemm_bf16")
            assert not bool(torch.isnan(c).any()), f"epilogue {epi}: output elements left unwritten"
            got = _rows(c, rows)
            if epi == 0:
                _within(f"bf16 gemm {tile} epi 0", got, hb, bf16_epilogue_bound("bf16", hb, K))
            elif epi == 4:
                _within(f"bf16 gemm {tile} epi 4", got, h, bf16_epilogue_bound("f32", h, K))
            else:
                assert not bool(torch.isnan(c2).any())
                g = O.gelu_exact(hb)
                _within(f"bf16 gemm {tile} epi 5 gelu", got, g, bf16_epilogue_bound("gelu", g, K))
                _within(f"bf16 gemm {tile} epi 5 copy", _rows(c2, rows), hb, bf16_epilogue_bound("bf16", hb, K))
            del c, c2
    assert lib0 is _lib()
    del a


def sampled_rows_for(M, row_bytes, seed):
    """sampled_rows with the boundary rows of every operand whose rows are `row_bytes[i]` bytes long"""
    from helpers import sampled_rows
    more = []
    for rb in row_bytes:
        more += boundary_rows(M, rb, itemsize=1)
    return sampled_rows(M, extra=64, seed=seed, more=more)


def test_wgrad_bf16_over_700_000_token_rows(amd):
    """dgvit_wgrad_bf16 at T = 700 000, Mo = 768, Ko = 3072: X is 4.3 GB of bf16, read by the TN ring kernel whose k-slices rebase
    at `k0 * ld` (gemm_bf16.hip set_load_tile), and dY by colsum_bf16_kernel.  Probe rows: dY is zero except ~80 token rows (first,
    last, around byte offsets 2^31 / 2^32 of X = rows 349 525 / 699 050 and of dY, random); X is dense.  dW and db come exactly
    from those rows: bound of test_wgrad_bf16 with T = the rows that contribute."""
    from dgvit_amd import functional as F
    T, Mo, Ko = 700000, 768, 3072
    need_device_memory(T * Ko * 2 + T * Mo * 2 + 2 * GIB)
    x = _randn_bf16((T, Ko), 1)
    dy = torch.zeros(T, Mo, dtype=torch.bfloat16, device="cuda")
    rng = np.random.RandomState(7)
    probe = sorted(set([0, 1, T - 2, T - 1] + boundary_rows(T, Ko * 2, itemsize=1) + boundary_rows(T, Mo * 2, itemsize=1)
                       + [int(v) for v in rng.randint(0, T, size=64)]))
    assert {349525, 699050} <= set(probe)
    d_rows = torch.randn(len(probe), Mo, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    for i, r in enumerate(probe):
        dy[r] = d_rows[i].cuda()
    dw, db = F.op_wgrad_bf16(dy, x, want_bias=True)
    n = len(probe)
    bound = 3e-5 * n ** 0.5 + 1e-6 * n
    ref_w = d_rows.double().T @ _rows(x, probe)
    ew, eb = _maxerr(dw.cpu(), ref_w), _maxerr(db.cpu(), d_rows.double().sum(0))
    print(f"wgrad bf16 probe rows: dW {ew:.3e}, db {eb:.3e}, bound {bound:.3e} ({n} rows)")
    assert ew <= bound and eb <= bound
    del x, dy


def test_layernorm_bf16_past_2_31_elements(amd):
    """dgvit_layernorm_forward_bf16 at 8 400 000 x 256 (fp32 x of 8.6 GB, bf16 y of 4.3 GB): `(long long)row * rs * D` of
    layernorm_fwd_bf16_kernel around rows 2^21, 2^22 (byte offsets of x), 2^23 (element 2^31; byte 2^32 of y).  Bounds of
    test_layernorm_bf16: y 1e-5 + 2^-8 |ref|, mean 1e-5, rstd 1e-5 relative."""
    from dgvit_amd import functional as F
    T, D = 8400000, 256
    need_device_memory(T * D * 6 + 2 * GIB)
    rows = sorted(set(large_rows(T, D, extra=64, seed=1).tolist()) | set(boundary_rows(T, D, itemsize=2)))
    assert {1 << 21, 1 << 22, 1 << 23} <= set(rows)
    x = _randn_(torch.empty(T, D, device="cuda"), 1, scale=2.0, shift=0.5)
    g = (1 + 0.1 * torch.randn(D, generator=torch.Generator().manual_seed(2))).cuda()
    b = (0.1 * torch.randn(D, generator=torch.Generator().manual_seed(3))).cuda()
    y, mean, rstd = F.op_layernorm_bf16(x, g, b)
    xr = _rows(x, rows)
    ref = torch.nn.functional.layer_norm(xr, (D,), g.double().cpu(), b.double().cpu(), 1e-5)
    _within("layernorm bf16 y", _rows(y, rows), ref, 1e-5 + 2 ** -8 * ref.abs())
    assert _maxerr(_rows(mean, rows), xr.mean(-1)) <= 1e-5
    rr = torch.rsqrt(xr.var(-1, unbiased=False) + 1e-5)
    assert float(((_rows(rstd, rows) - rr).abs() / rr).max()) <= 1e-5
    del x, y


def test_attention_bf16_qkv_past_2_32_bytes(amd):
    """dgvit_attention_forward_bf16 (with lse) and _backward_bf16 at B = 4 736, N = 197, H = 12: qkv and dqkv are 4.3 GB.  N <= 224
    with B*H = 56 832 items takes the persistent forward chosen under the `3*H*dh*2*256 < 2^31` condition of attention_bf16.hip.
    Frames around byte offsets 2^31 / 2^32 of qkv (frames 2 365 / 4 731) and of out, frames 0 and 4 735 and a seeded sample, all heads
    of each; bounds of tests/test_gpu_bf16.py (out 6e-3 + 2^-7 |ref|, lse 2e-4, dqkv 6e-2 + 3e-2 |ref|)."""
    from dgvit_amd import functional as F
    B, N, H, dh = 4736, 197, 12, 64
    inner = H * dh
    need_device_memory((2 * B * N * 3 * inner + 3 * B * N * inner) * 2 + 2 * GIB)
    rng = np.random.RandomState(12)
    frames = sorted(set([0, B - 1] + boundary_rows(B, N * 3 * inner * 2, itemsize=1) + boundary_rows(B, N * inner * 2, itemsize=1)
                        + [int(v) for v in rng.randint(0, B, size=6)]))
    assert {2365, 4731} <= set(frames)
    qkv = _randn_bf16((B, N, 3 * inner), 1)
    dout = _randn_bf16((B, N, inner), 2)
    out, lse = F.op_attention_bf16(qkv, H, dh, want_lse=True)
    dqkv = F.op_attention_bwd_bf16(qkv, out, dout, lse, H, dh)
    qr = _rows(qkv, frames).requires_grad_(True)
    ref, lse_ref = _attn_ref(qr, H, dh)
    ref.backward(_rows(dout, frames))
    ref = ref.detach()
    _within("bf16 attention out", _rows(out, frames), ref, 6e-3 + 2 ** -7 * ref.abs())
    el = _maxerr(_rows(lse, frames), lse_ref.detach())
    print(f"bf16 attention lse {el:.3e}")
    assert el <= 2e-4
    _within("bf16 attention dqkv", _rows(dqkv, frames), qr.grad, 6e-2 + 3e-2 * qr.grad.abs())
    del qkv, dout, out, dqkv


# ------------------------------------------------------------------------------------------------ CNN feature stack
def _cnn_params():
    g = torch.Generator().manual_seed(41)
    shapes = [(16, 1, 5, 5), (16,), (64, 16, 5, 5), (64,), (256, 64, 5, 5), (256,)]
    return [(torch.randn(*s, generator=g) * (0.2 if len(s) > 1 else 0.05)) for s in shapes]


def _cnn_ref(params, x):
    x = x[:, None]
    for l in range(3):
        x = torch.relu(torch.nn.functional.conv2d(x, params[2 * l].double(), params[2 * l + 1].double(), stride=2))
    return x.mean(dim=(2, 3))


def _cnn_frames(B, seed):
    """frames 0 and B - 1, those on each side of every byte / element boundary of the three activations and of the im2col column
    matrices (floats per frame in `per`), and a seeded sample"""
    per = [128 * 160, 62 * 78 * 16, 29 * 37 * 64, 13 * 17 * 256, 62 * 78 * 28, 29 * 37 * 400, 13 * 17 * 1600]
    fr = {0, B - 1}
    for p in per:
        fr |= set(boundary_rows(B, p))
    fr |= set(int(v) for v in np.random.RandomState(seed).randint(0, B, size=8))
    return sorted(fr)


@pytest.mark.parametrize("B", [6912, 6944, 7840])
def test_cnn_forward_across_the_im2col_fallbacks(amd, B):
    """dgvit_cnn_forward on 128 x 160 frames.  B = 6 912: conv2 and conv3 gather (implicit GEMM, cnn_api.hip:93-94).  B = 6 944: conv1's
    output reaches 2^29 floats, conv2 falls back to im2col with a 2.98e9-element column matrix (im2col_c4_kernel; A of the GEMM 11.9
    GB).  B = 7 840: conv3 falls back too.  Features of sampled frames against fp64 conv2d (1e-4 of the scale, as
    test_implicit_gemm_convolutions_take_k_slices_at_small_batches), and against the same frames run alone at 1e-5."""
    from dgvit_amd import functional as F
    lib = _lib()
    need = (int(lib.dgvit_cnn_workspace_floats(B, 128, 160)) + int(lib.dgvit_cnn_forward_scratch_floats(B, 128, 160)) + B * 20480) * 4
    need_device_memory(need + 2 * GIB)
    params = _cnn_params()
    dev = [p.cuda() for p in params]
    img = torch.empty(B, 128, 160, device="cuda").uniform_(0, 1, generator=torch.Generator(device="cuda").manual_seed(B))
    frames = _cnn_frames(B, B)
    with torch.no_grad():
        feat = F.cnn_features(img, dev)
        sub = torch.cat([img[f:f + 1] for f in frames])
        alone = F.cnn_features(sub, dev)
    ref = _cnn_ref(params, sub.double().cpu())
    got = _rows(feat, frames)
    scale = max(1.0, float(ref.abs().max()))
    e, ea = _maxerr(got, ref), _maxerr(got, alone.cpu())
    print(f"cnn forward B={B}: vs fp64 {e:.3e}, vs the frames alone {ea:.3e} (scale {scale:.2f}, {len(frames)} frames)")
    assert e <= 1e-4 * scale
    assert ea <= 1e-5 * scale
    assert bool(torch.isfinite(feat).all())
    del img, feat


def test_cnn_backward_with_image_gradient_at_the_conv2_fallback(amd):
    """dgvit_cnn_backward_v2 with dimg at B = 6 944 (conv2 on im2col forward; 16.3 GB of backward scratch).  dimg of sampled frames
    against fp64 autograd (relative L2 1e-4, as test_cnn_image_gradient); every weight and bias gradient of the sum loss against
    the sum of the kernel's own gradients on four chunks of 1 736 frames (the assertion form of test_large_batch_indexing)."""
    from dgvit_amd import functional as F
    B = 6944
    lib = _lib()
    need = (int(lib.dgvit_cnn_workspace_floats(B, 128, 160)) + int(lib.dgvit_cnn_backward_scratch_floats(B, 128, 160))
            + int(lib.dgvit_cnn_forward_scratch_floats(B, 128, 160)) + 3 * B * 20480) * 4
    need_device_memory(need + 2 * GIB)
    params = _cnn_params()
    dev = [p.cuda().requires_grad_(True) for p in params]
    img = torch.empty(B, 128, 160, device="cuda").uniform_(0, 1, generator=torch.Generator(device="cuda").manual_seed(3)).requires_grad_(True)
    w = torch.randn(B, 256, generator=torch.Generator().manual_seed(4)).cuda() / B
    (F.cnn_features(img, dev) * w).sum().backward()
    frames = _cnn_frames(B, 5)
    pr = [p.double().requires_grad_(True) for p in params]
    xr = _rows(img.detach(), frames).requires_grad_(True)
    (_cnn_ref(pr, xr) * _rows(w, frames)).sum().backward()
    got = _rows(img.grad, frames)
    rel = float((got - xr.grad).norm() / xr.grad.norm())
    print(f"cnn backward B={B}: dimg relative L2 error {rel:.3e} on {len(frames)} frames")
    assert rel <= 1e-4
    big = [p.grad.clone() for p in dev]
    acc = [torch.zeros_like(g) for g in big]
    for q in range(4):
        for p in dev:
            p.grad = None
        sl = slice(q * 1736, (q + 1) * 1736)
        (F.cnn_features(img.detach()[sl], dev) * w[sl]).sum().backward()
        for a_, p in zip(acc, dev):
            a_ += p.grad
    for i, (a_, g) in enumerate(zip(acc, big)):
        assert float((a_ - g).abs().max()) <= 2e-3 * float(g.abs().max()) + 1e-8, f"cnn parameter gradient {i}"
    del img, w


# ------------------------------------------------------------------------------------------------ fp32 encoder
def _got_module(amd, cfg, seed):
    params = O.make_params(O.got_param_spec(cfg, prefix=""), seed)
    m = amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=cfg.num_classes, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads,
                mlp_dim=cfg.mlp_dim, channels=1, dim_head=cfg.dim_head, dropout=0.0, emb_dropout=0.0)
    m.load_state_dict(params, strict=True)
    return m.cuda().eval(), params


def _encoder_need(cfg, B, train):
    from dgvit_amd._lib import dgvit_config
    c = dgvit_config(cfg.image[0], cfg.image[1], cfg.patch[0], cfg.patch[1], cfg.dim, cfg.depth, cfg.heads, cfg.dim_head, cfg.mlp_dim)
    lib = _lib()
    n = int(lib.dgvit_got_workspace_floats(ctypes.byref(c), B, 1 if train else 0))
    if train:
        n += int(lib.dgvit_got_backward_scratch_floats(ctypes.byref(c), B))
    return (n + (3 if train else 1) * B * cfg.image[0] * cfg.image[1] + 4 * B * cfg.dim) * 4


def test_encoder_headline_width_with_fc1_output_past_4_gib(amd):
    """dgvit_got_forward / _backward_v3 at the headline width (84 x 84 @ 12, D 256, H 8, M 2048), depth 1, B = 10 496: T = 524 800
    token rows, so the fc1 output and its gradient are 4.3 GB (NT GEMM with C2 past 4 GiB, NN dgelu GEMM with aux past 4 GiB, TN
    weight gradients over 524 800 rows) and qkv is 3.2 GB.  No-grad forward and one training forward + backward with dimg.  Frames 0,
    10 495, those around byte offsets 2^31 / 2^32 of the fc1 output, qkv and the token stream, and a seeded sample against the fp64
    oracle (features 1e-4; dimg relative L2 2e-3 and max-abs 1e-4 of max |ref|, as tests/test_gpu_input_grad.py); parameter
    gradients of the sum loss against the sum over four quarters (the assertion form of test_large_batch_indexing)."""
    cfg = O.GoTConfig(image=(84, 84), patch=(12, 12), dim=256, depth=1, heads=8)
    B, N = 10496, cfg.tokens
    assert B * N * cfg.mlp_dim * 4 > 1 << 32
    need_device_memory(_encoder_need(cfg, B, True) + 2 * GIB)
    m, params = _got_module(amd, cfg, 21)
    gen = torch.Generator(device="cuda").manual_seed(22)
    img = torch.empty(B, 84, 84, device="cuda").uniform_(0, 1, generator=gen)
    goal = torch.empty(B, cfg.dim, device="cuda").normal_(0, 1, generator=gen)
    w = torch.empty(B, cfg.dim, device="cuda").normal_(0, 1, generator=gen) / B
    rng = np.random.RandomState(23)
    frames = {0, B - 1} | set(int(v) for v in rng.randint(0, B, size=8))
    for per in (N * cfg.mlp_dim, N * 3 * cfg.inner, N * cfg.dim):
        frames |= set(boundary_rows(B, per))
    frames = sorted(frames)
    with torch.no_grad():
        feat = m(img, goal)
    pd = {k: v.double() for k, v in params.items()}
    xr = _rows(img, frames).requires_grad_(True)
    ref = O.got_forward(pd, xr, _rows(goal, frames), cfg, prefix="")
    e = _maxerr(_rows(feat, frames), ref.detach())
    print(f"encoder B={B} no-grad: features {e:.3e} on {len(frames)} frames")
    assert e <= 1e-4
    x = img.requires_grad_(True)
    out = m(x, goal)
    (out * w).sum().backward()
    e = _maxerr(_rows(out.detach(), frames), ref.detach())
    assert e <= 1e-4
    (ref * _rows(w, frames)).sum().backward()
    got = _rows(x.grad, frames)
    rel = float((got - xr.grad).norm() / xr.grad.norm())
    mx = float((got - xr.grad).abs().max() / xr.grad.abs().max())
    print(f"encoder B={B} training: features {e:.3e}, dimg rel L2 {rel:.3e}, max-abs / max {mx:.3e}")
    assert rel <= 2e-3 and mx <= 1e-4
    big = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert len(big) >= 10
    acc = {k: torch.zeros_like(g) for k, g in big.items()}
    q4 = B // 4
    for q in range(4):
        m.zero_grad()
        sl = slice(q * q4, (q + 1) * q4)
        (m(img.detach()[sl], goal[sl]) * w[sl]).sum().backward()
        for k, p in m.named_parameters():
            if p.grad is not None:
                acc[k] += p.grad
    for k, g in big.items():
        assert float((acc[k] - g).abs().max()) <= 2e-3 * float(g.abs().max()) + 1e-8, k
    del img, x, feat, out


def test_encoder_patch_gather_falls_back_at_2_29_pixels(amd):
    """128 x 160 @ 16 x 20, D 64, H 2, dh 32, M 64, depth 1.  B = 26 208 (5.37e8 pixels, under 2^29) embeds the patches through the
    gather loader (gemm_tile.h Fetch::plan_gather: one descriptor over the whole 2.15 GB image buffer, unsigned 32-bit byte offsets); B = 26 215
    (2^29 pixels and more: the clamped descriptor would read zeros) must take the patchify fallback of encoder.hip:235.  At both
    batches the last 8 frames agree with the same frames run as a small batch at 2e-5, and frames 0, the last, and those around the
    image buffer's byte offset 2^31 agree with the fp64 oracle at 1e-4."""
    cfg = O.GoTConfig(image=(128, 160), patch=(16, 20), dim=64, depth=1, heads=2, dim_head=32, mlp_dim=64)
    m, params = _got_module(amd, cfg, 31)
    pd = {k: v.double() for k, v in params.items()}
    assert 26208 * 20480 < 1 << 29 <= 26215 * 20480
    need_device_memory(_encoder_need(cfg, 26215, False) + 2 * GIB)
    for B in (26208, 26215):
        gen = torch.Generator(device="cuda").manual_seed(B)
        img = torch.empty(B, 128, 160, device="cuda").uniform_(0, 1, generator=gen)
        goal = torch.empty(B, cfg.dim, device="cuda").normal_(0, 1, generator=gen)
        with torch.no_grad():
            feat = m(img, goal)
            small = m(img[B - 8:].clone(), goal[B - 8:].clone())
        es = _maxerr(feat[B - 8:].cpu(), small.cpu())
        frames = sorted({0, 1, B // 2, B - 9} | set(range(B - 8, B)) | set(boundary_rows(B, 20480)))
        ref = O.got_forward(pd, _rows(img, frames), _rows(goal, frames), cfg, prefix="")
        e = _maxerr(_rows(feat, frames), ref)
        print(f"encoder patch gather B={B}: last 8 frames vs small batch {es:.3e}, {len(frames)} frames vs fp64 {e:.3e}")
        assert es <= 2e-5
        assert e <= 1e-4
        del img, feat
