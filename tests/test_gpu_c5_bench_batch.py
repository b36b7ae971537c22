"""GPU: the bf16 configuration C5 (224x224 @ 16, D 768, 12 layers, 12 heads, MLP 3072) at the batch bench.py times, B = 440
(86 680 token rows = 338 full 256-row panels + 152; the patch GEMM's 86 240 rows = 336 + 224).

Sizes that only occur here: the stream GEMM's L2-budgeted column blocks (QKV: 5 + 4 column tiles, fc1: 3 x 4) dealt over 8 XCD chunks
of a tile count that is not a multiple of 8, the ring kernel for the residual and gelu' epilogues at full M, the 64 x 64 tiles of the
token-0-only last block, 5 280 attention items on the 256-workgroup persistent kernel, weight gradients reduced over 86 680 rows.

Every output buffer is NaN-poisoned before the launch (a skipped tile cannot inherit the right answer from a cached block), operators
are called through the raw C ABI with the production dispatch (tile hint 0), and sampled rows / columns / items are compared with a
float64 CPU reference of the same bf16-rounded operands; the remaining elements are checked to be written (not NaN)."""
import ctypes
import gc
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from helpers import O, C5_BENCH_BATCH, bf16_epilogue_bound, gemm_ref_rows, knobs, sampled_rows  # noqa: E402

B = C5_BENCH_BATCH
NTOK, D, H, DH, MLP = 197, 768, 12, 64, 3072
I = H * DH
T = B * NTOK            # 86 680 token rows
TP = B * (NTOK - 1)     # 86 240 patch rows
C5 = dict(image=(224, 224), patch=(16, 16), dim=D, heads=H, dim_head=DH, mlp_dim=MLP)
NAN16 = -1              # bf16 bit pattern 0xFFFF: a NaN


@pytest.fixture(scope="module")
def lib():
    import dgvit_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return dgvit_amd.load_library()


@pytest.fixture(autouse=True)
def _release_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()        # the B = 440 buffers are several GB: later tests must not inherit them as cached blocks


def _ptr(t, offset_elems=0):
    return ctypes.c_void_p(0 if t is None else t.data_ptr() + offset_elems * t.element_size())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc, what):
    if rc != 0:
        msg = lib.dgvit_last_error()
        raise AssertionError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")


def _randn(shape, seed, scale=1.0, dtype=torch.bfloat16):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(*shape, device="cuda", generator=g) * scale).to(dtype)


def _poison(shape, dtype):
    if dtype == torch.bfloat16:
        return torch.full(shape, NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _report(what, got, ref, bound):
    frac = float(((got.double() - ref).abs() / bound).max())
    print(f"[c5 B={B}] {what}: max error / bound = {frac:.3f}")
    assert frac <= 1.0, f"{what}: error reaches {frac:.2f} x the bound (max abs error {float((got.double() - ref).abs().max()):.3g})"
    return frac


# ------------------------------------------------------------------------------------------------ walk model (which rows to check)
def _xcd_chunk_starts(n):
    """first tile index of each XCD's contiguous chunk of an n-tile walk (xcd_chunk in gemm_bf16*.hip)"""
    q, r = n >> 3, n & 7
    return [x * (q + 1) if x < r else r * (q + 1) + (x - r) * q for x in range(8)]


def _stream_col_blocks(N, K, budget_kb=2048):
    """launch_stream: column blocks of the tile walk for an L2 budget (0 = the older group_m walk)"""
    tiles_n = (N + 255) // 256
    fit = budget_kb * 1024 // (256 * K * 2)
    return 0 if budget_kb <= 0 else 1 if (fit >= tiles_n or fit < 4) else -(-tiles_n // fit)


def _tile_mn(t, M, N, col_blocks, group_m=8):
    """(first row, first column) of walk tile t: tile_mn of the stream kernel; col_blocks == 0 is the group_m walk (also the ring
    kernel's)"""
    tiles_m, tiles_n = (M + 255) // 256, (N + 255) // 256
    if col_blocks > 0:
        wq, wrem = divmod(tiles_n, col_blocks)
        big = tiles_m * (wq + 1)
        if t < wrem * big:
            b, rem = divmod(t, big)
            w, c0 = wq + 1, b * (wq + 1)
        else:
            b, rem = divmod(t - wrem * big, tiles_m * wq)
            w, c0 = wq, wrem * (wq + 1) + b * wq
        return rem // w * 256, (c0 + rem % w) * 256
    g, within = divmod(t, group_m * tiles_n)
    rows = min(group_m, tiles_m - g * group_m)
    return (g * group_m + within % rows) * 256, within // rows * 256


def _boundary_rows(M, N, col_blocks):
    """the first two and last two rows of the tiles either side of each XCD chunk boundary"""
    ntiles = ((M + 255) // 256) * ((N + 255) // 256)
    out = []
    for s in _xcd_chunk_starts(ntiles)[1:]:
        for t in (s - 1, s):
            r0 = _tile_mn(t, M, N, col_blocks)[0]
            out += [r0, r0 + 1, r0 + 254, r0 + 255]
    return out


def test_walk_model_matches_the_bench_shapes():
    """(host arithmetic of the model above, which only picks the rows to check) QKV: two column blocks of 5 + 4 tiles, fc1: three of 4;
    339 x 9 = 3051 tiles over 8 XCD chunks; ragged last panels; every walk visits each tile once"""
    assert _stream_col_blocks(3 * I, D) == 2 and _stream_col_blocks(MLP, D) == 3 and _stream_col_blocks(D, MLP) == 1
    assert T == 338 * 256 + 152 and TP == 336 * 256 + 224
    assert _xcd_chunk_starts(3051)[:4] == [0, 382, 764, 1146] and _xcd_chunk_starts(3051)[-1] == 3051 - 381
    assert _tile_mn(339 * 5 - 1, T, 3 * I, 2) == (338 * 256, 4 * 256) and _tile_mn(339 * 5, T, 3 * I, 2) == (0, 5 * 256)
    for N, blocks in ((3 * I, 2), (MLP, 3), (3 * I, 0)):
        n = 339 * (N // 256)
        assert len({_tile_mn(t, T, N, blocks) for t in range(n)}) == n


# ------------------------------------------------------------------------------------------------ 1. GEMMs at the exact C5 / B = 440 shapes
# (name, M, N, K, epilogue, bias, residual, route): route is what dispatch() picks with tile hint 0 (gemm_bf16.hip): the stream kernel
# takes epilogues 0 / 1 / 5 / 4 without a residual; the residual (2) and gelu' (3) epilogues go to the 256 x 256 ring kernel (>= 512
# tiles); the M = 440 last-block GEMMs to 64 x 64 tiles (< 128 tiles of 128 x 128).
FULL_GEMMS = [
    ("patch embedding (epilogue 2, bias + residual)", TP, D, 256, 2, True, True, "ring"),
    ("qkv", T, 3 * I, D, 0, False, False, "stream"),
    ("to_out", T, D, I, 0, True, False, "stream"),
    ("to_out with an fp32 residual", T, D, I, 2, True, True, "ring"),
    ("fc1 (no-grad GELU)", T, MLP, D, 1, True, False, "stream"),
    ("fc2", T, D, MLP, 0, True, False, "stream"),
    ("fc2 with an fp32 residual", T, D, MLP, 2, True, True, "ring"),
    ("dgrad dln2 = dh1 W1", T, D, MLP, 0, False, False, "stream"),
    ("dgrad dao = dxmid Wo", T, I, D, 0, False, False, "stream"),
    ("dgrad dln1 = dqkv Wqkv", T, D, 3 * I, 0, False, False, "stream"),
]


@pytest.mark.parametrize("name,M,N,K,epi,use_bias,use_res,route", FULL_GEMMS,
                         ids=["patch", "qkv", "to_out", "to_out_res", "fc1_gelu", "fc2", "fc2_res", "dln2", "dao", "dln1"])
def test_gemm_at_bench_batch(lib, name, M, N, K, epi, use_bias, use_res, route):
    seed = M + N + K + epi
    a = _randn((M, K), seed)
    scale = 1.0 if epi == 2 else K ** -0.5
    b = _randn((N, K), seed + 1, scale)
    bias = _randn((N,), seed + 2, dtype=torch.float32) if use_bias else None
    res = _randn((M, N), seed + 3, dtype=torch.float32) if use_res else None
    out_dtype = torch.float32 if epi in (2, 4) else torch.bfloat16
    c = _poison((M, N), out_dtype)
    _check(lib, lib.dgvit_gemm_bf16(epi, _ptr(a), K, _ptr(b), K, _ptr(c), N, M, N, K, _ptr(bias), _ptr(res), N if use_res else 0,
                                    _ptr(None), 0, _ptr(None), 0, _stream()), name)
    assert not bool(torch.isnan(c).any()), f"{name}: output elements left unwritten"
    more = _boundary_rows(M, N, _stream_col_blocks(N, K) if route == "stream" else 0)
    rows = sampled_rows(M, seed=seed, more=more)
    ref = gemm_ref_rows(a, b.double().cpu(), rows, bias)
    if use_res:
        ref = ref + res[rows.cuda()].double().cpu()
    got = c[rows.cuda()].cpu()
    if epi == 1:
        ref = O.gelu_exact(ref)
    kind = {0: "bf16", 1: "gelu", 2: "f32_res", 4: "f32"}[epi]
    _report(f"{name} {M}x{N}x{K}", got, ref, bf16_epilogue_bound(kind, ref, K))


def test_gemm_fc1_gelu2_both_outputs_at_bench_batch(lib):
    """fc1 of the saving forward: GELU output and the pre-activation copy (epilogue 5, stream kernel, three column blocks)"""
    M, N, K = T, MLP, D
    a, b, bias = _randn((M, K), 51), _randn((N, K), 52, K ** -0.5), _randn((N,), 53, dtype=torch.float32)
    c, c2 = _poison((M, N), torch.bfloat16), _poison((M, N), torch.bfloat16)
    _check(lib, lib.dgvit_gemm_bf16(5, _ptr(a), K, _ptr(b), K, _ptr(c), N, M, N, K, _ptr(bias), _ptr(None), 0, _ptr(c2), N,
                                    _ptr(None), 0, _stream()), "fc1 gelu2")
    assert not bool(torch.isnan(c).any()) and not bool(torch.isnan(c2).any())
    rows = sampled_rows(M, seed=5, more=_boundary_rows(M, N, _stream_col_blocks(N, K)))
    h = gemm_ref_rows(a, b.double().cpu(), rows, bias)
    _report("fc1 pre-activation copy", c2[rows.cuda()].cpu(), h, bf16_epilogue_bound("bf16", h, K))
    g = O.gelu_exact(h)
    _report("fc1 GELU", c[rows.cuda()].cpu(), g, bf16_epilogue_bound("gelu", g, K))


def test_gemm_dgelu_with_aux_at_bench_batch(lib):
    """the backward's dh1 = (dxout W2) * gelu'(h1): epilogue 3 with the saved pre-activation as aux, on the ring kernel"""
    M, N, K = T, MLP, D
    a, b, aux = _randn((M, K), 61), _randn((N, K), 62, K ** -0.5), _randn((M, N), 63)
    c = _poison((M, N), torch.bfloat16)
    _check(lib, lib.dgvit_gemm_bf16(3, _ptr(a), K, _ptr(b), K, _ptr(c), N, M, N, K, _ptr(None), _ptr(None), 0, _ptr(None), 0,
                                    _ptr(aux), N, _stream()), "dgelu")
    assert not bool(torch.isnan(c).any())
    rows = sampled_rows(M, seed=6, more=_boundary_rows(M, N, 0))
    x = aux[rows.cuda()].double().cpu()
    dg = 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-x * x / 2) / math.sqrt(2 * math.pi)
    ref = gemm_ref_rows(a, b.double().cpu(), rows) * dg
    _report("dgrad dh1 (gelu' epilogue with aux)", c[rows.cuda()].cpu(), ref, bf16_epilogue_bound("dgelu", ref, K))


def test_gemm_inference_last_block_kv_into_the_qkv_buffer(lib):
    """no-grad last block: K / V of every token written into columns I .. 3I of the (T, 3I) qkv buffer (ldc = 3I != N); the Q
    columns stay untouched"""
    M, N, K = T, 2 * I, D
    a, w = _randn((M, K), 71), _randn((3 * I, K), 72, K ** -0.5)
    qkv = _poison((M, 3 * I), torch.bfloat16)
    _check(lib, lib.dgvit_gemm_bf16(0, _ptr(a), K, _ptr(w, I * K), K, _ptr(qkv, I), 3 * I, M, N, K, _ptr(None), _ptr(None), 0,
                                    _ptr(None), 0, _ptr(None), 0, _stream()), "kv")
    assert bool((qkv[:, :I].view(torch.int16) == NAN16).all()), "the kv GEMM wrote into the Q columns"
    assert not bool(torch.isnan(qkv[:, I:]).any())
    rows = sampled_rows(M, seed=7, more=_boundary_rows(M, N, _stream_col_blocks(N, K)))
    ref = gemm_ref_rows(a, w[I:].double().cpu(), rows)
    _report("last-block K/V (ldc 3I)", qkv[rows.cuda(), I:].cpu(), ref, bf16_epilogue_bound("bf16", ref, K))


LAST_BLOCK = [  # (name, N, K, epilogue, bias, A row stride, C row stride): token 0 of each frame, A rows NTOK tokens apart
    ("last-block q", I, D, 0, False, NTOK * D, NTOK * 3 * I),
    ("last-block to_out", D, I, 0, True, NTOK * I, NTOK * D),
    ("last-block fc1 (GELU)", MLP, D, 1, True, NTOK * D, MLP),
    ("last-block fc2", D, MLP, 0, True, MLP, NTOK * D),
]


@pytest.mark.parametrize("name,N,K,epi,use_bias,lda,ldc", LAST_BLOCK, ids=["q", "to_out", "fc1", "fc2"])
def test_gemm_token0_last_block_at_bench_batch(lib, name, N, K, epi, use_bias, lda, ldc):
    """M = 440 token-0 rows with the row strides of dgvit_got_forward_bf16's pruned last block; every row checked, and the columns
    past N of a strided output stay untouched"""
    M = B
    a = _randn((M, lda), 80 + N + K)
    b = _randn((N, K), 81 + N + K, K ** -0.5)
    bias = _randn((N,), 82, dtype=torch.float32) if use_bias else None
    c = _poison((M, ldc), torch.bfloat16)
    _check(lib, lib.dgvit_gemm_bf16(epi, _ptr(a), lda, _ptr(b), K, _ptr(c), ldc, M, N, K, _ptr(bias), _ptr(None), 0, _ptr(None), 0,
                                    _ptr(None), 0, _stream()), name)
    assert not bool(torch.isnan(c[:, :N]).any())
    if ldc > N:
        assert bool((c[:, N:].view(torch.int16) == NAN16).all()), f"{name}: wrote past column N"
    rows = torch.arange(M)
    ref = gemm_ref_rows(a, b.double().cpu(), rows, bias)
    kind = "bf16"
    if epi == 1:
        ref, kind = O.gelu_exact(ref), "gelu"
    _report(f"{name} {M}x{N}x{K}", c[:, :N].cpu(), ref, bf16_epilogue_bound(kind, ref, K))


WGRADS = [("fc2", D, MLP, True), ("fc1", MLP, D, True), ("to_out", D, I, True), ("qkv", 3 * I, D, False)]


@pytest.mark.parametrize("name,Mo,Ko,use_bias", WGRADS, ids=[w[0] for w in WGRADS])
def test_wgrad_at_bench_batch(lib, name, Mo, Ko, use_bias):
    """dW = dY^T X (split-K slabs + fixed-order reduction) and db = column sums of dY over T = 86 680 token rows.  Checked on sampled
    columns of dW (dW[:, j] = dY^T X[:, j] needs only X[:, j]): both edge columns of every 256-column tile and a seeded sample."""
    dy, x = _randn((T, Mo), 90 + Mo), _randn((T, Ko), 91 + Ko)
    ns = lib.dgvit_wgrad_bf16_scratch_floats(Mo, Ko, T)
    scratch = _poison((max(ns, 4),), torch.float32)
    dw = _poison((Mo, Ko), torch.float32)
    db = _poison((Mo,), torch.float32) if use_bias else None
    _check(lib, lib.dgvit_wgrad_bf16(_ptr(dy), _ptr(x), _ptr(dw), _ptr(db), _ptr(scratch), ns, T, Mo, Ko, _stream()), f"wgrad {name}")
    assert not bool(torch.isnan(dw).any()) and (db is None or not bool(torch.isnan(db).any()))
    cols = set()
    for c0 in range(0, Ko, 256):
        cols |= {c0, c0 + 1, min(Ko, c0 + 256) - 2, min(Ko, c0 + 256) - 1}
    cols |= set(int(j) for j in np.random.RandomState(Ko).randint(0, Ko, size=8))
    cols = torch.tensor(sorted(cols))
    ref_w = torch.zeros(Mo, len(cols), dtype=torch.float64)
    ref_b = torch.zeros(Mo, dtype=torch.float64)
    xc = x[:, cols.cuda()]
    for s in range(0, T, 8192):
        d = dy[s:s + 8192].cpu().double()
        ref_w += d.T @ xc[s:s + 8192].cpu().double()
        ref_b += d.sum(0)
    bound = 3e-5 * T ** 0.5 + 1e-6 * T          # tests/test_gpu_bf16.py test_wgrad_bf16: accumulation over T terms
    _report(f"wgrad {name} dW {Mo}x{Ko} over T={T}", dw[:, cols.cuda()].cpu(), ref_w, torch.full_like(ref_w, bound))
    if use_bias:
        _report(f"wgrad {name} db", db.cpu(), ref_b, torch.full_like(ref_b, bound))


# ------------------------------------------------------------------------------------------------ 2. walk invariance at full M
WALKS = [dict(gemm_bf16_l2_budget_kb=1 << 20),        # one column block
         dict(gemm_bf16_l2_budget_kb=2048),           # the default (QKV 5 + 4, fc1 4 + 4 + 4)
         dict(gemm_bf16_l2_budget_kb=1536),           # QKV 3 + 3 + 3, fc1 4 + 4 + 4
         dict(gemm_bf16_l2_budget_kb=2688),           # QKV 5 + 4, fc1 6 + 6
         dict(gemm_bf16_l2_budget_kb=0, gemm_bf16_group_m=7),    # the older walk: groups of row panels (339 = 48 x 7 + 3)
         dict(gemm_bf16_l2_budget_kb=0, gemm_bf16_group_m=16)]   # (339 = 21 x 16 + 3)


@pytest.mark.parametrize("N", [3 * I, MLP], ids=["qkv", "fc1"])
@pytest.mark.parametrize("epi", [0, 4])
def test_stream_walks_are_bit_identical_at_bench_batch(lib, N, epi):
    """every column-block split of the stream kernel's walk and the older group_m walk compute each tile's sum in the same order:
    bit-identical outputs, each launch into its own freshly poisoned buffer"""
    M, K = T, D
    a, b = _randn((M, K), 100 + N), _randn((N, K), 101 + N, K ** -0.5)
    out_dtype = torch.float32 if epi == 4 else torch.bfloat16
    first = None
    for kw in WALKS:
        with knobs(gemm_bf16_tile=256257, **kw) as walk_lib:
            c = _poison((M, N), out_dtype)
            _check(walk_lib, walk_lib.dgvit_gemm_bf16(epi, _ptr(a), K, _ptr(b), K, _ptr(c), N, M, N, K, _ptr(None), _ptr(None), 0,
                                                      _ptr(None), 0, _ptr(None), 0, _stream()), f"walk {kw}")
            torch.cuda.synchronize()
        assert not bool(torch.isnan(c).any()), f"walk {kw}: tiles left unwritten"
        if first is None:
            first = c
            rows = sampled_rows(M, extra=100, seed=N + epi)
            ref = gemm_ref_rows(a, b.double().cpu(), rows)
            _report(f"stream walk N={N} epi {epi}", c[rows.cuda()].cpu(), ref, bf16_epilogue_bound("f32" if epi == 4 else "bf16", ref, K))
        else:
            assert torch.equal(c.view(torch.int16), first.view(torch.int16)), f"walk {kw}: not bit-identical to {WALKS[0]}"
        del c


# ------------------------------------------------------------------------------------------------ 3. attention at B = 440, H = 12, N = 197
def test_attention_forward_and_backward_at_bench_batch(lib):
    """the persistent forward (5 280 (frame, head) items over 256 workgroups) with lse, and the two-pass backward, against fp64
    softmax attention on sampled items: the first, either side of the first and second 256-item rounds, the start of the last round
    (5 120), the very last (frame 439, head 11) and a seeded sample"""
    qkv = _randn((B, NTOK, 3 * I), 110)
    dout = _randn((B, NTOK, I), 111)
    out = _poison((B, NTOK, I), torch.bfloat16)
    lse = _poison((B, H, NTOK), torch.float32)
    _check(lib, lib.dgvit_attention_forward_bf16(_ptr(qkv), _ptr(out), _ptr(lse), B, NTOK, H, DH, _stream()), "attention forward")
    assert not bool(torch.isnan(out).any()) and bool(torch.isfinite(lse).all())
    dqkv = _poison((B, NTOK, 3 * I), torch.bfloat16)
    delta = _poison((B * H * NTOK,), torch.float32)
    _check(lib, lib.dgvit_attention_backward_bf16(_ptr(qkv), _ptr(out), _ptr(dout), _ptr(lse), _ptr(dqkv), _ptr(delta), B, NTOK, H, DH,
                                                  _stream()), "attention backward")
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(delta).all())
    items = {0, 1, 255, 256, 511, 512, 5119, 5120, B * H - 2, B * H - 1}
    items |= set(int(v) for v in np.random.RandomState(11).randint(0, B * H, size=22))
    worst = {"out": 0.0, "lse": 0.0, "dqkv": 0.0, "dqkv rel L2": 0.0}
    for it in sorted(items):
        f, h = divmod(it, H)
        qv, kv, vv = (qkv[f, :, j * I + h * DH: j * I + (h + 1) * DH].double().cpu() for j in range(3))
        q, k, v = (t.clone().requires_grad_(True) for t in (qv, kv, vv))
        dots = (q @ k.T) * DH ** -0.5
        ref = torch.softmax(dots, -1) @ v
        do = dout[f, :, h * DH:(h + 1) * DH].double().cpu()
        (ref * do).sum().backward()
        o = out[f, :, h * DH:(h + 1) * DH].double().cpu()
        # bounds of tests/test_gpu_bf16.py: bf16 probabilities in P.V and one output rounding; lse in base 2
        b_out = 6e-3 + 2 ** -7 * ref.detach().abs()
        worst["out"] = max(worst["out"], float(((o - ref.detach()).abs() / b_out).max()))
        lref = torch.logsumexp(dots.detach(), -1) / math.log(2.0)
        worst["lse"] = max(worst["lse"], float((lse[f, h].double().cpu() - lref).abs().max() / 2e-4))
        for j, g in enumerate((q.grad, k.grad, v.grad)):
            got = dqkv[f, :, j * I + h * DH: j * I + (h + 1) * DH].double().cpu()
            worst["dqkv"] = max(worst["dqkv"], float(((got - g).abs() / (6e-2 + 3e-2 * g.abs())).max()))
            worst["dqkv rel L2"] = max(worst["dqkv rel L2"], float((got - g).norm()) / (1.5e-2 * float(g.norm()) + 1e-3))
    print(f"[c5 B={B}] attention, {len(items)} items: max error / bound = " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= 1.0, f"attention {k}: {v:.2f} x the bound"


# ------------------------------------------------------------------------------------------------ 4. encoder at B = 440
def _c5_params(depth, seed):
    cfg = O.GoTConfig(depth=depth, **C5)
    return cfg, O.make_params(O.got_param_spec(cfg, prefix=""), seed)


def _c5_model(cfg, params):
    import dgvit_amd
    m = dgvit_amd.GoT(image_size=cfg.image, patch_size=cfg.patch, num_classes=2, dim=cfg.dim, depth=cfg.depth, heads=cfg.heads,
                      mlp_dim=cfg.mlp_dim, dim_head=cfg.dim_head, channels=1)
    m.load_state_dict(params, strict=True)
    return m.cuda().set_compute_dtype(torch.bfloat16)


def test_encoder_forward_12_layers_at_bench_batch():
    """the no-grad forward c5_bf16 times (token-0-only last block): frames 0, 217, 438 and 439 (rows in the last two panels) against
    the oracle's bf16-storage model and its fp32 restatement (bounds of test_encoder_bf16_vs_reference_and_oracle); the same frames at
    other positions of a second 440-frame batch, and alone as a 4-frame batch, give the same bits"""
    cfg, params = _c5_params(12, 4401)
    m = _c5_model(cfg, params).eval()
    img, _, _, _ = O.make_inputs(cfg, B, 4401)
    goal = torch.from_numpy(np.random.RandomState(4402).standard_normal((B, D))).float()
    sel = [0, 217, 438, 439]
    shift = 221
    with torch.no_grad():
        full = m(img.cuda(), goal.cuda())
        rolled = m(torch.roll(img, shift, 0).cuda(), torch.roll(goal, shift, 0).cuda())
        small = m(img[sel].cuda(), goal[sel].cuda())
    assert bool(torch.isfinite(full).all())
    assert torch.equal(rolled[[(s + shift) % B for s in sel]], full[sel]), "a frame's features depend on its position in the batch"
    feat = full[sel].cpu()
    emu = O.got_forward_bf16(params, img[sel], goal[sel], cfg, prefix="")
    p64 = {k: v.double() for k, v in params.items()}
    ref = O.got_forward(p64, img[sel].double(), goal[sel].double(), cfg, prefix="")
    d_emu, d32 = (feat.double() - emu.double()).abs(), (feat.double() - ref).abs()
    d_small = (small.cpu() - feat).abs()
    print(f"[c5 B={B}] forward L12: vs bf16 model max {float(d_emu.max()):.4f} (/2e-2 = {float(d_emu.max()) / 2e-2:.3f}) mean "
          f"{float(d_emu.mean()):.5f} (/3e-3 = {float(d_emu.mean()) / 3e-3:.3f}) | vs fp64 max {float(d32.max()):.4f} "
          f"(/3e-2 = {float(d32.max()) / 3e-2:.3f}) mean {float(d32.mean()):.5f} (/6e-3 = {float(d32.mean()) / 6e-3:.3f}) | "
          f"4-frame batch max diff {float(d_small.max()):.3g}")
    assert d_emu.max() < 2e-2 and d_emu.mean() < 3e-3
    assert d32.max() < 3e-2 and d32.mean() < 6e-3
    # a 4-frame batch runs other GEMM kernels (64 x 64 tiles instead of the stream kernel) and the per-item attention kernel: the
    # same sums in the same k order, so the same bits
    assert torch.equal(small, full[sel]), "a frame's features depend on the batch it is in"


def _philox_mask(amd, seed, batch, rows):
    ones = torch.ones(batch * NTOK * D, device="cuda")
    amd.functional.op_dropout_(ones, seed, 0.9)
    return (ones != 0).float().reshape(batch, NTOK, D)[rows].cpu()


def test_encoder_backward_depth2_selected_frames_match_oracle():
    """train mode as bench.py's forward + backward (dense last block, activations kept, emb dropout live) at B = 440 and the bench
    dims, depth 2: the loss weights are zero except on 8 frames scattered over the batch (frame 439 in the ragged panel), so every
    parameter gradient, dgoal and dimg of the full-batch backward (weight gradients reduced over 86 680 rows) must equal the oracle's
    on those 8 frames alone (relative L2 per tensor < 2e-2, test_encoder_bf16_gradients), and no gradient reaches the other frames"""
    import dgvit_amd
    cfg, params = _c5_params(2, 4403)
    m = _c5_model(cfg, params).train()
    img, _, _, _ = O.make_inputs(cfg, B, 4403)
    rs = np.random.RandomState(4404)
    goal = torch.from_numpy(rs.standard_normal((B, D))).float()
    sel = [0, 1, 129, 130, 255, 256, 438, 439]
    wout = torch.zeros(B, D)
    wout[sel] = torch.from_numpy(rs.standard_normal((len(sel), D))).float()
    torch.manual_seed(4405)
    dseed = dgvit_amd.GoT.draw_dropout_seed()
    torch.manual_seed(4405)                      # the module draws the same seed
    gi, gg = img.cuda().requires_grad_(True), goal.cuda().requires_grad_(True)
    feat = m(gi, gg)
    (feat * wout.cuda()).sum().backward()
    mask = _philox_mask(dgvit_amd, dseed, B, sel)
    assert 0.88 < float(mask.mean()) < 0.92
    ours = {k: (None if v.grad is None else v.grad.cpu()) for k, v in m.named_parameters()}
    dgoal, dimg = gg.grad.cpu(), gi.grad.cpu()
    rest = torch.ones(B, dtype=torch.bool)
    rest[sel] = False
    assert bool(torch.isfinite(dgoal).all()) and bool(torch.isfinite(dimg).all())
    assert float(dgoal[rest].abs().max()) == 0.0 and float(dimg[rest].abs().max()) == 0.0
    worst = {}
    for name, fn in (("fp32", O.got_forward), ("bf16 model", O.got_forward_bf16)):
        ps = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        g = goal[sel].clone().requires_grad_(True)
        x = img[sel].clone().requires_grad_(True)
        (fn(ps, x, g, cfg, drop_mask=mask, prefix="") * wout[sel]).sum().backward()
        errs = {}
        for k, r in ps.items():
            if r.grad is None or float(r.grad.abs().max()) == 0.0:
                assert ours[k] is None or float(ours[k].abs().max()) == 0.0, f"{k} should have no gradient"
                continue
            assert ours[k] is not None, f"{k}: no gradient"
            errs[k] = float((ours[k] - r.grad).norm() / r.grad.norm())
        errs["dgoal"] = float((dgoal[sel] - g.grad).norm() / g.grad.norm())
        errs["dimg"] = float((dimg[sel] - x.grad).norm() / x.grad.norm())
        worst[name] = max(errs.items(), key=lambda kv: kv[1])
    print(f"[c5 B={B}] backward L2, 8 frames: worst relative L2 error vs fp32 {worst['fp32']} , vs bf16 model {worst['bf16 model']} "
          f"(bound 2e-2)")
    assert worst["fp32"][1] < 2e-2 and worst["bf16 model"][1] < 2e-2


def test_encoder_backward_12_layers_full_batch_equals_mean_of_quarters():
    """bench.py's forward + backward exactly (its model, inputs and loss, train mode with emb dropout): every gradient finite.  Then,
    with the embedding dropout off (a mask drawn for 440 frames is not the four masks drawn for 110), the full-batch gradient of every
    parameter equals the mean of the gradients of the four 110-frame quarters within test_large_batch_indexing's bound"""
    import dgvit_amd
    torch.manual_seed(5)
    m = dgvit_amd.GoT(image_size=224, patch_size=16, num_classes=2, dim=D, depth=12, heads=H, mlp_dim=MLP, channels=1)
    m = m.cuda().eval().set_compute_dtype(torch.bfloat16).train()
    g = torch.Generator(device="cpu").manual_seed(5)
    img, goal = torch.rand(B, 224, 224, generator=g).cuda(), torch.randn(B, D, generator=g).cuda()
    tgt = torch.randn(B, D, generator=g).cuda()

    def grads(lo, hi):
        for p_ in m.parameters():
            p_.grad = None
        loss = ((m(img[lo:hi], goal[lo:hi]) - tgt[lo:hi]) ** 2).mean()
        loss.backward()
        assert bool(torch.isfinite(loss))
        return {k: p_.grad.clone() for k, p_ in m.named_parameters() if p_.grad is not None}

    live = grads(0, B)
    assert len(live) == 4 + 12 * 11                      # pos_embedding, patch weight / bias, RMSNorm gain + 11 per layer
    for k, v in live.items():
        assert bool(torch.isfinite(v).all()), k
    del live
    m.dropout.p = 0.0
    full = grads(0, B)
    acc = {k: torch.zeros_like(v) for k, v in full.items()}
    for q in range(4):
        for k, v in grads(q * B // 4, (q + 1) * B // 4).items():
            acc[k] += v / 4
    worst = max(((float((acc[k] - v).abs().max()) / (2e-3 * float(v.abs().max()) + 1e-8), k) for k, v in full.items()))
    print(f"[c5 B={B}] backward L12: full batch vs mean of quarters, worst max error / bound = {worst[0]:.4f} ({worst[1]})")
    assert worst[0] <= 1.0, worst
