"""CPU (no GPU): the size queries and launch checks on both sides of the size boundaries of DESIGN 3.21 (operands past 2 GiB, 4 GiB and
2^31 elements).

A caller sizes its buffers from these functions, so at a large batch they must return positive 64-bit values (no 32-bit wrap), grow with
the batch, cover at least the operands the header says are stored, and turn negative exactly where the entry point itself refuses
(schedule.h "batch too large", cnn_api.hip "frame too small or batch too large")."""
import ctypes

import pytest

from helpers import O  # noqa: F401  (puts the repository root on sys.path)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


def _cfg(image, patch, dim, depth, heads, dim_head, mlp):
    from dgvit_amd._lib import dgvit_config
    return dgvit_config(image[0], image[1], patch[0], patch[1], dim, depth, heads, dim_head, mlp)


def _strictly_increasing(values):
    return all(a < b for a, b in zip(values, values[1:]))


def test_encoder_size_queries_across_the_boundaries(lib):
    """Headline width (84x84 @ 12, D 256, H 8, M 2048), depth 1: B = 10 496 is T = 524 800 token rows (fc1 output over 4 GiB); the
    `T * max(3I, M) < 2^40` rule of make_dims (schedule.h) flips between B = 10 737 418 and 10 737 419."""
    cfg = _cfg((84, 84), (12, 12), 256, 1, 8, 64, 2048)
    N, I3, M = 50, 3 * 8 * 64, 2048
    batches = [512, 2048, 10495, 10496, 10497, 10737418]
    for save in (0, 1):
        got = [lib.dgvit_got_workspace_floats(ctypes.byref(cfg), b, save) for b in batches]
        assert all(v > 0 for v in got) and _strictly_increasing(got), got
        for b, v in zip(batches, got):
            # stored per the header: with save_for_backward every layer keeps its activations (at least qkv and the MLP hidden);
            # without, one set of buffers that must hold the widest operand
            assert v >= b * N * ((I3 + M) if save else max(I3, M)), (b, save, v)
    sc = [lib.dgvit_got_backward_scratch_floats(ctypes.byref(cfg), b) for b in batches]
    assert all(v > 0 for v in sc) and _strictly_increasing(sc), sc
    for b, v in zip(batches, sc):
        assert v >= b * N * M, (b, v)        # the gradient of the MLP hidden is a temporary of the backward
    assert got[-1] > 1 << 41 and sc[-1] > 1 << 41, "the largest accepted batch needs more than 2^41 floats: a 64-bit value"
    for q in (lib.dgvit_got_workspace_floats(ctypes.byref(cfg), 10737419, 1), lib.dgvit_got_workspace_floats(ctypes.byref(cfg), 10737419, 0),
              lib.dgvit_got_backward_scratch_floats(ctypes.byref(cfg), 10737419)):
        assert q < 0
    assert b"batch too large" in lib.dgvit_last_error()


def test_encoder_size_queries_at_the_token_row_limit(lib):
    """The patch-gather shape (128x160 @ 16x20, D 64, H 2, dh 32, M 64; N = 65): the gather loader is dropped at B*128*160 >= 2^29
    (B = 26 215; 26 208 still gathers), and T = B*65 reaches 2^31 between B = 33 038 209 and 33 038 210, where make_dims refuses."""
    cfg = _cfg((128, 160), (16, 20), 64, 1, 2, 32, 64)
    N, I3, M = 65, 192, 64
    batches = [8, 26208, 26214, 26215, 33038209]
    for save in (0, 1):
        got = [lib.dgvit_got_workspace_floats(ctypes.byref(cfg), b, save) for b in batches]
        assert all(v > 0 for v in got) and _strictly_increasing(got), got
        for b, v in zip(batches, got):
            assert v >= b * N * ((I3 + M) if save else I3), (b, save, v)
    sc = [lib.dgvit_got_backward_scratch_floats(ctypes.byref(cfg), b) for b in batches]
    assert all(v > 0 for v in sc) and _strictly_increasing(sc), sc
    assert 33038209 * N < 1 << 31 <= 33038210 * N
    assert lib.dgvit_got_workspace_floats(ctypes.byref(cfg), 33038210, 1) < 0
    assert lib.dgvit_got_backward_scratch_floats(ctypes.byref(cfg), 33038210) < 0
    assert b"batch too large" in lib.dgvit_last_error()


def test_cnn_size_queries_across_the_im2col_fallbacks(lib):
    """128x160 frames: 77 376 floats per frame after conv1 and 68 672 after conv2, so the 2^29-float guards of dgvit_cnn_forward
    (cnn_api.hip) flip at B = 6 939 (conv2) and B = 7 818 (conv3); the row count of conv1's output reaches 2^31 at B = 444 062."""
    h = [128, 62, 29, 13]
    w = [160, 78, 37, 17]
    assert h[1] * w[1] * 16 == 77376 and h[2] * w[2] * 64 == 68672
    assert 6938 * 77376 < 1 << 29 <= 6939 * 77376 and 7817 * 68672 < 1 << 29 <= 7818 * 68672
    batches = [512, 6912, 6938, 6939, 6944, 7817, 7818, 7840, 444061]
    ws = [lib.dgvit_cnn_workspace_floats(b, 128, 160) for b in batches]
    fs = [lib.dgvit_cnn_forward_scratch_floats(b, 128, 160) for b in batches]
    bs = [lib.dgvit_cnn_backward_scratch_floats(b, 128, 160) for b in batches]
    for vals in (ws, fs, bs):
        assert all(v > 0 for v in vals) and _strictly_increasing(vals), vals
    for b, v_ws, v_fs, v_bs in zip(batches, ws, fs, bs):
        m = [b * h[l] * w[l] for l in range(4)]
        acts = m[1] * 16 + m[2] * 64 + m[3] * 256                         # the three NHWC activations kept for the backward
        cols = max(m[1] * 25, m[2] * 400, m[3] * 1600)                    # the widest im2col column matrix
        assert v_ws >= acts, (b, v_ws)
        assert v_fs >= cols, (b, v_fs)
        assert v_bs >= cols + 2 * max(m[1] * 16, m[2] * 64, m[3] * 256), (b, v_bs)   # columns + an activation gradient in and out
    assert fs[4] > 1 << 31, "the conv2 column matrix at B = 6 944 has 2.98e9 elements"
    assert 444061 * h[1] * w[1] < 1 << 31 <= 444062 * h[1] * w[1]
    for f in (lib.dgvit_cnn_workspace_floats, lib.dgvit_cnn_forward_scratch_floats, lib.dgvit_cnn_backward_scratch_floats):
        assert f(444062, 128, 160) < 0
    assert b"batch too large" in lib.dgvit_last_error()


def test_operator_scratch_queries_at_the_large_shapes(lib):
    """The operator-level scratch sizes at operands past 2^31 elements (8 400 000 x 256 norms, a 4 200 000-row TN GEMM, 700 000 bf16
    token rows).  The column reductions run on a capped number of workgroups (norm.hip: 2048 / 64 partial rows; schedule.h: at most
    512 / tiles split-K slabs), so past the cap the size must not move at all: any wrap of a 32-bit row count would show as a
    different value, small positive ones included.  The sizes that do grow (tiled attention: B*H*N) are checked against that product."""
    D = 256
    ln = [lib.dgvit_layernorm_backward_scratch_floats(r, D) for r in (16384, 1 << 21, 1 << 23, 8400000, (1 << 31) - 1)]
    assert ln == [2048 * 2 * D] * len(ln), ln                                 # one dgamma and one dbeta row per workgroup
    rm = [lib.dgvit_rmsnorm_backward_scratch_floats(r, D) for r in (256, 1 << 23, 8400000, (1 << 31) - 1)]
    assert rm == [64 * D] * len(rm), rm
    slab = 256 * 64 + 256                                                     # dW and the fused column sums of A
    tn = [lib.dgvit_gemm_scratch_floats(2, 256, 64, k) for k in (1 << 15, 1 << 21, 4200000, (1 << 31) - 1)]   # (K + 255 used to wrap in int here: 1 slab)
    assert tn == [128 * slab] * len(tn), tn                                   # 512 / 4 tiles = 128 slabs
    for b in (1, 28000, 41943, 5368710):
        assert lib.dgvit_attention_backward_tiled_scratch_floats(b, 50, 8) == b * 8 * 50
    assert 5368710 * 400 > 1 << 31
    wg = [lib.dgvit_wgrad_bf16_scratch_floats(768, 3072, t) for t in (86680, 700000, (1 << 31) - 8)]
    assert all(v >= 768 * 3072 for v in wg) and wg[0] == wg[1] == wg[2], wg   # at least one fp32 slab; capped like the fp32 one
    assert lib.dgvit_layernorm_backward_scratch_floats(0, D) < 0 and lib.dgvit_rmsnorm_backward_scratch_floats(-1, D) < 0
    assert lib.dgvit_attention_backward_tiled_scratch_floats(0, 50, 8) < 0


def test_bf16_size_queries_at_the_large_attention_batch(lib):
    """ViT-Base width (224x224 @ 16, D 768, H 12, M 3072; N = 197): B = 4 736 makes the bf16 qkv of one layer exceed 2^32 bytes."""
    cfg = _cfg((224, 224), (16, 16), 768, 12, 12, 64, 3072)
    batches = [8, 440, 4735, 4736]
    assert 4736 * 197 * 2304 * 2 > 1 << 32
    for save in (0, 1):
        got = [lib.dgvit_got_bf16_workspace_bytes(ctypes.byref(cfg), b, save) for b in batches]
        assert all(v > 0 for v in got) and _strictly_increasing(got), got
        for b, v in zip(batches, got):
            assert v >= b * 197 * 2 * (12 * (2304 + 3072) if save else 3072), (b, save, v)
    sc = [lib.dgvit_got_bf16_backward_scratch_bytes(ctypes.byref(cfg), b) for b in batches]
    assert all(v > 0 for v in sc) and _strictly_increasing(sc), sc


def _placeholders(n):
    """n distinct 16-byte aligned non-null addresses for calls that must be refused before anything is dereferenced."""
    return [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(n)]


def test_gemm_leading_dimension_refusals(lib):
    """gemm_f32 checks its leading dimensions before anything touches the device: `lda*512 >= 2^31`, an output / residual / aux leading
    dimension whose 128-row tile would leave the direct epilogue's 2 GiB descriptor window, and `kchunk * ldb * 4 >= 2 GiB` for an NN
    B operand all return DGVIT_ERR_ARG with a message.  Without a device the pointers are placeholders (a refused call dereferences
    nothing; a call that is wrongly let through fails in the launch).  With a device they are real buffers that cover everything the
    refused problem would touch, so a regressed check gives a wrong return code, never a stray access."""
    import torch
    device = torch.cuda.is_available()
    if device:
        need = 160 * 4000000 * 4                                     # B of the NN case: 160 k-rows 4 000 000 floats apart
        free, total = torch.cuda.mem_get_info()
        if free < need + (1 << 30):
            pytest.skip(f"needs {need / 2**30:.1f} GiB (+1 GiB slack) of device memory, {free / 2**30:.1f} of {total / 2**30:.1f} GiB free")
        big_b = torch.zeros(160 * 4000000, device="cuda")
        small = torch.zeros(1 << 22, device="cuda")                  # 16 MB: row 0 of every small operand, and the accepted call below
        a, c, b = ctypes.c_void_p(small.data_ptr()), ctypes.c_void_p(small.data_ptr() + (1 << 23)), ctypes.c_void_p(big_b.data_ptr())
    else:
        a, b, c = _placeholders(3)

    def gemm(layout, lda, ldb, ldc, M, N, K, res=None, ldr=0, aux=None, ldaux=0, epi=0):
        return lib.dgvit_gemm(layout, epi, a, lda, b, ldb, c, ldc, M, N, K, None, res, ldr, None, 0, aux, ldaux, None, 0, None)
    big = 1 << 22                                          # 2^22 * 512 = 2^31; M = 1 everywhere: only row 0 of any operand exists
    assert gemm(0, big, 32, 4, 1, 4, 32) == -1
    assert b"gemm: leading dimension too large" in lib.dgvit_last_error()
    assert gemm(0, 32, big, 4, 1, 1, 32) == -1
    assert b"gemm: leading dimension too large" in lib.dgvit_last_error()
    assert gemm(0, 32, 32, big, 1, 4, 32) == -1
    assert b"output leading dimension too large" in lib.dgvit_last_error()
    assert gemm(0, 32, 32, 4, 1, 4, 32, res=c, ldr=big) == -1
    assert b"output leading dimension too large" in lib.dgvit_last_error()
    assert gemm(1, 32, 4, 4, 1, 4, 32, aux=c, ldaux=big, epi=2) == -1
    assert b"output leading dimension too large" in lib.dgvit_last_error()
    assert gemm(1, 160, 4000000, 8, 4, 8, 160) == -1       # ldb*512 < 2^31, but 160 k-rows of it span 2.56e9 bytes
    assert b"k-chunk x ldb" in lib.dgvit_last_error()
    # half the limit passes every argument check: with a device the one-row problem runs, without one the launch itself fails
    assert gemm(0, (big >> 1) + 4, 32, 4, 1, 4, 32) == (0 if device else -2), lib.dgvit_last_error()
    if device:
        torch.cuda.synchronize()
        del big_b, small
        torch.cuda.empty_cache()


def test_bf16_gemm_leading_dimension_refusals(lib):
    """gemm_bf16.hip: `lda` / `ldb` of 2^21 elements or more ("leading dimension too large", the 2^30-byte window of 256 rows), and an
    output leading dimension whose tile leaves the epilogue's 32-bit offsets, on the stream kernel (gemm_bf16_stream.hip launch check;
    no residual) and on the ring kernel (gemm_bf16.hip launch<>; a residual keeps the stream kernel away).  Every call is epilogue 5
    shaped so that the NEXT check would refuse it too (no C2, or ldc2 != ldc): a regressed check cannot reach a launch."""
    a, b, c, c2, res = _placeholders(5)

    def gemm(lda, ldb, ldc, ldc2, M, N, K, c2=None, res=None):
        return lib.dgvit_gemm_bf16(5, a, lda, b, ldb, c, ldc, M, N, K, None, res, N, c2, ldc2, None, 0, None)
    assert gemm(1 << 21, 8, 8, 8, 8, 8, 8) == -1
    assert b"gemm_bf16: leading dimension too large" in lib.dgvit_last_error()
    assert gemm(8, 1 << 21, 8, 8, 8, 8, 8) == -1
    assert b"gemm_bf16: leading dimension too large" in lib.dgvit_last_error()
    assert gemm((1 << 21) - 8, 8, 8, 8, 8, 8, 8) == -1 and b"epilogue 5 needs C2" in lib.dgvit_last_error()   # just under: the next check
    # 8192 x 8192 outputs take the 256 x 256 tiles (1024 of them)
    assert gemm(8, 8, 1 << 22, 8, 8192, 8192, 8, c2=c2) == -1
    assert b"gemm_bf16: output leading dimension too large" in lib.dgvit_last_error()
    assert gemm(8, 8, 1 << 22, 8, 8192, 8192, 8, c2=c2, res=res) == -1
    assert b"gemm_bf16: output leading dimension too large" in lib.dgvit_last_error()
    assert gemm(8, 8, 8192, 1 << 23, 8192, 8192, 8, c2=c2, res=res) == -1
    assert b"gemm_bf16: output leading dimension too large" in lib.dgvit_last_error()
    assert gemm(8, 8, 8192, 8, 8192, 8192, 8, c2=c2) == -1 and b"needs ldc2 == ldc" in lib.dgvit_last_error()  # in range: the next check


def test_tiled_attention_refuses_above_its_grid_guard(lib):
    """attention_long.hip check_tiled: `B*H*ceil(N/64) >= 2^24` ("B*H*N too large") for the forward and the backward.  B = 2^21, H = 8,
    N = 1 is exactly 2^24; B = 2^21 - 1 passes that check.  out / scratch are null, so the check after it refuses as well."""
    q, lse, o, do, dq = _placeholders(5)
    B = 1 << 21
    assert lib.dgvit_attention_forward_tiled(q, None, lse, B, 1, 8, 64, 1, None) == -1
    assert b"attention_fwd_tiled: B*H*N too large" in lib.dgvit_last_error()
    assert lib.dgvit_attention_backward_tiled(q, o, do, lse, dq, None, 0, B, 1, 8, 64, 1, None) == -1
    assert b"attention_bwd_tiled: B*H*N too large" in lib.dgvit_last_error()
    assert lib.dgvit_attention_forward_tiled(q, None, lse, B - 1, 1, 8, 64, 1, None) == -1
    assert b"attention_fwd_tiled: bad arguments" in lib.dgvit_last_error()
    # one frame whose rows do not fit int offsets: N * 3 * H * dh >= 2^31
    assert lib.dgvit_attention_forward_tiled(q, None, lse, 1, 1 << 20, 32, 64, 1, None) == -1
    assert b"B*H*N too large" in lib.dgvit_last_error()


def test_attention_maps_refuse_oversized_grids(lib):
    """attention_maps.hip: `B*H >= 2^31` ("B*H too large"; rows = 7 is invalid too, so the next check would refuse) and, for
    DGVIT_MAPS_ALL, `B*H*query blocks >= 2^31` (N = 288: 3 blocks per head; B*H = 2^30).  The second has no later check; were it
    let through, the launch itself would be rejected: 3 * 2^30 workgroups exceed the 2^31 - 1 a grid dimension can hold."""
    q, lse, pr = _placeholders(3)
    assert lib.dgvit_attention_probs(q, lse, pr, 1 << 28, 50, 8, 64, 7, None) == -1
    assert b"attention maps: B*H too large" in lib.dgvit_last_error()
    assert lib.dgvit_attention_probs_bf16(q, lse, pr, 1 << 28, 50, 8, 64, 7, None) == -1
    assert b"attention maps: B*H too large" in lib.dgvit_last_error()
    assert lib.dgvit_attention_probs(q, lse, pr, 1 << 27, 288, 8, 64, 1, None) == -1
    assert b"attention maps: B*H*query blocks too large" in lib.dgvit_last_error()


def test_encoder_entry_points_refuse_the_batch_by_name(lib):
    """dgvit_got_forward / _backward / _forward_maps at T = B*N >= 2^31 (N = 65, B = 33 038 210) and at T*max(3I, M) >= 2^40 (headline
    width, B = 10 737 419) return DGVIT_ERR_ARG and name the batch; every pointer but the config is null, so the null-pointer check
    that follows make_dims would refuse as well."""
    small = _cfg((128, 160), (16, 20), 64, 1, 2, 32, 64)
    wide = _cfg((84, 84), (12, 12), 256, 1, 8, 64, 2048)
    for cfg, batch in ((small, 33038210), (wide, 10737419)):
        assert lib.dgvit_got_forward(ctypes.byref(cfg), None, None, None, None, None, 0, batch, 0, 1.0, 0, None, None) == -1
        assert b"batch too large" in lib.dgvit_last_error()
        assert lib.dgvit_got_backward(ctypes.byref(cfg), None, None, None, None, None, 0, None, 0, batch, 1.0, 0, None, None) == -1
        assert b"batch too large" in lib.dgvit_last_error()
        assert lib.dgvit_got_forward_maps(ctypes.byref(cfg), None, None, None, None, None, 0, None, 0, batch, 1.0, 1.0, 0, None, None) == -1
        assert b"batch too large" in lib.dgvit_last_error()
    assert lib.dgvit_got_forward(ctypes.byref(small), None, None, None, None, None, 0, 33038209, 0, 1.0, 0, None, None) == -1
    assert b"null pointer" in lib.dgvit_last_error()       # one frame fewer passes the batch check
    assert lib.dgvit_cnn_forward(None, None, None, None, 0, None, 0, 444062, 128, 160, None) == -1
    assert b"batch too large" in lib.dgvit_last_error()
