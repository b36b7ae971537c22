"""CPU: the last block's K / V fold (csrc/last_block.hip) -- the eligibility rule the forward and the backward share
(dgvit_got_last_block_folds), the size queries it must not move, the new entry points' bindings and refusals, and the FLOP model.
The kernels are tested in tests/test_gpu_last_block_fold.py."""
import ctypes

import pytest

from helpers import O  # noqa: F401  (puts the repository root on sys.path)

DENSE, OVERLAP, LONG = 1, 2, 4


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__
    __graft_entry__.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    import dgvit_amd
    return dgvit_amd


def _cfg(image=(84, 84), patch=(12, 12), dim=256, depth=6, heads=8, dim_head=64, mlp_dim=2048, pool_mean=0, flags=0):
    from dgvit_amd._lib import dgvit_config
    return dgvit_config(image[0], image[1], patch[0], patch[1], dim, depth, heads, dim_head, mlp_dim, pool_mean, flags)


def _folds(lib, cfg, batch=512, lkeep=1.0, maps=0):
    return lib.dgvit_got_last_block_folds(ctypes.byref(cfg), batch, lkeep, maps)


def test_bindings_follow_the_header(amd):
    from dgvit_amd import _lib
    I, P, LL, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float
    assert _lib.SIGNATURES["dgvit_goal_attention_scratch_floats"] == (LL, [I, I, I])
    assert _lib.SIGNATURES["dgvit_goal_attention_forward"] == (I, [P, P, P, LL, P, LL, P, P, P, I, I, I, I, I, P])
    assert _lib.SIGNATURES["dgvit_goal_attention_backward"] == (I, [P, P, P, LL, P, LL, P, P, P, P, LL, P, P, P, LL, I, I, I, I, I, P])
    assert _lib.SIGNATURES["dgvit_got_last_block_folds"][1][1:] == [I, F, I]
    assert _lib.DIAG_SIGNATURES["dgvit_set_last_block_fold"] == (None, [I])
    lib = amd.load_library()
    assert lib.dgvit_abi_version() == 7 and not hasattr(lib, "dgvit_set_last_block_fold")
    with amd.diagnostic_library() as dlib:
        assert hasattr(dlib, "dgvit_set_last_block_fold") and hasattr(dlib, "dgvit_goal_attention_forward")


def test_the_fold_runs_where_the_issue_says(amd):
    lib = amd.load_library()
    assert _folds(lib, _cfg()) == 1                                                   # C3
    assert _folds(lib, _cfg(), batch=1) == 1
    assert _folds(lib, _cfg(image=(128, 160), patch=(16, 20), dim=64, depth=4, heads=4)) == 1      # the shipped model
    assert _folds(lib, _cfg(dim=64, heads=1)) == 1                                    # no output projection (H = 1, dh = D)
    assert _folds(lib, _cfg(dim=64, heads=4, dim_head=32)) == 1
    assert _folds(lib, _cfg(flags=OVERLAP)) == 1


def test_the_fold_is_off_where_the_issue_says(amd):
    lib = amd.load_library()
    assert _folds(lib, _cfg(flags=DENSE)) == 0                                        # not the token-0 last block
    assert _folds(lib, _cfg(pool_mean=1)) == 0
    assert _folds(lib, _cfg(), lkeep=0.9) == 0                                        # transformer dropout
    assert _folds(lib, _cfg(), maps=1) == 0                                           # an attention-maps call
    assert _folds(lib, _cfg(image=(224, 224), patch=(14, 14)), batch=2) == 0          # 257 x 256 floats = 263 KB of LDS
    assert _folds(lib, _cfg(image=(136, 168), patch=(8, 8), flags=LONG), batch=2) == 0   # 358 tokens: the K / V-tiled attention
    # the LDS budget (80 KB: two workgroups per CU) sits between 65 and 82 tokens at dim 256, 8 heads
    assert _folds(lib, _cfg(image=(96, 96), patch=(12, 12))) == 1                     # 65 tokens: 70.9 KB
    assert _folds(lib, _cfg(image=(108, 108), patch=(12, 12))) == 0                   # 82 tokens: 89.3 KB
    # u and r must fit behind q in the frame's N x 3I rows of the qkv buffer: dim 1024 with two 32-wide heads and 2 tokens does not
    assert _folds(lib, _cfg(image=(12, 12), patch=(12, 12), dim=1024, heads=2, dim_head=32)) == 0
    # bad configurations are errors, not answers
    assert _folds(lib, _cfg(), batch=0) < 0 and _folds(lib, _cfg(dim_head=48)) < 0


def test_size_queries_do_not_move(amd):
    """u, r and p live in the last layer's qkv / lse slots and du, dr in the dqkv scratch: the workspace and scratch sizes are those of
    the parent commit (figures taken from its library), with or without anything that switches the fold off."""
    lib = amd.load_library()
    want = {  # (image, patch, dim, depth, heads, batch): (workspace save=1, workspace save=0, backward scratch)
        ((84, 84), (12, 12), 256, 6, 8, 512): (1117342848, 204856448, 178870848),
        ((128, 160), (16, 20), 64, 4, 4, 5): (7515992, 2770696, 2210632),
        ((224, 224), (14, 14), 256, 2, 8, 2): (12332240, 8773296, 12411024),
    }
    for (image, patch, dim, depth, heads, B), sizes in want.items():
        for flags in (0, DENSE):
            c = _cfg(image, patch, dim, depth, heads, flags=flags)
            got = (lib.dgvit_got_workspace_floats(ctypes.byref(c), B, 1), lib.dgvit_got_workspace_floats(ctypes.byref(c), B, 0),
                   lib.dgvit_got_backward_scratch_floats(ctypes.byref(c), B))
            assert got == sizes, (image, dim, B, flags, got)
    # what the fold keeps in those slots fits them: p is exactly the lse slot, q + u + r fit a frame's rows of qkv
    B, N, H, D, I = 512, 50, 8, 256, 512
    assert I + 2 * H * D <= N * 3 * I
    assert lib.dgvit_goal_attention_scratch_floats(B, H, D) == 2 * B * H * D <= B * N * 3 * I


def test_operator_refusals_need_no_gpu(amd):
    lib = amd.load_library()
    fake = ctypes.c_void_p(0x1000)
    fwd = lambda B, N, H, dh, D: lib.dgvit_goal_attention_forward(fake, fake, fake, H * dh, fake, H * dh, fake, fake, None, B, N, H, dh, D, None)
    assert fwd(2, 50, 8, 48, 256) != 0 and b"dim_head" in lib.dgvit_last_error()
    assert fwd(2, 50, 8, 64, 258) != 0
    assert fwd(2, 50, 8, 64, 2048) != 0
    assert fwd(2, 257, 8, 64, 256) != 0 and b"LDS" in lib.dgvit_last_error()       # 263 KB
    assert fwd(0, 50, 8, 64, 256) != 0
    assert lib.dgvit_goal_attention_backward(fake, fake, fake, 512, fake, 512, fake, fake, fake, fake, 512, fake, None, fake, 1, 2, 50, 8, 64, 256,
                                             None) != 0 and b"scratch" in lib.dgvit_last_error()
    assert lib.dgvit_goal_attention_scratch_floats(2, 8, 256) == 2 * 2 * 8 * 256
    assert lib.dgvit_goal_attention_scratch_floats(-1, 8, 256) < 0


def test_flop_model_counts_the_folded_last_layer():
    import synthetic
    image, patch, D, L, H, dh, M = (84, 84), (12, 12), 256, 6, 8, 64, 2048
    N, I, P, pd = 50, 512, 49, 144
    layer = 2.0 * N * D * 3 * I + 4.0 * N * N * I + 2.0 * N * I * D + 4.0 * N * D * M
    folded = 3 * 2.0 * D * I + 4.0 * N * H * D + 2.0 * I * D + 4.0 * D * M
    assert synthetic.last_block_folds(N, D, H, dh)
    assert synthetic.fwd_flops_per_frame_executed(image, patch, D, L, H) == 2.0 * P * pd * D + (L - 1) * layer + folded
    # a no-grad forward keeps the K / V GEMM
    kept = 2.0 * N * D * 2 * I + 2.0 * D * I + 4.0 * N * I + 2.0 * I * D + 4.0 * D * M
    assert synthetic.fwd_flops_per_frame_executed(image, patch, D, L, H, training=False) == 2.0 * P * pd * D + (L - 1) * layer + kept
    # the dense-credited figures do not move
    assert synthetic.fwd_flops_per_frame_executed(image, patch, D, L, H, prune_last=False) == synthetic.fwd_flops_per_frame(image, patch, D, L, H)
    assert abs(synthetic.fwd_flops_per_frame(image, patch, D, L, H) / 1e9 - 0.9781) < 1e-3
    # a shape over the LDS budget keeps the K / V GEMM in the count (257 tokens)
    n257 = 257
    assert not synthetic.last_block_folds(n257, 256, 8)
    unfolded = 2.0 * n257 * 256 * 2 * 512 + 2.0 * 256 * 512 + 4.0 * n257 * 512 + 2.0 * 512 * 256 + 4.0 * 256 * 2048
    lay257 = 2.0 * n257 * 256 * 3 * 512 + 4.0 * n257 * n257 * 512 + 2.0 * n257 * 512 * 256 + 4.0 * n257 * 256 * 2048
    assert synthetic.fwd_flops_per_frame_executed((224, 224), (14, 14), 256, 2, 8) == 2.0 * 256 * 196 * 256 + lay257 + unfolded


def test_python_rule_agrees_with_the_library(amd):
    import synthetic
    lib = amd.load_library()
    for image, patch, dim, heads, dh in [((84, 84), (12, 12), 256, 8, 64), ((96, 96), (12, 12), 256, 8, 64), ((108, 108), (12, 12), 256, 8, 64),
                                         ((224, 224), (14, 14), 256, 8, 64), ((128, 160), (16, 20), 64, 4, 64), ((84, 84), (12, 12), 64, 4, 32),
                                         ((12, 12), (12, 12), 1024, 2, 32), ((84, 84), (12, 12), 64, 1, 64)]:
        N = (image[0] // patch[0]) * (image[1] // patch[1]) + 1
        assert _folds(lib, _cfg(image, patch, dim, 2, heads, dh), batch=3) == int(synthetic.last_block_folds(N, dim, heads, dh)), (image, dim, heads, dh)
