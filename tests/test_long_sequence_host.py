"""CPU: the long-sequence schedule flag (DGVIT_FLAG_LONG_SEQUENCE = 4) -- size queries and refusals of the C ABI with and without it,
GoT.set_schedule(long_sequence=True) and the bf16 refusal.  The kernels themselves are tested in tests/test_gpu_long_sequence.py."""
import ctypes

import pytest
import torch

from helpers import O  # noqa: F401  (puts the repository root on sys.path)

LONG = 4


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__
    __graft_entry__.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    import dgvit_amd
    return dgvit_amd


def _cfg(flags, image=(224, 224), patch=(8, 8), dim_head=64):
    from dgvit_amd._lib import dgvit_config
    return dgvit_config(image[0], image[1], patch[0], patch[1], 256, 6, 8, dim_head, 2048, 0, flags)


def test_flag_value_matches_the_header(amd):
    from dgvit_amd import _lib
    assert _lib.FLAG_LONG_SEQUENCE == LONG
    assert _lib.FLAG_LONG_SEQUENCE & (_lib.FLAG_DENSE_LAST_BLOCK | _lib.FLAG_WGRAD_OVERLAP) == 0


def test_785_tokens_are_sized_with_the_flag(amd):
    """224x224 @ 8x8 = 785 tokens: positive workspace and backward scratch with the flag; the backward scratch holds the tiled
    backward's B*H*N delta floats on top of what the same shape would otherwise need."""
    lib = amd.load_library()
    B = 4
    for save in (0, 1):
        assert lib.dgvit_got_workspace_floats(ctypes.byref(_cfg(LONG)), B, save) > 0
    sc = lib.dgvit_got_backward_scratch_floats(ctypes.byref(_cfg(LONG)), B)
    assert sc > B * 785 * 2048
    assert sc >= lib.dgvit_attention_backward_tiled_scratch_floats(B, 785, 8) == B * 8 * 785
    for flags in (LONG | 1, LONG | 2, LONG | 3):
        assert lib.dgvit_got_backward_scratch_floats(ctypes.byref(_cfg(flags)), B) == sc


def test_785_tokens_are_still_refused_without_the_flag(amd):
    lib = amd.load_library()
    for flags in (0, 1, 2, 3):
        assert lib.dgvit_got_workspace_floats(ctypes.byref(_cfg(flags)), 4, 1) < 0
        err = lib.dgvit_last_error()
        assert b"288" in err and b"DGVIT_FLAG_LONG_SEQUENCE" in err and b"long_sequence" in err
        assert lib.dgvit_got_backward_scratch_floats(ctypes.byref(_cfg(flags)), 4) < 0


def test_sizes_up_to_288_tokens_do_not_change_with_the_flag(amd):
    """N <= 288 keeps the fused kernels with the flag set: the same workspace and scratch as without it."""
    lib = amd.load_library()
    for image, patch in (((224, 224), (14, 14)), ((84, 84), (12, 12)), ((128, 160), (16, 20))):
        for save in (0, 1):
            a = lib.dgvit_got_workspace_floats(ctypes.byref(_cfg(0, image, patch)), 8, save)
            b = lib.dgvit_got_workspace_floats(ctypes.byref(_cfg(LONG, image, patch)), 8, save)
            assert a == b > 0
        assert (lib.dgvit_got_backward_scratch_floats(ctypes.byref(_cfg(0, image, patch)), 8)
                == lib.dgvit_got_backward_scratch_floats(ctypes.byref(_cfg(LONG, image, patch)), 8) > 0)


def test_other_limits_stay_with_the_flag(amd):
    lib = amd.load_library()
    assert lib.dgvit_got_workspace_floats(ctypes.byref(_cfg(LONG, dim_head=48)), 4, 1) < 0
    assert b"dim_head" in lib.dgvit_last_error()
    assert lib.dgvit_got_backward_scratch_floats(ctypes.byref(_cfg(LONG, dim_head=48)), 4) < 0
    assert lib.dgvit_got_workspace_floats(ctypes.byref(_cfg(LONG, patch=(7, 7))), 4, 1) > 0      # 32 * 32 + 1 = 1025 tokens
    assert lib.dgvit_got_workspace_floats(ctypes.byref(_cfg(LONG, patch=(6, 6))), 4, 1) < 0      # 224 % 6 != 0
    assert b"divisible by the patch size" in lib.dgvit_last_error()
    assert lib.dgvit_attention_backward_tiled_scratch_floats(0, 785, 8) < 0


def _got(**kw):
    import dgvit_amd
    return dgvit_amd.GoT(image_size=(224, 224), patch_size=(8, 8), num_classes=2, dim=64, depth=2, heads=2, mlp_dim=128, channels=1, **kw)


def test_set_schedule_sets_the_bit_and_keeps_the_others(amd):
    m = _got()
    assert m._cfg[10] == 0 and not m.long_sequence()
    m.set_schedule(long_sequence=True)
    assert m._cfg[10] == LONG and m.long_sequence()
    m.set_schedule(dense_last_block=True, wgrad_overlap=True, long_sequence=True)
    assert m._cfg[10] == LONG | 1 | 2
    m.set_schedule(dense_last_block=True)
    assert m._cfg[10] == 1 and not m.long_sequence()
    m.set_schedule()
    assert m._cfg[10] == 0


def test_bf16_configuration_refuses_long_sequence_in_either_order(amd):
    with pytest.raises(NotImplementedError, match="fp32"):
        _got().set_schedule(long_sequence=True).set_compute_dtype(torch.bfloat16)
    with pytest.raises(NotImplementedError, match="256"):
        _got().set_compute_dtype(torch.bfloat16).set_schedule(long_sequence=True)
    m = _got().set_compute_dtype(torch.bfloat16).set_schedule(wgrad_overlap=True)   # the other options stay allowed
    assert m._cfg[10] == 2 and m.compute_dtype == torch.bfloat16
    m = _got().set_schedule(long_sequence=True).set_compute_dtype(torch.float32)
    assert m.long_sequence()
