"""CPU: the attention-maps entry points of the C ABI (include/dgvit_hip.h: Attention maps) -- exported with the bound signatures, the
ABI version unchanged, and the refusals that need no GPU; GoT.attention_maps' argument checks.  The kernels and the encoder paths are
tested in tests/test_gpu_attention_maps.py."""
import ctypes

import pytest
import torch

from helpers import O  # noqa: F401  (puts the repository root on sys.path)


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__
    __graft_entry__.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    import dgvit_amd
    return dgvit_amd


def _cfg(image=(84, 84), patch=(12, 12), dim_head=64, heads=8, dim=256, flags=0):
    from dgvit_amd._lib import dgvit_config
    return dgvit_config(image[0], image[1], patch[0], patch[1], dim, 2, heads, dim_head, 512, 0, flags)


def _fake(n):
    """non-null dummy host pointers: every call below is refused before anything is dereferenced"""
    buf = (ctypes.c_float * 16)()
    return (ctypes.c_void_p * n)(*([ctypes.addressof(buf)] * n)), ctypes.c_void_p(ctypes.addressof(buf)), buf


def _fwd(lib, cfg, maps, rows, batch=2):
    table, p, _keep = _fake(4 + 11 * 2)
    return lib.dgvit_got_forward_maps(ctypes.byref(cfg), table, p, p, p, maps, rows, p, 1 << 40, batch, 1.0, 1.0, 0, None, None)


def _fwd_bf16(lib, cfg, maps, rows, batch=2):
    table, p, _keep = _fake(4 + 11 * 2)
    return lib.dgvit_got_forward_maps_bf16(ctypes.byref(cfg), table, p, p, p, p, maps, rows, p, 1 << 40, batch, 1.0, 0, None, None)


def test_symbols_signatures_and_abi(amd):
    from dgvit_amd import _lib
    lib = amd.load_library()
    assert lib.dgvit_abi_version() == 7
    for name in ("dgvit_got_forward_maps", "dgvit_got_forward_maps_bf16", "dgvit_attention_probs", "dgvit_attention_probs_bf16"):
        fn = getattr(lib, name)
        ret, args = _lib.SIGNATURES[name]
        assert fn.restype == ret and list(fn.argtypes) == list(args), name
    assert len(_lib.SIGNATURES["dgvit_got_forward_maps"][1]) == 15
    assert len(_lib.SIGNATURES["dgvit_got_forward_maps_bf16"][1]) == 15
    assert (_lib.MAPS_GOAL, _lib.MAPS_ALL) == (0, 1)


def test_bad_rows_and_null_maps_are_refused(amd):
    lib = amd.load_library()
    _, p, _keep = _fake(1)
    for call in (_fwd, _fwd_bf16):
        for rows in (-1, 2, 7):
            assert call(lib, _cfg(), p, rows) == -1
            assert b"rows" in lib.dgvit_last_error()
        assert call(lib, _cfg(), None, 0) == -1
        assert b"null maps" in lib.dgvit_last_error()
    for fn in (lib.dgvit_attention_probs, lib.dgvit_attention_probs_bf16):
        assert fn(p, p, p, 2, 50, 4, 64, 2, None) == -1
        assert b"rows" in lib.dgvit_last_error()
        assert fn(None, p, p, 2, 50, 4, 64, 0, None) == -1
    assert lib.dgvit_attention_probs_bf16(p, p, p, 2, 50, 4, 32, 0, None) == -1
    assert b"dim_head" in lib.dgvit_last_error()


def _forward_error(lib, cfg):
    assert lib.dgvit_got_workspace_floats(ctypes.byref(cfg), 2, 0) < 0
    return lib.dgvit_last_error()


def test_forward_refusals_apply_with_the_same_messages(amd):
    lib = amd.load_library()
    _, p, _keep = _fake(1)
    long_cfg = _cfg(image=(224, 224), patch=(8, 8))            # 785 tokens without DGVIT_FLAG_LONG_SEQUENCE
    want = _forward_error(lib, long_cfg)
    assert b"288" in want
    for rows in (0, 1):
        assert _fwd(lib, long_cfg, p, rows) == -1
        assert lib.dgvit_last_error() == want
        assert _fwd_bf16(lib, long_cfg, p, rows) == -1
        assert lib.dgvit_last_error() == want
    # bf16 with dim_head 32: the bf16 forward's own refusal
    table, q, _k = _fake(4 + 11 * 2)
    c32 = _cfg(dim_head=32)
    assert lib.dgvit_got_forward_bf16(ctypes.byref(c32), table, q, q, q, q, q, 1 << 40, 2, 0, 1.0, 0, None, None) == -1
    want = lib.dgvit_last_error()
    assert b"dim_head" in want
    assert _fwd_bf16(lib, c32, p, 0) == -1
    assert lib.dgvit_last_error() == want
    # batch 0 is the Python layer's (empty tensors); the C ABI refuses it as the forward does
    assert _fwd(lib, _cfg(), p, 0, batch=0) == -1
    assert b"batch" in lib.dgvit_last_error()


def test_got_attention_maps_argument_checks(amd):
    m = amd.GoT(image_size=(84, 84), patch_size=12, num_classes=2, dim=64, depth=2, heads=4, mlp_dim=128)
    img, goal = torch.zeros(2, 84, 84), torch.zeros(2, 64)
    for rows in ("bad", "Goal", None, 0):
        with pytest.raises(ValueError):
            m.attention_maps(img, goal, rows=rows)
    for rows in ("goal", "all"):
        with pytest.raises(amd.DgvitError):
            m.attention_maps(img, goal, rows=rows)
    m.set_compute_dtype(torch.bfloat16)
    with pytest.raises(amd.DgvitError):
        m.attention_maps(img, goal)
