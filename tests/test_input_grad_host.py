"""CPU: the C ABI of the frame gradient (dgvit_got_backward_v3[_ev], dgvit_got_backward_bf16_v2[_ev], dgvit_cnn_backward_v2) -- exported and
bound, the size queries unchanged, arguments refused before anything touches a device.  The kernels are tested in
tests/test_gpu_input_grad.py."""
import ctypes

import pytest

from helpers import O  # noqa: F401  (puts the repository root on sys.path)

NEW = ["dgvit_got_backward_v3", "dgvit_got_backward_v3_ev", "dgvit_got_backward_bf16_v2", "dgvit_got_backward_bf16_v2_ev",
       "dgvit_cnn_backward_v2"]


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__
    __graft_entry__.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    import dgvit_amd
    return dgvit_amd


def _cfg(image, patch, dim=256, depth=6, heads=8, dim_head=64, mlp=2048, pool=0, flags=0):
    from dgvit_amd._lib import dgvit_config
    return dgvit_config(image[0], image[1], patch[0], patch[1], dim, depth, heads, dim_head, mlp, pool, flags)


def test_new_symbols_are_exported_and_bound(amd):
    from dgvit_amd import _lib
    lib = amd.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    # one more pointer (dimg) than the entry points they extend
    sig = _lib.SIGNATURES
    assert len(sig["dgvit_got_backward_v3"][1]) == len(sig["dgvit_got_backward_v2"][1]) + 1
    assert len(sig["dgvit_got_backward_v3_ev"][1]) == len(sig["dgvit_got_backward_v2_ev"][1]) + 1
    assert len(sig["dgvit_got_backward_bf16_v2"][1]) == len(sig["dgvit_got_backward_bf16"][1]) + 1
    assert len(sig["dgvit_got_backward_bf16_v2_ev"][1]) == len(sig["dgvit_got_backward_bf16_ev"][1]) + 1
    assert len(sig["dgvit_cnn_backward_v2"][1]) == len(sig["dgvit_cnn_backward"][1]) + 1
    assert lib.dgvit_abi_version() == 7


# the configurations of test_abi_and_host.py and test_long_sequence_host.py with the sizes the library reported before the frame gradient
# existed: (image, patch, dim, depth, heads, dim_head, mlp, flags, batch) -> (workspace save=0, save=1, backward scratch) in floats
SIZES = [
    (((84, 84), (12, 12), 256, 6, 8, 64, 2048, 0, 512), (204856448, 1117342848, 178870848)),
    (((224, 224), (8, 8), 256, 6, 8, 64, 2048, 4, 4), (34185608, 146107768, 44746472)),
    (((224, 224), (14, 14), 256, 6, 8, 64, 2048, 0, 8), (25950832, 99234896, 34683408)),
    (((128, 160), (16, 20), 64, 4, 4, 64, 2048, 0, 32), (14285092, 47748132, 12390308)),
]


def test_size_queries_are_unchanged(amd):
    """The frame gradient needs no scratch of its own: its GEMM reads the packed patch rows the backward already holds and writes the
    caller's dimg.  Every workspace / scratch query returns what it returned before."""
    lib = amd.load_library()
    for (image, patch, dim, depth, heads, dh, mlp, flags, B), want in SIZES:
        c = _cfg(image, patch, dim, depth, heads, dh, mlp, 0, flags)
        got = (lib.dgvit_got_workspace_floats(ctypes.byref(c), B, 0), lib.dgvit_got_workspace_floats(ctypes.byref(c), B, 1),
               lib.dgvit_got_backward_scratch_floats(ctypes.byref(c), B))
        assert got == want, (image, patch, got)
    c = _cfg((224, 224), (16, 16), 768, 12, 12, 64, 3072)      # bf16, test_abi_and_host.py's configuration
    assert lib.dgvit_got_bf16_backward_scratch_bytes(ctypes.byref(c), 64) == 360315904
    assert lib.dgvit_got_bf16_workspace_bytes(ctypes.byref(c), 64, 1) == 4296163328
    assert [lib.dgvit_cnn_backward_scratch_floats(2, H, W) for H, W in ((128, 160), (61, 75), (29, 29))] == [2858912, 1514368, 1311968]
    assert lib.dgvit_cnn_backward_scratch_floats(2, 28, 40) < 0


def _got_v3(lib, cfg, params, grads, dfeat, dimg, ws=1, nws=1 << 40, scratch=1, nsc=1 << 40, B=2):
    P = ctypes.c_void_p
    return lib.dgvit_got_backward_v3(ctypes.byref(cfg), params, grads, P(dfeat), None, P(dimg), P(ws), nws, P(scratch), nsc, B, 1.0, 1.0,
                                     0, None, None)


def test_got_v3_refuses_bad_arguments_without_a_gpu(amd):
    lib = amd.load_library()
    cfg = _cfg((84, 84), (12, 12), 64, 1, 4)
    n = 4 + 11
    fake = (ctypes.c_void_p * n)(*([16] * n))
    none = (ctypes.c_void_p * n)()
    # a null parameter (the patch weight the frame gradient reads among them)
    params = (ctypes.c_void_p * n)(*([16] * n))
    params[1] = None
    assert _got_v3(lib, cfg, params, none, 16, 16) != 0
    assert b"parameter 1 is null" in lib.dgvit_last_error()
    # null dfeat
    assert _got_v3(lib, cfg, fake, none, 0, 16) != 0
    assert b"null pointer" in lib.dgvit_last_error()
    # workspace / scratch too small
    assert _got_v3(lib, cfg, fake, none, 16, 16, nws=4) != 0
    assert b"workspace" in lib.dgvit_last_error()
    # an image that the patches do not tile
    bad = _cfg((84, 84), (16, 20), 64, 1, 4)
    assert _got_v3(lib, bad, fake, none, 16, 16) != 0
    assert b"divisible by the patch size" in lib.dgvit_last_error()


def test_got_bf16_v2_refuses_bad_arguments_without_a_gpu(amd):
    lib = amd.load_library()
    P = ctypes.c_void_p
    cfg = _cfg((84, 84), (12, 12), 64, 1, 4)
    n = 4 + 11
    params = (ctypes.c_void_p * n)(*([256] * n))
    none = (ctypes.c_void_p * n)()
    rc = lib.dgvit_got_backward_bf16_v2(ctypes.byref(cfg), params, None, none, P(256), None, P(256), P(256), P(256), 1 << 40, P(256), 1 << 40,
                                        2, 1.0, 0, None, None)
    assert rc != 0 and b"null pointer" in lib.dgvit_last_error()     # no packed weights
    bad = _cfg((84, 84), (12, 12), 64, 1, 4, dim_head=32)
    rc = lib.dgvit_got_backward_bf16_v2(ctypes.byref(bad), params, P(256), none, P(256), None, P(256), P(256), P(256), 1 << 40, P(256),
                                        1 << 40, 2, 1.0, 0, None, None)
    assert rc != 0 and b"dim_head" in lib.dgvit_last_error()


def test_cnn_v2_refuses_bad_arguments_and_allows_frozen_parameters(amd):
    lib = amd.load_library()
    P = ctypes.c_void_p
    params = (ctypes.c_void_p * 6)(*([16] * 6))
    none = (ctypes.c_void_p * 6)()
    # the old entry point still demands every gradient
    rc = lib.dgvit_cnn_backward(P(16), params, none, P(16), P(16), 1 << 40, P(16), 1 << 40, 2, 64, 64, None)
    assert rc != 0 and b"gradient 0 is null" in lib.dgvit_last_error()
    # the new one refuses null parameters, frames below 29 x 29 and short scratch ...
    params[2] = None
    rc = lib.dgvit_cnn_backward_v2(P(16), params, none, P(16), P(16), P(16), 1 << 40, P(16), 1 << 40, 2, 64, 64, None)
    assert rc != 0 and b"cnn parameter 2 is null" in lib.dgvit_last_error()
    params[2] = 16
    rc = lib.dgvit_cnn_backward_v2(P(16), params, none, P(16), P(16), P(16), 1 << 40, P(16), 1 << 40, 2, 28, 64, None)
    assert rc != 0 and b"29x29" in lib.dgvit_last_error()
    rc = lib.dgvit_cnn_backward_v2(P(16), params, none, P(16), P(16), P(16), 1 << 40, P(16), 4, 2, 64, 64, None)
    assert rc != 0 and b"scratch too small" in lib.dgvit_last_error()
    # ... but not null gradients: (a device-free check -- the call is stopped by the workspace test, after the gradient table passed)
    rc = lib.dgvit_cnn_backward_v2(P(16), params, none, P(16), P(16), P(16), 4, P(16), 1 << 40, 2, 64, 64, None)
    assert rc != 0 and b"gradient" not in lib.dgvit_last_error() and b"workspace or scratch" in lib.dgvit_last_error()
