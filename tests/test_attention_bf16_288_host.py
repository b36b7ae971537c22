"""CPU (no GPU): the bf16 attention entry points take up to 288 tokens, the limit the shared shape check and the fp32 kernels
already have, and refuse more with a message that names it.  Every call here fails its argument check before anything touches
a device: the pointers are never dereferenced."""
import ctypes

import pytest
import torch

FAKE = ctypes.c_void_p(0x1000)   # non-null, never read: only argument checks run


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


def _fwd(lib, N, dh=64):
    return lib.dgvit_attention_forward_bf16(FAKE, FAKE, FAKE, 2, N, 12, dh, None)


def _bwd(lib, N, dh=64):
    return lib.dgvit_attention_backward_bf16(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, N, 12, dh, None)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
@pytest.mark.parametrize("N", [289, 320, 785])
def test_bf16_attention_refuses_more_than_288_tokens(lib, call, N):
    assert call(lib, N) != 0
    msg = lib.dgvit_last_error()
    assert f"N={N}".encode() in msg and b"288" in msg, msg
    assert b"224" not in msg, msg


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
@pytest.mark.parametrize("N", [0, -1])
def test_bf16_attention_refuses_empty_sequences(lib, call, N):
    assert call(lib, N) != 0
    assert b"288" in lib.dgvit_last_error()


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
@pytest.mark.parametrize("N", [197, 257, 288])
def test_bf16_attention_still_refuses_dim_head_32(lib, call, N):
    assert call(lib, N, dh=32) != 0
    assert b"dim_head=32" in lib.dgvit_last_error()


def test_bf16_encoder_size_queries_accept_257_tokens(lib):
    """ViT-B/14 at 224x224 (257 tokens) passes the shape check both configurations share; 289 tokens does not"""
    from dgvit_amd._lib import dgvit_config
    ok = dgvit_config(224, 224, 14, 14, 768, 12, 12, 64, 3072)
    assert lib.dgvit_got_workspace_floats(ctypes.byref(ok), 8, 1) > 0
    bad = dgvit_config(224, 224, 8, 14, 768, 12, 12, 64, 3072)   # 28 x 16 + 1 = 449 tokens
    assert lib.dgvit_got_workspace_floats(ctypes.byref(bad), 8, 1) < 0


def test_long_sequence_message_states_the_bf16_limit():
    import dgvit_amd
    m = dgvit_amd.GoT(image_size=(32, 32), patch_size=(8, 8), num_classes=2, dim=64, depth=1, heads=2, mlp_dim=64, channels=1)
    with pytest.raises(NotImplementedError, match="288 tokens") as e:
        m.set_compute_dtype(torch.bfloat16).set_schedule(long_sequence=True)
    assert "fp32" in str(e.value) and "256" in str(e.value)
    assert "256 tokens" not in m.set_schedule.__doc__ and "288 tokens" in m.set_schedule.__doc__
