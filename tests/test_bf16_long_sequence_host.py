"""CPU (no GPU): the bf16 long-sequence path -- the K / V-tiled bf16 attention entry points (symbols, prototypes, refusals before any
launch), the bf16 size queries with and without DGVIT_FLAG_LONG_SEQUENCE, and GoT.set_schedule(long_sequence_bf16=True).  The kernels
themselves are tested in tests/test_gpu_bf16_long_sequence.py.  Every C call here fails its argument check or only computes a size:
the pointers are never dereferenced."""
import copy
import ctypes

import pytest
import torch

from helpers import O  # noqa: F401  (puts the repository root on sys.path)

LONG = 4
FAKE = ctypes.c_void_p(0x1000)   # non-null, never read: only argument checks run


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd


@pytest.fixture(scope="module")
def lib(amd):
    return amd.load_library()


def _fwd(lib, N, dh=64, nq=None, qkv=FAKE, B=2, H=12):
    return lib.dgvit_attention_forward_bf16_tiled(qkv, FAKE, FAKE, B, N, H, dh, N if nq is None else nq, None)


def _bwd(lib, N, dh=64, nq=None, qkv=FAKE, B=2, H=12):
    return lib.dgvit_attention_backward_bf16_tiled(qkv, FAKE, FAKE, FAKE, FAKE, FAKE, B, N, H, dh, None)


def test_symbols_and_prototypes(amd, lib):
    from dgvit_amd import _lib
    I, P = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["dgvit_attention_forward_bf16_tiled"] == (I, [P, P, P, I, I, I, I, I, P])
    assert _lib.SIGNATURES["dgvit_attention_backward_bf16_tiled"] == (I, [P, P, P, P, P, P, I, I, I, I, P])
    for name in ("dgvit_attention_forward_bf16_tiled", "dgvit_attention_backward_bf16_tiled"):
        fn = getattr(lib, name)
        assert fn.restype is I and list(fn.argtypes) == _lib.SIGNATURES[name][1]
    assert callable(amd.functional.op_attention_bf16_tiled) and callable(amd.functional.op_attention_bwd_bf16_tiled)


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
@pytest.mark.parametrize("N", [0, -1])
def test_refuses_empty_sequences(lib, call, N):
    assert call(lib, N, nq=1) != 0
    assert f"N={N}".encode() in lib.dgvit_last_error()


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
@pytest.mark.parametrize("N", [197, 577])
def test_refuses_dim_head_32(lib, call, N):
    assert call(lib, N, dh=32) != 0
    assert b"dim_head=32" in lib.dgvit_last_error()


@pytest.mark.parametrize("N", [1, 321])
def test_forward_refuses_query_counts_outside_1_to_N(lib, N):
    for nq in (0, N + 1):
        assert _fwd(lib, N, nq=nq) != 0
        msg = lib.dgvit_last_error()
        assert f"nq={nq}".encode() in msg and f"[1, {N}]".encode() in msg, msg


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_refuses_a_null_qkv(lib, call):
    assert call(lib, 321, qkv=None) != 0
    msg = lib.dgvit_last_error()
    assert b"null pointer" in msg and b"qkv=" in msg, msg


@pytest.mark.parametrize("call", [_fwd, _bwd], ids=["forward", "backward"])
def test_refuses_a_grid_of_2_to_the_31_workgroups(lib, call):
    """B * H * ceil(N / block) >= 2^31 with every single argument in range (refused before any launch)"""
    B, H, N = 1 << 20, 64, 1 << 13
    assert call(lib, N, B=B, H=H) != 0
    msg = lib.dgvit_last_error()
    assert b"workgroups" in msg and b"2^31" in msg, msg


def test_fused_entry_points_keep_their_range(lib):
    assert lib.dgvit_attention_forward_bf16(FAKE, FAKE, FAKE, 2, 289, 12, 64, None) != 0
    assert b"N=289 outside [1, 288]" in lib.dgvit_last_error()
    assert lib.dgvit_attention_backward_bf16(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 2, 289, 12, 64, None) != 0
    assert b"N=289 outside [1, 288]" in lib.dgvit_last_error()


def _cfg(flags, image, patch):
    from dgvit_amd._lib import dgvit_config
    return dgvit_config(image[0], image[1], patch[0], patch[1], 768, 12, 12, 64, 3072, 0, flags)


@pytest.mark.parametrize("image,patch,tokens", [((384, 384), (16, 16), 577), ((224, 224), (8, 8), 785)])
def test_bf16_sizes_of_long_shapes_need_the_flag(lib, image, patch, tokens):
    assert (image[0] // patch[0]) * (image[1] // patch[1]) + 1 == tokens
    for save in (0, 1):
        assert lib.dgvit_got_bf16_workspace_bytes(ctypes.byref(_cfg(LONG, image, patch)), 4, save) > 0
        assert lib.dgvit_got_bf16_workspace_bytes(ctypes.byref(_cfg(0, image, patch)), 4, save) < 0
        assert b"288" in lib.dgvit_last_error()
    sc = lib.dgvit_got_bf16_backward_scratch_bytes(ctypes.byref(_cfg(LONG, image, patch)), 4)
    assert sc >= 4 * 12 * tokens * 4     # holds the B*H*N delta floats
    assert lib.dgvit_got_bf16_backward_scratch_bytes(ctypes.byref(_cfg(0, image, patch)), 4) < 0


@pytest.mark.parametrize("image,patch,tokens", [((224, 224), (16, 16), 197), ((256, 256), (16, 16), 257), ((328, 56), (8, 8), 288)])
def test_bf16_sizes_up_to_288_tokens_do_not_change_with_the_flag(lib, image, patch, tokens):
    assert (image[0] // patch[0]) * (image[1] // patch[1]) + 1 == tokens
    for save in (0, 1):
        a = lib.dgvit_got_bf16_workspace_bytes(ctypes.byref(_cfg(0, image, patch)), 8, save)
        b = lib.dgvit_got_bf16_workspace_bytes(ctypes.byref(_cfg(LONG, image, patch)), 8, save)
        assert a == b > 0
    assert (lib.dgvit_got_bf16_backward_scratch_bytes(ctypes.byref(_cfg(0, image, patch)), 8)
            == lib.dgvit_got_bf16_backward_scratch_bytes(ctypes.byref(_cfg(LONG, image, patch)), 8) > 0)


def _got(amd):
    return amd.GoT(image_size=(128, 160), patch_size=(8, 8), num_classes=2, dim=64, depth=2, heads=2, mlp_dim=128, channels=1)


def test_long_sequence_bf16_sets_the_flag_in_either_order(amd):
    m = _got(amd)
    assert m._cfg[10] == 0 and not m.long_sequence()
    assert m.set_schedule(long_sequence_bf16=True) is m
    assert m._cfg[10] == LONG and m.long_sequence()           # on an fp32 model: long_sequence=True
    m.set_compute_dtype(torch.bfloat16)                        # ... and bf16 afterwards is accepted
    assert m.compute_dtype == torch.bfloat16 and m.long_sequence()
    m = _got(amd).set_compute_dtype(torch.bfloat16).set_schedule(long_sequence_bf16=True)
    assert m._cfg[10] == LONG and m.long_sequence() and m.compute_dtype == torch.bfloat16
    m.set_compute_dtype(torch.float32).set_compute_dtype(torch.bfloat16)
    assert m.long_sequence()


def test_long_sequence_bf16_composes_and_is_cleared(amd):
    m = _got(amd).set_compute_dtype(torch.bfloat16)
    m.set_schedule(dense_last_block=True, wgrad_overlap=True, long_sequence_bf16=True)
    assert m._cfg[10] == LONG | 1 | 2
    m.set_schedule(long_sequence=True, long_sequence_bf16=True)
    assert m._cfg[10] == LONG
    m.set_schedule(wgrad_overlap=True)
    assert m._cfg[10] == 2 and not m.long_sequence()
    m.set_schedule(long_sequence_bf16=True).set_schedule()
    assert m._cfg[10] == 0 and not m.long_sequence()
    with pytest.raises(NotImplementedError):                   # the cleared request no longer covers bf16
        m.set_schedule(long_sequence=True)


def test_long_sequence_bf16_survives_deepcopy(amd):
    m = _got(amd).set_compute_dtype(torch.bfloat16).set_schedule(long_sequence_bf16=True, dense_last_block=True)
    c = copy.deepcopy(m)
    assert c._cfg == m._cfg and c.long_sequence() and c.compute_dtype == torch.bfloat16
    c.set_compute_dtype(torch.float32).set_compute_dtype(torch.bfloat16)   # the copy still knows the request covers bf16
    assert c.long_sequence()


def test_long_sequence_alone_still_refuses_bf16_and_names_the_new_keyword(amd):
    for build in (lambda: _got(amd).set_compute_dtype(torch.bfloat16).set_schedule(long_sequence=True),
                  lambda: _got(amd).set_schedule(long_sequence=True).set_compute_dtype(torch.bfloat16)):
        with pytest.raises(NotImplementedError, match="long_sequence_bf16") as e:
            build()
        assert "fp32" in str(e.value) and "288 tokens" in str(e.value) and "256" in str(e.value)
    assert "long_sequence_bf16" in amd.GoT.set_schedule.__doc__


def test_bf16_transformer_dropout_stays_refused(amd):
    m = amd.GoT(image_size=(128, 160), patch_size=(8, 8), num_classes=2, dim=64, depth=2, heads=2, mlp_dim=128, channels=1, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        m.set_schedule(long_sequence_bf16=True).set_compute_dtype(torch.bfloat16)


def test_bounds_hold_for_the_restatement_at_1025_tokens():
    """The bounds the GPU tests take over from 288 tokens (out 6e-3 + 2^-7 |ref|; 1.5e-2 relative L2 and 6e-2 + 3e-2 |ref| per
    gradient) against an fp64 restatement of the kernels that applies their roundings -- P (relative to the row maximum) and dS to bf16
    before the second product, every output to bf16 -- at N = 1025: it must use less than half of each bound, so the bounds say
    something about the kernels' arithmetic and not about the formats."""
    import math
    N, H, DH = 1025, 2, 64
    rb = lambda t: t.float().to(torch.bfloat16).double()   # noqa: E731
    g = torch.Generator().manual_seed(5)
    q, k, v, do = (rb(torch.randn(H, N, DH, generator=g, dtype=torch.float64)) for _ in range(4))
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    dots = (qa @ ka.transpose(-1, -2)) * DH ** -0.5
    ref = torch.softmax(dots, -1) @ va
    (ref * do).sum().backward()
    s = dots.detach()
    e = torch.exp(s - s.amax(-1, keepdim=True))
    out = rb((rb(e) @ v) / e.sum(-1, keepdim=True))
    use = {"out": float(((out - ref.detach()).abs() / (6e-3 + 2 ** -7 * ref.detach().abs())).max())}
    p = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    delta = (do * out).sum(-1, keepdim=True)
    ds = rb(p * (do @ v.transpose(-1, -2) - delta) * DH ** -0.5)
    grads = {"dq": (rb(ds @ k), qa.grad), "dk": (rb(ds.transpose(-1, -2) @ q), ka.grad), "dv": (rb(rb(p).transpose(-1, -2) @ do), va.grad)}
    for name, (got, r) in grads.items():
        use[name + " rel L2"] = float((got - r).norm()) / (1.5e-2 * float(r.norm()) + 1e-3)
        use[name] = float(((got - r).abs() / (6e-2 + 3e-2 * r.abs())).max())
    print("restatement at N=1025, error / bound: " + ", ".join(f"{k} {x:.3f}" for k, x in use.items()))
    assert math.isfinite(sum(use.values()))
    for name, x in use.items():
        assert x < 0.5, f"{name}: the restatement uses {x:.2f} of the bound"
