"""CPU (no GPU): the opt-in for transformer dropout in the bf16 configuration, GoT.set_schedule(dropout_bf16=True) -- host state,
refusals, buffer sizes and the binding of the new entry points.  The kernels are tested in tests/test_gpu_bf16_dropout.py."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import dgvit_amd
    dgvit_amd.load_library()
    return dgvit_amd


def _got(amd, dropout):
    return amd.GoT(image_size=(84, 84), patch_size=(12, 12), num_classes=2, dim=64, depth=2, heads=2, mlp_dim=128, channels=1,
                   dropout=dropout)


def _raise_dropout(m, p):
    for attn, ff in m.transformer.layers:
        attn.fn.dropout.p = attn.fn.to_out[1].p = ff.fn.net[2].p = ff.fn.net[4].p = p


def test_keyword_exists_and_is_documented(amd):
    import inspect
    sig = inspect.signature(amd.GoT.set_schedule)
    assert sig.parameters["dropout_bf16"].default is False
    doc = amd.GoT.set_schedule.__doc__
    assert "dropout_bf16" in doc and "reset by the next call that omits it" in doc
    assert "dropout_bf16" in amd.GoT.set_compute_dtype.__doc__


def test_without_the_keyword_both_orders_refuse_as_before(amd):
    with pytest.raises(NotImplementedError, match="fp32") as e:
        _got(amd, 0.1).set_compute_dtype(torch.bfloat16)
    assert "dropout" in str(e.value) and "dropout_bf16" in str(e.value)
    m = _got(amd, 0.0).set_compute_dtype(torch.bfloat16)
    _raise_dropout(m, 0.2)
    with pytest.raises(NotImplementedError, match="fp32"):
        m(torch.rand(1, 84, 84), torch.randn(1, 64))
    with pytest.raises(NotImplementedError, match="dropout"):
        m.attention_maps(torch.rand(1, 84, 84), torch.randn(1, 64))
    # the other schedule options do not lift it
    with pytest.raises(NotImplementedError, match="dropout"):
        _got(amd, 0.1).set_schedule(long_sequence_bf16=True, dense_last_block=True).set_compute_dtype(torch.bfloat16)


def test_with_the_keyword_both_orders_are_accepted(amd):
    a = _got(amd, 0.1).set_schedule(dropout_bf16=True).set_compute_dtype(torch.bfloat16)      # keyword, then dtype
    assert a.compute_dtype == torch.bfloat16 and a._dropout_bf16 is True
    b = _got(amd, 0.0).set_compute_dtype(torch.bfloat16)                                      # dtype, then keyword, then p
    assert b.set_schedule(dropout_bf16=True) is b
    _raise_dropout(b, 0.2)
    b._check_dropout_dtype(b.compute_dtype)
    assert b.train()._dropout_args(torch.rand(1, 84, 84))[2] == pytest.approx(0.8)
    assert b.eval()._dropout_args(torch.rand(1, 84, 84)) == (1.0, 0, 1.0)
    # a copy keeps the option (DRL.py deep-copies the policy)
    import copy
    assert copy.deepcopy(a)._dropout_bf16 is True and copy.deepcopy(a).compute_dtype == torch.bfloat16


def test_the_next_set_schedule_clears_the_keyword(amd):
    m = _got(amd, 0.1).set_schedule(dropout_bf16=True).set_compute_dtype(torch.bfloat16)
    m.set_schedule()
    assert m._dropout_bf16 is False
    with pytest.raises(NotImplementedError, match="fp32"):
        m(torch.rand(1, 84, 84), torch.randn(1, 64))
    m.set_schedule(dense_last_block=True)                        # another option alone does not bring it back
    with pytest.raises(NotImplementedError, match="dropout"):
        m(torch.rand(1, 84, 84), torch.randn(1, 64))
    m.set_schedule(dense_last_block=True, dropout_bf16=True)
    m._check_dropout_dtype(m.compute_dtype)


def test_keyword_is_a_python_side_no_op_on_an_fp32_model(amd):
    m = _got(amd, 0.1)
    before = m._cfg
    m.set_schedule(dropout_bf16=True)
    assert m._cfg == before and m._cfg[10] == 0 and m.compute_dtype == torch.float32
    for kw in ({"dense_last_block": True}, {"wgrad_overlap": True}, {"long_sequence_bf16": True}):
        flags = _got(amd, 0.0).set_schedule(**kw)._cfg[10]
        assert _got(amd, 0.0).set_schedule(dropout_bf16=True, **kw)._cfg[10] == flags      # dgvit_config.flags has no bit for it


# (config tuple, batch) -> (backward scratch, workspace with save, workspace without) in bytes, recorded on the commit before this option
_SIZES = {
    ((84, 84, 12, 12, 64, 3, 2, 64, 128, 0, 0), 4): (587008, 1585664, 520192),
    ((224, 224, 16, 16, 768, 12, 12, 64, 3072, 0, 0), 8): (75741184, 537026560, 39634944),
}


@pytest.mark.parametrize("key", list(_SIZES), ids=["84p12", "c5"])
def test_buffer_sizes_are_those_of_the_parent(amd, key):
    """Dropout adds no buffer: the masked copies of the branch-output gradients live in the backward's dln buffer while it is free, so
    there is no new size query and the old ones keep their values."""
    from dgvit_amd._lib import dgvit_config
    lib = amd.load_library()
    tup, B = key
    cfg = dgvit_config(*tup)
    got = (lib.dgvit_got_bf16_backward_scratch_bytes(ctypes.byref(cfg), B), lib.dgvit_got_bf16_workspace_bytes(ctypes.byref(cfg), B, 1),
           lib.dgvit_got_bf16_workspace_bytes(ctypes.byref(cfg), B, 0))
    assert got == _SIZES[key]
    header = open(os.path.join(ROOT, "include", "dgvit_hip.h")).read()
    assert len(re.findall(r"\blong long dgvit_got_bf16_\w*(?:scratch|workspace)_bytes\w*\(", header)) == 2


def test_new_symbols_are_bound_and_the_abi_version_stays(amd):
    from dgvit_amd import _lib
    lib = amd.load_library()
    new = ["dgvit_got_forward_bf16_v2", "dgvit_got_forward_maps_bf16_v2", "dgvit_got_backward_bf16_v3", "dgvit_got_backward_bf16_v3_ev",
           "dgvit_attention_forward_bf16_tiled_drop", "dgvit_attention_backward_bf16_tiled_drop", "dgvit_drop_rows_bf16"]
    header = open(os.path.join(ROOT, "include", "dgvit_hip.h")).read()
    for name in new:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and re.search(rf"\bint {name}\(", header), name
    assert lib.dgvit_abi_version() == 7 and "#define DGVIT_ABI_VERSION 7" in header
    # the forms with layer_keep take exactly one float more than the forms without
    for old, v in (("dgvit_got_forward_bf16", "dgvit_got_forward_bf16_v2"), ("dgvit_got_forward_maps_bf16", "dgvit_got_forward_maps_bf16_v2"),
                   ("dgvit_got_backward_bf16_v2", "dgvit_got_backward_bf16_v3"), ("dgvit_got_backward_bf16_v2_ev", "dgvit_got_backward_bf16_v3_ev")):
        a, b = _lib.SIGNATURES[old][1], _lib.SIGNATURES[v][1]
        assert len(b) == len(a) + 1 and b.count(ctypes.c_float) == a.count(ctypes.c_float) + 1


def test_functional_wrappers_check_their_arguments_on_the_host(amd):
    from dgvit_amd import functional as F_
    m = _got(amd, 0.0)
    with pytest.raises(amd.DgvitError, match="layer_dropout_keep"):
        F_.got_encoder_bf16(torch.rand(1, 84, 84), torch.randn(1, 64), m._cfg, m.param_table(), m._bf16_weights, layer_dropout_keep=0.0)
    with pytest.raises(amd.DgvitError, match="layer_dropout_keep"):
        F_.got_attention_maps_bf16(torch.rand(1, 84, 84), torch.randn(1, 64), m._cfg, m.param_table(), m._bf16_weights,
                                   layer_dropout_keep=float("nan"))
    for name in ("op_attention_bf16_tiled_drop", "op_attention_bwd_bf16_tiled_drop", "op_drop_rows_bf16"):
        assert callable(getattr(F_, name))
    with pytest.raises(amd.DgvitError, match="bf16"):
        F_.op_drop_rows_bf16(torch.ones(4, 8), 0.5, 1, 0, 1)
