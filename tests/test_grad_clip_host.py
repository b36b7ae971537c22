"""CPU (no GPU): the gradient-norm clipping entry points (dgvit_grad_sqnorm_partials, dgvit_grad_clip_coef, dgvit_adam_step_scaled,
dgvit_scale_by_device_scalar), their argument checks, and the Python checks in front of them.  Every library call here fails its argument
check before any launch: the pointers are never dereferenced."""
import ctypes
import math
import os
import re

import pytest
import torch

FAKE = ctypes.c_void_p(0x1000)     # non-null, 16-byte aligned, never read: only argument checks run
OFF4 = ctypes.c_void_p(0x1004)     # misaligned by 4 bytes
NAMES = ["dgvit_grad_sqnorm_partials", "dgvit_grad_clip_coef", "dgvit_adam_step_scaled", "dgvit_scale_by_device_scalar"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


def _header():
    from dgvit_amd import _lib as L
    with open(os.path.join(os.path.dirname(L.LIB_PATH), os.pardir, "include", "dgvit_hip.h")) as f:
        return f.read()


def test_symbols_are_exported_and_bound(lib):
    from dgvit_amd import _lib as L
    P, I, LL, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    want = {"dgvit_grad_sqnorm_partials": [P, LL, P, I, P],
            "dgvit_grad_clip_coef": [P, F, P, P],
            "dgvit_adam_step_scaled": [P, P, P, P, LL, F, F, F, F, F, LL, P, P, P],
            "dgvit_scale_by_device_scalar": [P, LL, P, P]}
    assert sorted(want) == sorted(NAMES)
    for path in (L.LIB_PATH, L.DIAG_LIB_PATH):
        raw = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(raw, name), f"{os.path.basename(path)} does not export {name}"
    for name, args in want.items():
        res, got = L.SIGNATURES[name]
        assert res is I and list(got) == args, name


def test_abi_version_is_unchanged(lib):
    assert lib.dgvit_abi_version() == 7


def test_header_declares_the_entry_points_and_the_partials_constant():
    from dgvit_amd import _lib as L
    text = _header()
    for name in NAMES:
        assert f"int {name}(" in text, name
    m = re.search(r"^#define DGVIT_GRAD_NORM_PARTIALS (\d+)$", text, flags=re.M)
    assert m, "DGVIT_GRAD_NORM_PARTIALS is not defined"
    assert int(m.group(1)) in (512, 1024, 2048)
    assert L.GRAD_NORM_PARTIALS == int(m.group(1)), "the binding sizes the scratch from another value than the header"


def _sqnorm(lib, g=FAKE, n=1024, partials=FAKE, accumulate=0):
    return lib.dgvit_grad_sqnorm_partials(g, n, partials, accumulate, None)


def _coef(lib, partials=FAKE, max_norm=1.0, out=FAKE):
    return lib.dgvit_grad_clip_coef(partials, max_norm, out, None)


def _adam(lib, p=FAKE, g=FAKE, m=FAKE, v=FAKE, n=1024, scale=FAKE):
    return lib.dgvit_adam_step_scaled(p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, scale, None)


def _scale(lib, x=FAKE, n=1024, scale=FAKE):
    return lib.dgvit_scale_by_device_scalar(x, n, scale, None)


CASES = [
    (_sqnorm, b"grad_sqnorm_partials", dict(g=None), b"null"),
    (_sqnorm, b"grad_sqnorm_partials", dict(partials=None), b"null"),
    (_sqnorm, b"grad_sqnorm_partials", dict(n=0), b"n=0"),
    (_sqnorm, b"grad_sqnorm_partials", dict(n=-4), b"n=-4"),
    (_sqnorm, b"grad_sqnorm_partials", dict(n=6), b"n=6"),
    (_sqnorm, b"grad_sqnorm_partials", dict(g=OFF4), b"aligned"),
    (_sqnorm, b"grad_sqnorm_partials", dict(partials=OFF4), b"aligned"),
    (_coef, b"grad_clip_coef", dict(partials=None), b"null"),
    (_coef, b"grad_clip_coef", dict(out=None), b"null"),
    (_coef, b"grad_clip_coef", dict(partials=OFF4), b"aligned"),
    (_coef, b"grad_clip_coef", dict(max_norm=0.0), b"max_norm=0"),
    (_coef, b"grad_clip_coef", dict(max_norm=-1.0), b"max_norm=-1"),
    (_coef, b"grad_clip_coef", dict(max_norm=math.nan), b"max_norm="),
    (_coef, b"grad_clip_coef", dict(max_norm=math.inf), b"max_norm=inf"),
    (_adam, b"adam_step_scaled", dict(p=None), b"null"),
    (_adam, b"adam_step_scaled", dict(g=None), b"null"),
    (_adam, b"adam_step_scaled", dict(m=None), b"null"),
    (_adam, b"adam_step_scaled", dict(v=None), b"null"),
    (_adam, b"adam_step_scaled", dict(scale=None), b"grad_scale_dev"),
    (_adam, b"adam_step_scaled", dict(n=0), b"n=0"),
    (_adam, b"adam_step_scaled", dict(n=-4), b"n=-4"),
    (_adam, b"adam_step_scaled", dict(n=6), b"n=6"),
    (_adam, b"adam_step_scaled", dict(p=OFF4), b"aligned"),
    (_adam, b"adam_step_scaled", dict(g=OFF4), b"aligned"),
    (_adam, b"adam_step_scaled", dict(m=OFF4), b"aligned"),
    (_adam, b"adam_step_scaled", dict(v=OFF4), b"aligned"),
    (_scale, b"scale_by_device_scalar", dict(x=None), b"null"),
    (_scale, b"scale_by_device_scalar", dict(scale=None), b"null"),
    (_scale, b"scale_by_device_scalar", dict(n=0), b"n=0"),
    (_scale, b"scale_by_device_scalar", dict(n=-4), b"n=-4"),
    (_scale, b"scale_by_device_scalar", dict(n=6), b"n=6"),
    (_scale, b"scale_by_device_scalar", dict(x=OFF4), b"aligned"),
]


@pytest.mark.parametrize("call, name, kw, word", CASES,
                         ids=[f"{n.decode()}-" + "-".join(f"{k}={'off4' if x is OFF4 else x}" for k, x in kw.items()) for _, n, kw, _ in CASES])
def test_bad_arguments_are_refused_before_any_launch(lib, call, name, kw, word):
    assert call(lib, **kw) != 0
    msg = lib.dgvit_last_error()
    assert name in msg and word in msg, msg


@pytest.mark.parametrize("bad", [0, -1, "1", True, math.nan], ids=repr)
def test_flat_adam_refuses_bad_max_grad_norm(bad):
    """the value is validated before anything touches the parameters: no device, no library"""
    from dgvit_amd.optim import FlatAdam
    with pytest.raises(ValueError, match="max_grad_norm"):
        FlatAdam([torch.nn.Parameter(torch.zeros(4))], max_grad_norm=bad)


def test_flat_adam_takes_max_grad_norm_as_a_plain_attribute():
    """None is the default; a positive number is kept as given (read again on every step)"""
    import inspect
    from dgvit_amd.optim import FlatAdam
    assert inspect.signature(FlatAdam.__init__).parameters["max_grad_norm"].default is None


@pytest.mark.parametrize("norm_type", [1, 1.0, math.inf, "inf"], ids=repr)
def test_clip_grad_norm_refuses_other_norms(norm_type):
    from dgvit_amd.optim import clip_grad_norm_
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match=r"torch\.nn\.utils\.clip_grad_norm_"):
        clip_grad_norm_([p], 1.0, norm_type=norm_type)


def test_clip_grad_norm_refuses_cpu_gradients_and_has_torchs_signature():
    import inspect
    import dgvit_amd
    from dgvit_amd.optim import clip_grad_norm_
    ours = inspect.signature(clip_grad_norm_).parameters
    theirs = inspect.signature(torch.nn.utils.clip_grad_norm_).parameters
    assert list(ours) == list(theirs)
    assert [ours[k].default for k in ours] == [theirs[k].default for k in theirs]
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    with pytest.raises(dgvit_amd.DgvitError, match="no CPU path"):
        clip_grad_norm_([p], 1.0)
    with pytest.raises(dgvit_amd.DgvitError, match="no CPU path"):
        clip_grad_norm_(p, 1.0)
    lin = torch.nn.Linear(3, 2)
    lin(torch.ones(1, 3)).sum().backward()
    with pytest.raises(dgvit_amd.DgvitError, match="no CPU path"):
        clip_grad_norm_(lin, 1.0)
    # no gradients at all: a zero tensor, as torch returns
    q = torch.nn.Parameter(torch.ones(4))
    assert clip_grad_norm_([q], 1.0).item() == 0.0
