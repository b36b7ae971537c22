"""CPU: the CNN critic / actor on frame stacks -- constructor and input checks of QNetwork / GaussianPolicy with
``frame_channels=K``, state-dict keys and shapes, the ``_v2`` sizing functions, header / binding / library agreement, and the
exactness bound of the parity data (tests/cnn_stack_ref.py).  The kernels are tested in tests/test_gpu_cnn_frame_channels.py."""
import ctypes
import os
import re

import pytest
import torch

from helpers import O, ROOT
import cnn_stack_ref as R

NEW = {"dgvit_cnn_workspace_floats_v2": "dgvit_cnn_workspace_floats", "dgvit_cnn_forward_scratch_floats_v2": "dgvit_cnn_forward_scratch_floats",
       "dgvit_cnn_backward_scratch_floats_v2": "dgvit_cnn_backward_scratch_floats", "dgvit_cnn_forward_v2": "dgvit_cnn_forward",
       "dgvit_cnn_backward_v3": "dgvit_cnn_backward_v2"}
SIZING = [n for n in NEW if "floats" in n]


@pytest.fixture(scope="module")
def amd():
    import __graft_entry__
    __graft_entry__.build()          # hipcc cross-compiles gfx950 without a GPU; no-op when up to date
    import dgvit_amd
    return dgvit_amd


def _nets(amd, **kw):
    return [amd.QNetwork(2, 2, **kw), amd.GaussianPolicy(2, 2, **kw)]


@pytest.mark.parametrize("bad", [0, 17, 2.5, True], ids=repr)
def test_frame_channels_is_validated(amd, bad):
    for cls in (amd.QNetwork, amd.GaussianPolicy):
        with pytest.raises(ValueError, match="frame_channels"):
            cls(2, 2, frame_channels=bad)
    with pytest.raises(TypeError):
        amd.QNetwork(2, 2, 4)            # keyword-only: the positional signature is the reference's


def test_state_dict_keys_and_shapes(amd):
    for net, spec in zip(_nets(amd, frame_channels=1), (O.cnn_qnet_param_spec(), O.cnn_policy_param_spec())):
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == [(n, tuple(s)) for n, s, _ in spec]
    for plain, k1, k4 in zip(_nets(amd), _nets(amd, frame_channels=1), _nets(amd, frame_channels=4)):
        assert k4.frame_channels == 4 and k1.frame_channels == 1 and plain.frame_channels == 1
        sd1, sd4 = plain.state_dict(), k4.state_dict()
        assert list(sd1) == list(sd4) == list(k1.state_dict())
        assert tuple(sd4["conv1.weight"].shape) == (16, 4, 5, 5) and isinstance(k4.conv1, torch.nn.Conv2d)
        assert all(sd1[k].shape == sd4[k].shape for k in sd1 if k != "conv1.weight")
    for kind, net in zip(("qnet", "policy"), _nets(amd, frame_channels=5)):
        net.load_state_dict(R.exact_params(kind, 5), strict=True)


def test_wrong_input_shapes_are_refused_before_touching_a_device(amd):
    """CPU tensors throughout: a shape check that came after the device check would raise DgvitError instead"""
    K = 4
    ps, a = torch.zeros(3, 2), torch.zeros(3, 2)
    for net in _nets(amd, frame_channels=K):
        def call(x):
            return net([x, ps, a]) if isinstance(net, amd.QNetwork) else net([x, ps])
        for bad in (torch.zeros(3, K, 29, 31),                                   # channel-first
                    torch.zeros(3, K, 29, 31).permute(0, 2, 3, 1),               # the right shape, not contiguous
                    torch.zeros(3, 29, 31, K + 1), torch.zeros(3, 29, 31, 1),    # another K
                    torch.zeros(3, 29, 31)):                                     # single frames
            with pytest.raises(ValueError, match=r"\(B, H, W, 4\).*permute\(0, 2, 3, 1\)\.contiguous\(\)"):
                call(bad)
        with pytest.raises(ValueError, match="not contiguous"):
            call(torch.zeros(3, K, 29, 31).permute(0, 2, 3, 1))
        if not isinstance(net, amd.QNetwork):
            with pytest.raises(ValueError, match="frame_channels=4"):
                net.sample([torch.zeros(3, K, 29, 31), ps])
    with pytest.raises(amd.DgvitError):      # the right shape goes on to the device check: no CPU fallback
        _nets(amd, frame_channels=K)[0]([torch.zeros(3, 29, 31, K), ps, a])


def test_v2_sizing_functions(amd):
    lib = amd.load_library()
    shapes = [(1, 29, 29), (2, 128, 160), (3, 30, 37), (33, 61, 75), (512, 128, 160), (7, 84, 84)]
    for new in SIZING:
        f2, f1 = getattr(lib, new), getattr(lib, NEW[new])
        for B, H, W in shapes:
            assert f2(B, H, W, 1) == f1(B, H, W) > 0, (new, B, H, W)
            sizes = [f2(B, H, W, C) for C in range(1, 17)]
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (new, B, H, W, sizes)
            for C in (0, 17, -1):
                assert f2(B, H, W, C) == -1, (new, C)
                assert b"frame channels" in lib.dgvit_last_error()
        assert f2(2, 28, 40, 4) == -1 and f2(0, 64, 64, 4) == -1
    # the column matrix of the backward: M1 * al4(25 C) floats, and conv1's packed weight and its gradient
    B, H, W = 512, 128, 160
    M1 = B * 62 * 78
    for C, kp in ((1, 28), (3, 76), (4, 100), (16, 400)):
        assert lib.dgvit_cnn_backward_scratch_floats_v2(B, H, W, C) >= M1 * kp + 2 * 16 * kp
    grow = lib.dgvit_cnn_backward_scratch_floats_v2(B, H, W, 16) - lib.dgvit_cnn_backward_scratch_floats_v2(B, H, W, 8)
    assert grow >= M1 * 200
    assert lib.dgvit_cnn_workspace_floats_v2(B, H, W, 16) == lib.dgvit_cnn_workspace_floats(B, H, W)     # the activations do not depend on C


def test_header_binding_and_library_agree(amd):
    from dgvit_amd import _lib
    lib = amd.load_library()
    header = open(os.path.join(ROOT, "include", "dgvit_hip.h")).read()
    for new, old in NEW.items():
        res, args = _lib.SIGNATURES[new]
        ores, oargs = _lib.SIGNATURES[old]
        assert hasattr(lib, new) and hasattr(lib, old)
        m = re.search(rf"\b(long long|int) {new}\(([^;]*)\);", header)
        assert m, f"{new} is not declared in dgvit_hip.h"
        assert res is ores and res is (ctypes.c_longlong if m.group(1) == "long long" else ctypes.c_int)
        decl = [p.strip() for p in m.group(2).replace("\n", " ").split(",")]
        assert len(decl) == len(args) == len(oargs) + 1, new
        # `int C` follows `int W`
        w = decl.index("int W")
        assert decl[w + 1] == "int C" and args[w + 1] is ctypes.c_int
        assert args[:w + 1] == oargs[:w + 1] and args[w + 2:] == oargs[w + 1:]
        fn = getattr(lib, new)
        assert fn.restype is res and list(fn.argtypes) == args
    assert "channel-last" in header.lower() or "CHANNEL-LAST" in header
    assert "(16, C, 5, 5)" in header and "(B, H, W, C)" in header
    assert lib.dgvit_abi_version() == 7


def test_v2_entry_points_refuse_bad_arguments_without_a_gpu(amd):
    lib = amd.load_library()
    P = ctypes.c_void_p
    params = (ctypes.c_void_p * 6)(*([16] * 6))
    none = (ctypes.c_void_p * 6)()
    for C in (0, 17):
        assert lib.dgvit_cnn_forward_v2(P(16), params, P(16), P(16), 1 << 40, P(16), 1 << 40, 2, 64, 64, C, None) == -1
        assert b"frame channels" in lib.dgvit_last_error()
        assert lib.dgvit_cnn_backward_v3(P(16), params, none, P(16), P(16), P(16), 1 << 40, P(16), 1 << 40, 2, 64, 64, C, None) == -1
        assert b"frame channels" in lib.dgvit_last_error()
    for C in (1, 3, 4, 16):
        need = lib.dgvit_cnn_forward_scratch_floats_v2(2, 64, 64, C)
        assert lib.dgvit_cnn_forward_v2(P(16), params, P(16), P(16), 1 << 40, P(16), need - 1, 2, 64, 64, C, None) == -4
        need = lib.dgvit_cnn_backward_scratch_floats_v2(2, 64, 64, C)
        assert lib.dgvit_cnn_backward_v3(P(16), params, none, P(16), P(16), P(16), 1 << 40, P(16), need - 1, 2, 64, 64, C, None) == -4
        assert b"scratch too small" in lib.dgvit_last_error()


@pytest.mark.parametrize("hw, K, B", R.CASES, ids=str)
def test_the_parity_data_is_exact_in_fp32(hw, K, B):
    """the bound the reference module asserts holds at every layer of every case, fp32 pre-activations equal fp64 ones bit for bit (so
    the ReLU masks agree), and a fair share of the units is alive at every layer"""
    p = R.exact_params("qnet", K)
    stack = R.exact_stack(B, hw, K)
    assert set(stack.unique().tolist()) <= {0.0, 1.0, 2.0, 3.0} and stack.shape == (B, *hw, K) and stack.is_contiguous()
    bounds = []
    R.features({k: v.double() for k, v in p.items()}, stack.double(), bounds)
    assert len(bounds) == 3 and max(bounds) < R.EXACT / 8, bounds
    x32, x64 = stack.permute(0, 3, 1, 2), stack.double().permute(0, 3, 1, 2)
    for i in (1, 2, 3):
        w, b = p[f"conv{i}.weight"], p[f"conv{i}.bias"]
        assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0} and bool((b == b.round()).all()) and float(b.max()) <= 0
        z32 = torch.nn.functional.conv2d(x32, w, b, stride=2)
        z64 = torch.nn.functional.conv2d(x64, w.double(), b.double(), stride=2)
        assert torch.equal(z32.double(), z64), f"conv{i}: the fp32 pre-activations are not exact"
        alive = float((z64 > 0).double().mean())
        assert 0.1 <= alive <= 0.7, (i, alive)
        x32, x64 = torch.relu(z32), torch.relu(z64)
    assert R.param_spec("policy", K)[0][1] == (16, K, 5, 5)
