"""CPU (no GPU): dgvit_adam_step_groups (parameter groups and device-side learning-rate schedules in one launch) -- the
symbol, its binding and declaration, every argument check in front of the launch (the pointers are never dereferenced), and the Python
checks of LRSchedule / FlatAdam / FlatAdamW that come before anything touches a device."""
import ctypes
import inspect
import math
import os

import pytest
import torch

FAKE = ctypes.c_void_p(0x1000)     # non-null, 16-byte aligned, never read: only argument checks run
OFF4 = ctypes.c_void_p(0x1004)     # misaligned by 4 bytes
OFF2 = ctypes.c_void_p(0x1002)     # misaligned by 2 bytes
NAME = "dgvit_adam_step_groups"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import dgvit_amd
    return dgvit_amd.load_library()


def test_symbol_is_exported_bound_and_declared(lib):
    from dgvit_amd import _lib as L
    P, I, LL, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    want = [P, P, P, P, LL,          # p, g, m, v, n
            P, P, I,                 # seg_end4, seg_group, nseg
            P, I,                    # group_hyper, ngroups
            P,                       # lr_out
            F, F, F, I,              # beta1, beta2, eps, decoupled
            LL, LL, P,               # step, sched_step, step_dev
            I, LL, LL, F,            # sched_kind, warmup_steps, total_steps, final_ratio
            P, P]                    # grad_scale_dev, stream
    for path in (L.LIB_PATH, L.DIAG_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), NAME), f"{os.path.basename(path)} does not export {NAME}"
    res, got = L.SIGNATURES[NAME]
    assert res is I and list(got) == want
    for old in ("dgvit_adam_step", "dgvit_adam_step_scaled"):        # still there, still bound as they were
        assert hasattr(lib, old) and old in L.SIGNATURES
    with open(os.path.join(os.path.dirname(L.LIB_PATH), os.pardir, "include", "dgvit_hip.h")) as f:
        text = f.read()
    assert f"int {NAME}(float* p, const float* g, float* m, float* v, long long n," in text
    for arg in ("const long long* seg_end4", "const unsigned char* seg_group", "int nseg", "const float* group_hyper", "int ngroups",
                "float* lr_out", "int decoupled", "long long sched_step", "int sched_kind", "long long warmup_steps",
                "long long total_steps", "float final_ratio"):
        assert arg in text, arg


def test_abi_version_is_unchanged(lib):
    assert lib.dgvit_abi_version() == 7


def _call(lib, p=FAKE, g=FAKE, m=FAKE, v=FAKE, n=1024, seg_end4=FAKE, seg_group=FAKE, nseg=1, group_hyper=FAKE, ngroups=1, lr_out=None,
          beta1=0.9, beta2=0.999, eps=1e-8, decoupled=1, step=1, sched_step=1, step_dev=None, sched_kind=1, warmup_steps=2, total_steps=6,
          final_ratio=0.1, scale=None):
    return lib.dgvit_adam_step_groups(p, g, m, v, n, seg_end4, seg_group, nseg, group_hyper, ngroups, lr_out, beta1, beta2, eps, decoupled,
                                      step, sched_step, step_dev, sched_kind, warmup_steps, total_steps, final_ratio, scale, None)


CASES = [
    (dict(p=None), b"null"), (dict(g=None), b"null"), (dict(m=None), b"null"), (dict(v=None), b"null"),
    (dict(seg_end4=None), b"seg_end4"), (dict(seg_group=None), b"seg_group"), (dict(group_hyper=None), b"group_hyper"),
    (dict(n=0), b"n=0"), (dict(n=-4), b"n=-4"), (dict(n=6), b"n=6"),
    (dict(p=OFF4), b"aligned"), (dict(g=OFF4), b"aligned"), (dict(m=OFF4), b"aligned"), (dict(v=OFF4), b"aligned"),
    (dict(seg_end4=OFF4), b"seg_end4"), (dict(group_hyper=OFF2), b"group_hyper"), (dict(lr_out=OFF2), b"lr_out"),
    (dict(nseg=0), b"nseg=0"), (dict(nseg=2049), b"nseg=2049"), (dict(nseg=-1), b"nseg=-1"),
    (dict(ngroups=0), b"ngroups=0"), (dict(ngroups=257), b"ngroups=257"),
    (dict(beta1=1.0), b"beta1"), (dict(beta1=-0.1), b"beta1"), (dict(beta2=1.0), b"beta2"), (dict(beta2=-0.1), b"beta2"),
    (dict(step=0), b"step=0"), (dict(step=-3), b"step=-3"),
    (dict(sched_kind=3), b"sched_kind=3"), (dict(sched_kind=-1), b"sched_kind=-1"),
    (dict(warmup_steps=-1), b"warmup_steps=-1"),
    (dict(sched_kind=1, warmup_steps=7, total_steps=6), b"total_steps=6"),
    (dict(sched_kind=2, warmup_steps=7, total_steps=6), b"total_steps=6"),
    (dict(final_ratio=-0.1), b"final_ratio"), (dict(final_ratio=1.5), b"final_ratio"), (dict(final_ratio=math.nan), b"final_ratio"),
    (dict(final_ratio=math.inf), b"final_ratio"),
]


def _case_id(kw):
    names = {id(OFF4): "off4", id(OFF2): "off2"}
    return "-".join(f"{k}={names.get(id(x), x)}" for k, x in kw.items())


@pytest.mark.parametrize("kw, word", CASES, ids=[_case_id(kw) for kw, _ in CASES])
def test_bad_arguments_are_refused_before_any_launch(lib, kw, word):
    assert _call(lib, **kw) != 0
    msg = lib.dgvit_last_error()
    assert b"adam_step_groups" in msg and word in msg, msg


# ------------------------------------------------------------------------------------------------ LRSchedule
@pytest.mark.parametrize("kind", ["constant", "cosine", "linear"])
def test_schedule_factor(kind):
    from dgvit_amd.optim import LRSchedule
    W, T, r = 5, 25, 0.1
    s = LRSchedule(kind, warmup_steps=W, total_steps=T, final_ratio=r)
    assert s.factor(0) == 1 / W
    assert s.factor(W - 1) == 1
    assert s.factor(W) == 1
    after = [s.factor(k) for k in range(W, 3 * T)]
    assert all(a >= b for a, b in zip(after, after[1:])), "not monotone after the warm-up"
    assert all(a < b for a, b in zip([s.factor(k) for k in range(W)], [s.factor(k) for k in range(1, W)]))
    if kind == "constant":
        assert set(after) == {1.0}
        return
    assert s.factor(T) == r and s.factor(10 * T) == r
    mid = s.factor(W + (T - W) // 2)
    assert mid == (1 + r) / 2, mid        # half-way: cos(pi / 2) vanishes below the rounding of 1 + r; the linear kind is exact there


def test_schedule_without_warmup_and_defaults():
    from dgvit_amd.optim import LRSchedule
    assert [LRSchedule().factor(k) for k in (0, 1, 10 ** 9)] == [1.0, 1.0, 1.0]
    s = LRSchedule("linear", total_steps=4)
    assert [s.factor(k) for k in range(6)] == [1.0, 0.75, 0.5, 0.25, 0.0, 0.0]
    assert LRSchedule("cosine", warmup_steps=3, total_steps=3, final_ratio=0.5).factor(3) == 1.0     # an empty decay: q = 0 at its start
    p = inspect.signature(LRSchedule.__init__).parameters
    assert [(k, v.default) for k, v in p.items() if k != "self"] == [("kind", "constant"), ("warmup_steps", 0), ("total_steps", None),
                                                                      ("final_ratio", 0.0)]


@pytest.mark.parametrize("kw", [dict(kind="exp"), dict(kind="cosine"), dict(kind="linear"), dict(kind="cosine", warmup_steps=-1, total_steps=5),
                                dict(kind="cosine", warmup_steps=6, total_steps=5), dict(kind="cosine", warmup_steps=1.5, total_steps=5),
                                dict(kind="linear", total_steps=5, final_ratio=1.5), dict(kind="linear", total_steps=5, final_ratio=-0.1),
                                dict(kind="linear", total_steps=5, final_ratio=math.nan), dict(kind="linear", total_steps=True)],
                         ids=repr)
def test_schedule_refuses_bad_arguments(kw):
    from dgvit_amd.optim import LRSchedule
    with pytest.raises(ValueError, match="LRSchedule"):
        LRSchedule(**kw)


# ------------------------------------------------------------------------------------------------ signatures
def test_signatures():
    from dgvit_amd.optim import FlatAdam, FlatAdamW
    p = inspect.signature(FlatAdam.__init__).parameters
    assert [(k, v.default) for k, v in p.items() if k not in ("self", "params")] == [
        ("lr", 1e-3), ("betas", (0.9, 0.999)), ("eps", 1e-8), ("weight_decay", 0.0), ("capturable", False), ("max_grad_norm", None),
        ("schedule", None)]
    assert list(p)[:2] == ["self", "params"]
    w = inspect.signature(FlatAdamW.__init__).parameters
    assert list(w) == list(p)
    ref = inspect.signature(torch.optim.AdamW.__init__).parameters
    for k in ("lr", "betas", "eps", "weight_decay"):
        assert w[k].default == ref[k].default, k
    for k in ("capturable", "max_grad_norm", "schedule"):
        assert w[k].default == p[k].default
    assert issubclass(FlatAdamW, FlatAdam)
    for name in ("set_lr", "last_lr", "state_dict", "load_state_dict"):
        assert hasattr(FlatAdamW, name)


# ------------------------------------------------------------------------------------------------ group dicts, refused on the host
def _cpu_params():
    return torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(8, 2))


@pytest.mark.parametrize("cls_name", ["FlatAdam", "FlatAdamW"])
def test_group_dicts_are_checked_before_any_device_access(cls_name):
    """CPU parameters: had a check come late, the flat home would have refused them with a DgvitError first"""
    from dgvit_amd import optim
    cls = getattr(optim, cls_name)
    a, b = _cpu_params()
    with pytest.raises(ValueError, match="optimiser-wide"):
        cls([{"params": [a], "betas": (0.5, 0.9)}])
    with pytest.raises(ValueError, match="optimiser-wide"):
        cls([{"params": [a]}, {"params": [b], "eps": 1e-3}])
    with pytest.raises(ValueError, match="more than one parameter group"):
        cls([{"params": [a, b]}, {"params": [a]}])
    with pytest.raises(ValueError, match="more than one parameter group"):
        cls([{"params": torch.nn.Linear(2, 2)}, {"params": [a, a]}])
    lin = torch.nn.Linear(2, 2)
    with pytest.raises(ValueError, match="more than one parameter group"):
        cls([{"params": lin}, {"params": [lin.bias]}])
    with pytest.raises(ValueError, match="lr"):
        cls([{"params": [a], "lr": -1e-3}])
    with pytest.raises(ValueError, match="weight_decay"):
        cls([{"params": [a], "weight_decay": -0.1}])
    with pytest.raises(ValueError, match="lr"):
        cls([{"params": [a], "lr": math.nan}])
    with pytest.raises(ValueError, match="'params'"):
        cls([{"lr": 1e-3}])
    with pytest.raises(ValueError, match="lr"):
        cls([{"params": [a]}], lr=-1.0)                       # a group without its own lr inherits the bad one
    with pytest.raises(TypeError, match="mixture"):
        cls([{"params": [a]}, b])
    with pytest.raises(ValueError, match="schedule"):
        cls([a], schedule="cosine")


def test_flat_adamw_refuses_negative_hyper_parameters():
    from dgvit_amd.optim import FlatAdamW
    a, _ = _cpu_params()
    with pytest.raises(ValueError, match="lr"):
        FlatAdamW([a], lr=-1e-3)
    with pytest.raises(ValueError, match="weight_decay"):
        FlatAdamW([a], weight_decay=-1e-2)


def test_no_decay_groups_on_the_host():
    """the recipe: matrices decay; biases, norm gains, the position embedding and the class token do not"""
    import dgvit_amd
    from dgvit_amd.optim import no_decay_groups
    m = dgvit_amd.GoTPolicy(2, 2, 1, 2, 64, image_size=(84, 84), patch_size=(12, 12))
    groups = no_decay_groups(m, 0.05)
    assert [sorted(g) for g in groups] == [["params", "weight_decay"]] * 2
    assert [g["weight_decay"] for g in groups] == [0.05, 0.0]
    names = {id(p): k for k, p in m.named_parameters()}
    decay, rest = ([names[id(p)] for p in g["params"]] for g in groups)
    assert sorted(decay + rest) == sorted(k for k, p in m.named_parameters() if p.requires_grad)
    assert all(m.get_parameter(k).ndim >= 2 for k in decay)
    assert "trans.pos_embedding" in rest and "trans.cls_token" in rest
    assert all(m.get_parameter(k).ndim < 2 or k.endswith(("pos_embedding", "cls_token")) for k in rest)
    assert "trans.to_patch_embedding.1.weight" in decay and "trans.to_patch_embedding.1.bias" in rest and "trans.layer_norm.g" in rest
    both = no_decay_groups(m, 0.05, lr=3e-4, skip=lambda name, p: name.endswith("fc1.weight"))
    assert [g["lr"] for g in both] == [3e-4, 3e-4]
    assert any(p is m.fc1.weight for p in both[1]["params"]) and any(p is m.trans.pos_embedding for p in both[0]["params"])
    with pytest.raises(ValueError, match="weight_decay"):
        no_decay_groups(m, -1.0)
