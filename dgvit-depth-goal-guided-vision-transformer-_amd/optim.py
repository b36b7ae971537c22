"""Flat-buffer optimiser step and Polyak target update for the DGViT networks.

The reference calls ``torch.optim.Adam`` over ~70 tensors per network (DRL.py:126-168, 401-403, 412-414) and a
per-parameter Python loop ``soft_update`` (utils.py:31-33).  Here the parameters of a network are re-homed ONCE into
one flat fp32 buffer (its *home*: each ``nn.Parameter`` keeps its identity, its ``.data`` becomes a view), and both
updates are one HBM-bound HIP kernel per contiguous run of that buffer (``dgvit_adam_step`` / ``dgvit_soft_update``).

Gradient-norm clipping (``clip_grad_norm_(…, 10)`` of the reference's behaviour-cloning loop, attention_imitating.py:45-67) rides on
the same buffers: ``FlatAdam(max_grad_norm=…)`` folds it into the step (one streaming read for the norm, the coefficient stays on the
device, Adam applies it while it reads the gradient), and ``clip_grad_norm_`` here is torch's function over the flat runs.

``FlatAdamW``, parameter groups (``[{"params": …, "lr": …, "weight_decay": …}]``, ``no_decay_groups``) and ``LRSchedule`` (warm-up, cosine
or linear decay) go through ``dgvit_adam_step_groups``: still one kernel per run -- it looks up each element's group in a segment table
staged into LDS -- with the learning rates in device memory and the schedule evaluated in the kernel, so a captured step follows both
(DESIGN 3.37).

There is one owner of parameter storage per module: ``flatten_parameters(module)`` creates (or returns) the module's
home and ``FlatAdam`` adopts it, so an optimiser and a Polyak update on the same network share the same buffer.
Layout of a home: for every ``GoT`` encoder inside the module its trainable parameters in the C ABI's table order --
exactly the layout of the flat gradient buffer the fused encoder backward produces, which Adam then consumes in place --
followed by all remaining parameters in ``parameters()`` order.  Two networks of the same architecture get the same
layout, which is what the one-kernel ``soft_update`` needs.
"""
import ctypes
import math
import weakref
from typing import Iterable, List, Union

import torch
from torch.utils.weak import WeakIdKeyDictionary

from . import _lib
from . import functional as F_
from .goalformer import GoT


def _al4(n: int) -> int:
    return (n + 3) & ~3


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_HOME_OF = WeakIdKeyDictionary()   # parameter -> (home, index in home.params); keyed by identity (tensor == is elementwise)


def _no_home():
    return None


class _Home:
    """Parameters living back to back (4-float aligned slots) in one flat buffer, with room for Adam's moments."""

    def __init__(self, params: List[torch.Tensor], sections: List[int] = None):
        # sections[i]: which GoT encoder's table parameter i belongs to (-1: none); Adam runs never straddle two sections, so
        # the encoder run can pick up the fused backward's gradient buffer without a copy
        self.sections = list(sections) if sections is not None else [-1] * len(params)
        if not params:
            raise ValueError("no parameters to flatten")
        if not all(p.is_cuda for p in params):
            raise _lib.DgvitError("flat parameter buffers need the module on a ROCm device first (call .to(device) before)")
        self.params = params
        self.offsets, off = [], 0
        for p in params:
            self.offsets.append(off)
            off += _al4(p.numel())
        self.numel = off
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=params[0].device)   # zeros: padding lanes stay finite
        # Optimiser state follows a parameter into its new home: a parameter that has taken Adam steps in another (still intact)
        # home -- a loose FlatAdam(net.parameters()) home later adopted by the module's, a child module's home swallowed by its
        # parent's, a layout that changed -- keeps its moments and its step count (torch keeps them in `state[p]`, wherever p lives).
        carried, intact_cache = [], {}
        for i, p in enumerate(params):
            ent = _HOME_OF.get(p)
            if ent is None or ent[0] is self:
                continue
            old, j = ent
            if id(old) not in intact_cache:
                intact_cache[id(old)] = old.intact()
            if old.exp_avg is not None and old.steps[j] > 0:
                if not intact_cache[id(old)]:
                    raise _lib.DgvitError("parameter storage was replaced (e.g. by .to()) after optimiser state was built; rebuild the optimiser")
                carried.append((i, old, j))
        self.exp_avg = self.exp_avg_sq = self.gflat = None
        self.steps = [0] * len(params)          # per-parameter Adam step counts (torch keeps `state[p]["step"]`)
        self.owner = [None] * len(params)       # weak reference to the FlatAdam whose state lives in this home's slot (None: nobody's yet)
        for i, p in enumerate(params):
            ent = _HOME_OF.get(p)
            if ent is not None and ent[0] is not self:
                self.owner[i] = ent[0].owner[ent[1]]
        if carried:
            m, v = self.moments()
            for i, old, j in carried:
                n, o, oo = params[i].numel(), self.offsets[i], old.offsets[j]
                m[o:o + n].copy_(old.exp_avg[oo:oo + n])
                v[o:o + n].copy_(old.exp_avg_sq[oo:oo + n])
                self.steps[i] = old.steps[j]
        for i, (p, o) in enumerate(zip(params, self.offsets)):
            v = self.flat[o:o + p.numel()].view_as(p)
            v.copy_(p.data)
            p.data = v
            _HOME_OF[p] = (self, i)
        self.zero_copy_elems = self.copied_elems = 0   # gradient elements Adam consumed in place / had to gather (tests, tuning)
        self.signature = tuple((tuple(p.shape), o) for p, o in zip(params, self.offsets))

    def __deepcopy__(self, memo):
        return None     # a copied module's parameters are fresh tensors: its home is rebuilt on first use

    def __reduce__(self):
        return (_no_home, ())   # torch.save(module): parameters are pickled as ordinary tensors, the home is rebuilt on use

    def intact(self) -> bool:
        base = self.flat.data_ptr()
        return all(p.data.data_ptr() == base + 4 * o for p, o in zip(self.params, self.offsets))

    def moments(self):
        if self.exp_avg is None:
            self.exp_avg = torch.zeros_like(self.flat)
            self.exp_avg_sq = torch.zeros_like(self.flat)
        return self.exp_avg, self.exp_avg_sq

    def grad_view(self, idx: List[int]):
        """The gradients of the parameters ``idx`` (adjacent slots) as one flat tensor when they already are views of one buffer laid
        out like their slots (the fused encoder backward's), else None."""
        lo = self.offsets[idx[0]]
        hi = self.offsets[idx[-1]] + _al4(self.params[idx[-1]].numel())
        g0 = self.params[idx[0]].grad
        st, o0 = g0.untyped_storage().data_ptr(), g0.storage_offset()
        if o0 % 4 == 0 and g0.data_ptr() % 16 == 0 and (o0 + hi - lo) * 4 <= g0.untyped_storage().nbytes() and all(
                self.params[i].grad.untyped_storage().data_ptr() == st and self.params[i].grad.is_contiguous()
                and self.params[i].grad.storage_offset() - o0 == self.offsets[i] - lo for i in idx):
            return torch.empty(0, dtype=g0.dtype, device=g0.device).set_(g0.untyped_storage(), o0, (hi - lo,))
        return None

    def grad_run(self, idx: List[int], count: bool = True) -> torch.Tensor:
        """Gradients of the parameters ``idx`` (adjacent slots) as one flat tensor laid out like their slots: zero copy when
        they already are views of one buffer with that layout (``grad_view``), else one multi-tensor copy.  ``count``: an optimiser
        step's call, added to ``zero_copy_elems`` / ``copied_elems``."""
        lo = self.offsets[idx[0]]
        hi = self.offsets[idx[-1]] + _al4(self.params[idx[-1]].numel())
        view = self.grad_view(idx)
        if view is not None:
            if count:
                self.zero_copy_elems += hi - lo
            return view
        if count:
            self.copied_elems += hi - lo
        if self.gflat is None:
            self.gflat = torch.zeros_like(self.flat)
        views = [self.gflat[self.offsets[i]:self.offsets[i] + self.params[i].numel()].view_as(self.params[i]) for i in idx]
        torch._foreach_copy_(views, [self.params[i].grad for i in idx])
        return self.gflat[lo:hi]


class _Moments:
    """Adam state (moments, step counts) of ONE optimiser over a home's slots, kept beside the home: used when another live
    optimiser already keeps its state in the home itself.  torch.optim.Adam holds its state per optimiser, and the reference
    builds two of them over the same policy (Imitation_learning.py:379 and :812): the second must not see, or wipe, the first's."""

    def __init__(self, home: _Home):
        self.home = weakref.ref(home)
        self.exp_avg = self.exp_avg_sq = None
        self.steps = [0] * len(home.params)

    def moments(self):
        if self.exp_avg is None:
            flat = self.home().flat
            self.exp_avg, self.exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
        return self.exp_avg, self.exp_avg_sq


def _layout(module: torch.nn.Module):
    order, sections, taken, nsec = [], [], set(), 0
    for sub in module.modules():
        if isinstance(sub, GoT):
            for p in sub.param_table():     # frozen parameters keep their slot: a frozen target has its source's layout
                if id(p) not in taken:
                    order.append(p)
                    sections.append(nsec)
                    taken.add(id(p))
            nsec += 1
    for p in module.parameters():
        if id(p) not in taken:
            order.append(p)
            sections.append(-1)
            taken.add(id(p))
    return order, sections


def flatten_parameters(module: torch.nn.Module) -> torch.Tensor:
    """Re-home ALL parameters of ``module`` into one flat buffer (see the module docstring for the layout) and return it;
    a module that already has an intact home keeps it.  Call after ``.to(device)``; ``FlatAdam`` and ``soft_update`` do it
    themselves when needed."""
    return home_of(module).flat


def home_of(module: torch.nn.Module) -> _Home:
    h = getattr(module, "_dgvit_home", None)
    lay, sections = _layout(module)
    if isinstance(h, _Home) and len(h.params) == len(lay) and all(a is b for a, b in zip(h.params, lay)) and h.intact():
        return h
    h = _Home(lay, sections)        # (carries over the Adam state of parameters that lived in another intact home; raises if that
                                    #  home's storage was replaced, e.g. by .to(), after optimiser state was built)
    module._dgvit_home = h
    return h


def _check_max_norm(value, what: str) -> float:
    """a positive finite number (bool is not one), or ValueError"""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (value > 0) or not math.isfinite(value):
        raise ValueError(f"{what} must be a positive finite number, got {value!r}")
    return float(value)


def _adjacent_runs(params, steps_of=None, who="FlatAdam"):
    """[(home, [param indices])]: maximal runs of adjacent slots (of one section of one home) among those ``params`` that have a
    gradient; with ``steps_of(home)`` (per-slot step counts) a run also ends where the count changes."""
    by_home = {}
    for p in params:
        if p.grad is None:
            continue
        ent = _HOME_OF.get(p)
        if ent is None or not ent[0].intact():
            raise _lib.DgvitError(f"{who}: parameter storage was replaced (e.g. by .to() or deepcopy); rebuild the optimiser")
        by_home.setdefault(id(ent[0]), (ent[0], []))[1].append(ent[1])
    runs = []
    for home, idx in by_home.values():
        idx.sort()
        cur = [idx[0]]
        steps = steps_of(home) if steps_of is not None else None
        for a, b in zip(idx, idx[1:]):
            if b == a + 1 and (steps is None or steps[b] == steps[a]) and home.sections[b] == home.sections[a]:
                cur.append(b)
            else:
                runs.append((home, cur))
                cur = [b]
        runs.append((home, cur))
    return runs


class _ClipScratch:
    """Device scratch of one gradient-norm clip: DGVIT_GRAD_NORM_PARTIALS doubles and, behind them, the two floats of
    dgvit_grad_clip_coef (total norm, coefficient).  Never zeroed: the first norm launch of a clip writes every partial."""

    def __init__(self, device):
        self.device = device
        self.buf = torch.empty(_lib.GRAD_NORM_PARTIALS + 1, dtype=torch.float64, device=device)
        out = self.buf[_lib.GRAD_NORM_PARTIALS:].view(torch.float32)
        self.norm, self.coef = out[0], out[1]            # 0-d views

    def measure(self, lib, flats, max_norm: float) -> None:
        """norm of the concatenation of the flat buffers ``flats`` and its coefficient for ``max_norm``: len(flats) + 1 launches"""
        with torch.cuda.device(self.device):
            for k, g in enumerate(flats):
                if g.device != self.device:
                    raise _lib.DgvitError("gradient-norm clipping needs all gradients on one device")
                rc = lib.dgvit_grad_sqnorm_partials(ctypes.c_void_p(g.data_ptr()), g.numel(), ctypes.c_void_p(self.buf.data_ptr()),
                                                    int(k > 0), _stream())
                _lib.check(rc, "dgvit_grad_sqnorm_partials")
            rc = lib.dgvit_grad_clip_coef(ctypes.c_void_p(self.buf.data_ptr()), max_norm, ctypes.c_void_p(self.norm.data_ptr()), _stream())
            _lib.check(rc, "dgvit_grad_clip_coef")


def _check_non_negative(value, what: str) -> float:
    """a finite number >= 0 (bool is not one), or ValueError"""
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not (value >= 0) or not math.isfinite(value):
        raise ValueError(f"{what} must be a finite number >= 0, got {value!r}")
    return float(value)


class LRSchedule:
    """Learning-rate factor of a ``FlatAdam`` / ``FlatAdamW`` step as a function of the number ``s`` of optimiser steps already taken:
    linear warm-up ``(s + 1) / warmup_steps`` for ``s < warmup_steps``, then with ``q = min((s - warmup_steps) / max(1, total_steps -
    warmup_steps), 1)`` the factor is 1 (``"constant"``), ``r + (1 - r) (1 + cos(pi q)) / 2`` (``"cosine"``) or ``r + (1 - r)(1 - q)``
    (``"linear"``) with ``r = final_ratio``; past ``total_steps`` it stays ``r``.  ``torch.optim.lr_scheduler.LambdaLR(opt,
    schedule.factor)`` stepped after every optimiser step is the same schedule.  The optimiser's kernel evaluates this formula on the
    device (in double, from its step counter), so a captured step follows it; ``factor`` is the same formula on the host.
    ``total_steps`` is needed by the decaying kinds only."""
    KINDS = {"constant": 0, "cosine": 1, "linear": 2}

    def __init__(self, kind: str = "constant", warmup_steps: int = 0, total_steps=None, final_ratio: float = 0.0):
        if kind not in self.KINDS:
            raise ValueError(f"LRSchedule: kind must be one of {sorted(self.KINDS)}, got {kind!r}")
        if isinstance(warmup_steps, bool) or not isinstance(warmup_steps, int) or warmup_steps < 0:
            raise ValueError(f"LRSchedule: warmup_steps must be an integer >= 0, got {warmup_steps!r}")
        if total_steps is None:
            if kind != "constant":
                raise ValueError(f"LRSchedule: the {kind} schedule needs total_steps")
        elif isinstance(total_steps, bool) or not isinstance(total_steps, int) or total_steps < warmup_steps:
            raise ValueError(f"LRSchedule: total_steps must be an integer >= warmup_steps={warmup_steps}, got {total_steps!r}")
        if isinstance(final_ratio, bool) or not isinstance(final_ratio, (int, float)) or not (0.0 <= final_ratio <= 1.0):
            raise ValueError(f"LRSchedule: final_ratio must be in [0, 1], got {final_ratio!r}")
        self.kind, self.warmup_steps, self.total_steps, self.final_ratio = kind, warmup_steps, total_steps, float(final_ratio)

    def factor(self, s: int) -> float:
        """the factor of the step taken after ``s`` earlier ones (``s = 0`` is the first step)"""
        w, r = self.warmup_steps, self.final_ratio
        if s < w:
            return (s + 1) / w
        if self.kind == "constant":
            return 1.0
        q = min((s - w) / max(1, self.total_steps - w), 1.0)
        if self.kind == "cosine":
            return r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * q))
        return r + (1.0 - r) * (1.0 - q)

    def state_dict(self):
        return {"kind": self.kind, "warmup_steps": self.warmup_steps, "total_steps": self.total_steps, "final_ratio": self.final_ratio}

    def _c_args(self):
        total = self.total_steps if self.total_steps is not None else self.warmup_steps
        return self.KINDS[self.kind], self.warmup_steps, total, self.final_ratio

    def __repr__(self):
        return (f"LRSchedule({self.kind!r}, warmup_steps={self.warmup_steps}, total_steps={self.total_steps}, "
                f"final_ratio={self.final_ratio})")


_CONSTANT = LRSchedule()
MAX_SEGMENTS, MAX_GROUPS = 2048, 256     # include/dgvit_hip.h: dgvit_adam_step_groups
_GROUP_KEYS = ("params", "lr", "weight_decay")


def _group_items(params):
    """the entries of one ``params`` argument (a module, a tensor, or an iterable of modules and tensors) as a list"""
    return [params] if isinstance(params, (torch.nn.Module, torch.Tensor)) else list(params)


def _parse_groups(params, lr: float, weight_decay: float, who: str):
    """``params`` as FlatAdam takes it -> (list of (items, lr, weight_decay), whether group dicts were given).  Host work only: unknown
    keys, bad values and a parameter in two groups are refused before anything touches a device."""
    items = _group_items(params)
    if not any(isinstance(g, dict) for g in items):
        return [(items, lr, weight_decay)], False
    if not all(isinstance(g, dict) for g in items):
        raise TypeError(f"{who}: params must be modules / parameters, or a list of group dicts, not a mixture")
    if len(items) > MAX_GROUPS:
        raise ValueError(f"{who}: at most {MAX_GROUPS} parameter groups, got {len(items)}")
    out, seen = [], set()
    for k, g in enumerate(items):
        other = sorted(set(g) - set(_GROUP_KEYS))
        if other:
            raise ValueError(f"{who}: group {k} has the key(s) {other}; a group sets 'params', 'lr' and 'weight_decay' only -- betas, eps "
                             "and everything else are optimiser-wide here")
        if "params" not in g:
            raise ValueError(f"{who}: group {k} has no 'params'")
        g_lr = _check_non_negative(g.get("lr", lr), f"{who}: group {k}: lr")
        g_wd = _check_non_negative(g.get("weight_decay", weight_decay), f"{who}: group {k}: weight_decay")
        members = _group_items(g["params"])
        for it in members:
            for p in (it.parameters() if isinstance(it, torch.nn.Module) else [it]):
                if id(p) in seen:
                    raise ValueError(f"{who}: some parameters appear in more than one parameter group")
                seen.add(id(p))
        out.append((members, g_lr, g_wd))
    return out, True


def _default_skip(name: str, p) -> bool:
    last = name.rsplit(".", 1)[-1]
    return last in ("pos_embedding", "cls_token", "goal_token")


def no_decay_groups(module: torch.nn.Module, weight_decay: float, lr=None, skip=None):
    """The usual AdamW recipe as two group dicts for ``FlatAdamW`` / ``FlatAdam``: the trainable parameters of ``module`` with
    ``ndim >= 2`` (the GEMM weights) get ``weight_decay``; every other one -- biases, LayerNorm / RMSNorm gains -- and whatever
    ``skip(name, p)`` selects gets none.  ``skip`` defaults to the position embedding and the goal (class) token by name.  ``lr`` (None:
    the optimiser's) is set on both groups.  A module on the device whose parameters have no flat home yet is flattened here
    (``flatten_parameters``), so that the groups are segments of the MODULE's home -- the layout the fused encoder backward writes its gradients in -- whatever order the
    groups list the parameters in."""
    weight_decay = _check_non_negative(weight_decay, "no_decay_groups: weight_decay")
    if lr is not None:
        lr = _check_non_negative(lr, "no_decay_groups: lr")
    skip = _default_skip if skip is None else skip
    decay, rest = [], []
    for name, p in module.named_parameters():
        if p.requires_grad:
            (decay if p.ndim >= 2 and not skip(name, p) else rest).append(p)
    if decay + rest and all(p.is_cuda for p in decay + rest) and any(
            _HOME_OF.get(p) is None or not _HOME_OF[p][0].intact() for p in decay + rest):
        home_of(module)       # (parameters that already live in an intact home, e.g. a parent module's, stay there)
    groups = [{"params": decay, "weight_decay": weight_decay}, {"params": rest, "weight_decay": 0.0}]
    if lr is not None:
        for g in groups:
            g["lr"] = lr
    return [g for g in groups if g["params"]]


class _SegmentTable:
    """Device tables of one run for dgvit_adam_step_groups: the ends of its segments (float4 units from the run's start) and their
    groups, adjacent slots of one group merged.  Built once per distinct run and kept: a captured graph holds the pointers."""

    def __init__(self, home: _Home, idx, group_of_slot):
        self.home = weakref.ref(home)
        lo = home.offsets[idx[0]]
        ends, groups = [], []
        for i in idx:
            end4 = (home.offsets[i] + _al4(home.params[i].numel()) - lo) // 4
            if groups and groups[-1] == group_of_slot[i]:
                ends[-1] = end4
            else:
                ends.append(end4)
                groups.append(group_of_slot[i])
        if len(ends) > MAX_SEGMENTS:
            raise _lib.DgvitError(f"FlatAdam: a run of {len(ends)} segments (changes of parameter group along the flat buffer); "
                                  f"dgvit_adam_step_groups takes at most {MAX_SEGMENTS}")
        self.nseg = len(ends)
        dev = home.flat.device
        self.end4 = torch.tensor(ends, dtype=torch.int64).to(dev)
        self.group = torch.tensor(groups, dtype=torch.uint8).to(dev)


class FlatAdam:
    """``torch.optim.Adam`` semantics (amsgrad=False) with one HIP kernel per contiguous run of a flat parameter buffer.

    ``params``: modules (all their parameters) and / or an iterable of parameters, like the reference's optimisers over
    sub-sets of a network (DRL.py:107-111, 145-148).  As with torch's optimisers a parameter whose ``.grad`` is None at
    ``step()`` is skipped (no moment update, its own step count does not advance), and a parameter that first receives a
    gradient later starts its bias correction at 1 then.  Build it after ``module.to(device)``.  ``capturable=True`` keeps
    the step counter in device memory (like torch's ``capturable`` optimisers) so that ``step()`` can be recorded into a HIP
    graph; every replay must then see the same set of parameters with gradients.

    ``max_grad_norm`` (None: off; else a positive number): ``step()`` clips the global 2-norm of the gradients to it first, like
    ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` followed by the step (attention_imitating.py:66-67).  The norm covers
    exactly this optimiser's parameters that have a gradient at this step.  It is one streaming read per run of the flat buffers
    (double accumulation, fixed summation order); the coefficient ``min(max_grad_norm / (norm + 1e-6), 1)`` stays in device memory
    and Adam multiplies each gradient element by it as it reads it (weight decay is added to the clipped gradient, as in
    clip-then-step).  Nothing synchronises, so the step stays graph-capturable, with ``capturable`` True or False.  Unlike
    clip-then-step the ``.grad`` tensors are NOT modified: the clipped gradient is never written.  ``last_grad_norm`` is the norm
    before clipping as a 0-d device tensor (a view of the optimiser's scratch, overwritten by the next step; None before the first
    clipped step).  ``max_grad_norm`` is a plain attribute read on every ``step()``; it is passed as a kernel argument, so a
    captured graph keeps the value it was captured with.  It is not part of ``state_dict()`` (it is not optimiser state in torch
    either).

    Parameter groups and schedules.  ``params`` may also be a list of group dicts ``{"params": …, "lr": …,
    "weight_decay": …}`` (``params`` of a group: a module, or parameters and leaf tensors; missing keys take the constructor's values;
    betas and eps are optimiser-wide, any other key is refused; a parameter in two groups is refused), and ``schedule`` an
    ``LRSchedule``.  With either, the step goes through ``dgvit_adam_step_groups``: still ONE launch per run of the flat buffer -- runs
    are formed exactly as without groups; the kernel looks up each element's group in a segment table it stages into LDS -- with the
    learning rates in a device table and the schedule factor computed in the kernel, so a step captured by ``GraphedStep`` follows
    the schedule and ``set_lr``.  A schedule counts OPTIMISER steps (``step_count``; with ``capturable=True`` the device counter), not
    the steps of a single parameter: a parameter that first gets a gradient at step 100 takes the learning rate of step 100.
    ``param_groups`` lists the groups (``params``, ``lr``, ``weight_decay``) for inspection; change a learning rate with ``set_lr`` (an
    eager step also picks up a value written into ``param_groups``; a replayed graph sees only ``set_lr``).  ``last_lr``: the
    learning rates ``lr * factor`` the last step used, a ``(groups,)`` device tensor written by the kernel (None before the first
    step).  ``last_step_launches``: how many C entry points the last ``step()`` called.  Without groups and schedule nothing
    changes: ``dgvit_adam_step`` / ``dgvit_adam_step_scaled`` with ``lr`` by value, as before.
    """

    _decoupled = False      # FlatAdamW: weight decay multiplies the parameter (torch.optim.AdamW) instead of joining the gradient

    def __init__(self, params: Union[torch.nn.Module, Iterable], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 capturable: bool = False, max_grad_norm=None, schedule=None):
        who = type(self).__name__
        if max_grad_norm is not None:
            _check_max_norm(max_grad_norm, "FlatAdam: max_grad_norm")
        if schedule is not None and not isinstance(schedule, LRSchedule):
            raise ValueError(f"{who}: schedule must be an LRSchedule or None, got {type(schedule).__name__}")
        self.max_grad_norm, self._clip, self.last_grad_norm = max_grad_norm, None, None
        self.capturable, self._step_dev = bool(capturable), None
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        parsed, grouped = _parse_groups(params, self.lr, self.weight_decay, who)     # host checks only: nothing touched a device yet
        if self._decoupled or grouped or schedule is not None:
            _check_non_negative(lr, f"{who}: lr")
            _check_non_negative(weight_decay, f"{who}: weight_decay")
        self.schedule = schedule
        # the new entry point (dgvit_adam_step_groups) serves groups, schedules and decoupled decay; everything else runs as it always did
        self._grouped = bool(self._decoupled or grouped or schedule is not None)
        self._hyper = self._hyper_host = self._last_lr = self._last_lr_buf = None   # device (G, 2) table of (lr, weight_decay), its host mirror, (G,) lr * f
        self._tables = {}                                          # (id(home), slots of a run) -> _SegmentTable
        self.last_step_launches = 0
        items = [it for members, _, _ in parsed for it in members]
        self.modules = [m for m in items if isinstance(m, torch.nn.Module)]
        for p in items:
            if not isinstance(p, torch.nn.Module) and not (isinstance(p, torch.Tensor) and p.is_leaf and p.dtype == torch.float32):
                # nn.Parameter or a plain leaf such as DRL.py's log_alpha
                raise TypeError(f"FlatAdam: expected modules, parameters or fp32 leaf tensors, got {type(p).__name__}")
        for m in self.modules:
            home_of(m)
        chosen, seen, loose = [], set(), []
        self.param_groups = []
        for members, g_lr, g_wd in parsed:
            mine = []
            for it in members:
                if isinstance(it, torch.nn.Module):
                    for p in it.parameters():
                        if p.requires_grad and id(p) not in seen:
                            seen.add(id(p))
                            mine.append(p)
            for p in members:
                if isinstance(p, torch.nn.Module):
                    continue
                if p.requires_grad and id(p) not in seen:
                    seen.add(id(p))
                    mine.append(p)
                    ent = _HOME_OF.get(p)
                    if ent is None or not ent[0].intact():
                        loose.append(p)
            chosen.extend(mine)
            self.param_groups.append({"params": mine, "lr": g_lr, "weight_decay": g_wd})
        if loose:
            _Home(loose)               # parameters handed over one by one that no module home owns yet
        self._group_of = {id(p): k for k, g in enumerate(self.param_groups) for p in g["params"]}
        self.params = chosen
        self.step_count = 0
        # Like a new torch.optim.Adam, a new FlatAdam starts from empty state.  Moments and step counts normally live with the
        # parameters' home (they follow the parameters when a home is rebuilt), owned by ONE optimiser per slot.  A slot whose owner
        # is still alive keeps serving that optimiser -- this one then keeps its own state beside the home (`_Moments`), exactly as
        # two torch.optim.Adam instances over the same parameters would; a slot whose owner is gone is taken over and whatever it
        # left there is cleared.  load_state_dict() restores a saved state.
        self._private = {}                 # id(home) -> _Moments
        for p in chosen:
            home, i = _HOME_OF[p]
            other = home.owner[i]() if home.owner[i] is not None else None
            if other is not None and other is not self and id(home) not in self._private:
                self._private[id(home)] = _Moments(home)
        for p in chosen:
            home, i = _HOME_OF[p]
            if id(home) in self._private:
                continue
            home.owner[i] = weakref.ref(self)
            if home.steps[i]:
                home.steps[i] = 0
                if home.exp_avg is not None:
                    o, n = home.offsets[i], p.numel()
                    home.exp_avg[o:o + n].zero_()
                    home.exp_avg_sq[o:o + n].zero_()

    def _all_params(self):
        return self.params

    def _state(self, home: _Home):
        """where this optimiser's moments / step counts for `home`'s slots live: the home itself, or its own `_Moments`"""
        if not self._private:
            return home
        st = self._private.get(id(home))
        if st is not None and st.home() is home:
            return st
        if any(m.home() is None or not m.home().intact() for m in self._private.values()):
            raise _lib.DgvitError("FlatAdam: parameter storage was re-homed after this (second) optimiser over the same parameters was "
                                  "built; rebuild the optimiser")
        return home

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.params:
            if set_to_none:
                p.grad = None
            elif p.grad is not None:
                p.grad.zero_()

    def _runs(self):
        """[(home, [param indices])]: maximal runs of adjacent slots whose parameters have a gradient and equal step counts."""
        return _adjacent_runs(self.params, lambda home: self._state(home).steps)

    @torch.no_grad()
    def step(self) -> None:
        max_norm = self.max_grad_norm
        if max_norm is not None:
            max_norm = _check_max_norm(max_norm, "FlatAdam: max_grad_norm")
        lib = _lib.load()
        runs = self._runs()
        if not runs:
            return
        self.step_count += 1
        self.last_step_launches = 0
        step_ptr = ctypes.c_void_p(0)
        if self.capturable:
            if len({self._state(home).steps[idx[0]] for home, idx in runs}) != 1:
                raise _lib.DgvitError("FlatAdam(capturable=True): every parameter must receive a gradient on every step")
            if self._step_dev is None:
                self._step_dev = torch.full((1,), self._state(runs[0][0]).steps[runs[0][1][0]], dtype=torch.int64, device=runs[0][0].flat.device)
            self._step_dev += 1                      # a device op: replayed with the graph
            step_ptr = ctypes.c_void_p(self._step_dev.data_ptr())
        grads = None
        if max_norm is not None:
            # every run's gradient resolved once, for the norm and for Adam; 2 * runs + 1 launches in all
            grads = [home.grad_run(idx) for home, idx in runs]
            if self._clip is None or self._clip.device != grads[0].device:
                self._clip = _ClipScratch(grads[0].device)
                self.last_grad_norm = self._clip.norm
            self._clip.measure(lib, grads, max_norm)
            self.last_step_launches += len(grads) + 1
        if self._grouped:
            self._sync_hyper(runs[0][0].flat.device)
        for k, (home, idx) in enumerate(runs):
            lo = home.offsets[idx[0]]
            n = home.offsets[idx[-1]] + _al4(home.params[idx[-1]].numel()) - lo
            g = grads[k] if grads is not None else home.grad_run(idx)
            st = self._state(home)
            m, v = st.moments()
            t = st.steps[idx[0]] + 1
            for i in idx:
                st.steps[i] = t
            self.last_step_launches += 1
            if self._grouped:
                self._step_groups(lib, home, idx, lo, n, g, m, v, t, step_ptr, grads is not None)
                continue
            with torch.cuda.device(home.flat.device):
                if grads is None:
                    rc = lib.dgvit_adam_step(ctypes.c_void_p(home.flat.data_ptr() + 4 * lo), ctypes.c_void_p(g.data_ptr()),
                                             ctypes.c_void_p(m.data_ptr() + 4 * lo), ctypes.c_void_p(v.data_ptr() + 4 * lo), n,
                                             self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, t, step_ptr, _stream())
                else:
                    rc = lib.dgvit_adam_step_scaled(ctypes.c_void_p(home.flat.data_ptr() + 4 * lo), ctypes.c_void_p(g.data_ptr()),
                                                    ctypes.c_void_p(m.data_ptr() + 4 * lo), ctypes.c_void_p(v.data_ptr() + 4 * lo), n,
                                                    self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, t, step_ptr,
                                                    ctypes.c_void_p(self._clip.coef.data_ptr()), _stream())
            _lib.check(rc, "dgvit_adam_step" if grads is None else "dgvit_adam_step_scaled")
        # the kernel wrote the parameters through raw pointers: no autograd version counter moved
        F_.notify_parameters_changed(self.params)

    def _sync_hyper(self, device=None) -> None:
        """Bring the device table of (lr, weight_decay) per group in line with ``param_groups``: allocated on first use (and then kept:
        a captured graph holds its address), written entry by entry with stream-ordered fills -- no synchronisation, no copy from
        pageable host memory.  Without a device and before the first step there is nothing to write yet."""
        want = [(float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups]
        if self._hyper is None:
            if device is None:
                return
            self._hyper = torch.empty((len(want), 2), dtype=torch.float32, device=device)
            self._last_lr_buf = torch.zeros(len(want), dtype=torch.float32, device=device)
            self._hyper_host = [(None, None)] * len(want)
        for k, (have, new) in enumerate(zip(self._hyper_host, want)):
            for j in (0, 1):
                if have[j] != new[j]:
                    self._hyper[k, j].fill_(new[j])
        self._hyper_host = want

    def _step_groups(self, lib, home, idx, lo, n, g, m, v, t, step_ptr, scaled) -> None:
        """one run through dgvit_adam_step_groups"""
        if home.flat.device != self._hyper.device:
            raise _lib.DgvitError("FlatAdam with parameter groups or a schedule needs all its parameters on one device")
        key = (id(home), tuple(idx))
        tab = self._tables.get(key)
        if tab is None or tab.home() is not home:
            tab = self._tables[key] = _SegmentTable(home, idx, {i: self._group_of[id(home.params[i])] for i in idx})
        kind, warmup, total, final_ratio = (self.schedule or _CONSTANT)._c_args()
        with torch.cuda.device(home.flat.device):
            rc = lib.dgvit_adam_step_groups(
                ctypes.c_void_p(home.flat.data_ptr() + 4 * lo), ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(m.data_ptr() + 4 * lo),
                ctypes.c_void_p(v.data_ptr() + 4 * lo), n, ctypes.c_void_p(tab.end4.data_ptr()), ctypes.c_void_p(tab.group.data_ptr()),
                tab.nseg, ctypes.c_void_p(self._hyper.data_ptr()), len(self.param_groups), ctypes.c_void_p(self._last_lr_buf.data_ptr()),
                self.betas[0], self.betas[1], self.eps, int(self._decoupled), t, self.step_count, step_ptr, kind, warmup, total,
                final_ratio, ctypes.c_void_p(self._clip.coef.data_ptr()) if scaled else ctypes.c_void_p(0), _stream())
        _lib.check(rc, "dgvit_adam_step_groups")
        self._last_lr = self._last_lr_buf

    @property
    def last_lr(self):
        return self._last_lr

    def set_lr(self, value, group=None) -> None:
        """Set the learning rate of group ``group`` (None: of every group, and the optimiser-wide default): the host mirror
        ``param_groups[i]["lr"]`` and, stream-ordered, the device table the kernel reads -- the next eager step and the next replay
        of a captured step use it.  (Without groups and schedule the step passes ``lr`` by value: a captured one keeps the old.)"""
        who = type(self).__name__
        value = _check_non_negative(value, f"{who}.set_lr: lr")
        if group is None:
            which = range(len(self.param_groups))
            self.lr = value
        else:
            if isinstance(group, bool) or not isinstance(group, int) or not 0 <= group < len(self.param_groups):
                raise ValueError(f"{who}.set_lr: group must be an index below {len(self.param_groups)}, got {group!r}")
            which = [group]
            if len(self.param_groups) == 1:
                self.lr = value
        for k in which:
            self.param_groups[k]["lr"] = value
        self._sync_hyper()

    def _homes(self):
        out, seen = [], set()
        for p in self.params:
            ent = _HOME_OF.get(p)
            if ent is not None and id(ent[0]) not in seen:
                seen.add(id(ent[0]))
                out.append(ent[0])
        return out

    def state_dict(self):
        """Per parameter (in the optimiser's parameter order): step count and both moments, like torch.optim.Adam's state."""
        state = []
        if self.capturable and self._step_dev is not None:
            # graph replays advance only the device counter: bring the host mirror up to date (one device -> host read)
            dev_step = int(self._step_dev.item())
            for p in self.params:
                home, i = _HOME_OF[p]
                st = self._state(home)
                if st.steps[i] > 0:
                    st.steps[i] = dev_step
            self.step_count = max(self.step_count, dev_step)
        for p in self.params:
            home, i = _HOME_OF[p]
            st = self._state(home)
            o, n = home.offsets[i], p.numel()
            if st.exp_avg is None or st.steps[i] == 0:
                state.append(None)
            else:
                state.append({"step": st.steps[i], "exp_avg": st.exp_avg[o:o + n].view_as(p).clone(),
                              "exp_avg_sq": st.exp_avg_sq[o:o + n].view_as(p).clone()})
        return {"step": self.step_count, "lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                "state": state, "decoupled": bool(self._decoupled),
                "schedule": self.schedule.state_dict() if self.schedule is not None else None,
                "groups": [{"lr": g["lr"], "weight_decay": g["weight_decay"]} for g in self.param_groups]}

    def load_state_dict(self, sd) -> None:
        if len(sd["state"]) != len(self.params):
            raise ValueError("optimizer state does not match this optimiser's parameters")
        if "groups" in sd and len(sd["groups"]) != len(self.param_groups):
            raise ValueError(f"optimizer state has {len(sd['groups'])} parameter groups, this optimiser has {len(self.param_groups)}")
        if bool(sd.get("decoupled", self._decoupled)) != bool(self._decoupled):
            raise ValueError("optimizer state was saved with the other kind of weight decay (FlatAdam: L2, FlatAdamW: decoupled)")
        self.step_count = int(sd["step"])
        if "groups" in sd:               # (a dict saved before there were groups leaves groups and schedule as constructed)
            for mine, saved in zip(self.param_groups, sd["groups"]):
                mine["lr"] = _check_non_negative(saved["lr"], "load_state_dict: lr")
                mine["weight_decay"] = _check_non_negative(saved["weight_decay"], "load_state_dict: weight_decay")
            if len(self.param_groups) == 1:
                self.lr, self.weight_decay = self.param_groups[0]["lr"], self.param_groups[0]["weight_decay"]
            self._sync_hyper()
        if sd.get("schedule") is not None:
            self.schedule = LRSchedule(**sd["schedule"])
            self._grouped = True
        for p, st in zip(self.params, sd["state"]):
            home, i = _HOME_OF[p]
            mine = self._state(home)
            o, n = home.offsets[i], p.numel()
            m, v = mine.moments()
            if st is None:
                mine.steps[i] = 0
                m[o:o + n].zero_()
                v[o:o + n].zero_()
            else:
                mine.steps[i] = int(st["step"])
                m[o:o + n].view_as(p).copy_(st["exp_avg"])
                v[o:o + n].view_as(p).copy_(st["exp_avg_sq"])
        if self._step_dev is not None:
            self._step_dev.fill_(max((self._state(_HOME_OF[p][0]).steps[_HOME_OF[p][1]] for p in self.params), default=0))


class FlatAdamW(FlatAdam):
    """``torch.optim.AdamW`` semantics and defaults (decoupled weight decay: ``p *= 1 - lr_t * weight_decay`` before the Adam update, the
    moments from the raw gradient) on the flat buffers.  Everything else is ``FlatAdam``: parameter groups, ``schedule``, ``set_lr``,
    ``capturable``, ``max_grad_norm``; the step always goes through ``dgvit_adam_step_groups``, one launch per run."""
    _decoupled = True

    def __init__(self, params: Union[torch.nn.Module, Iterable], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 capturable: bool = False, max_grad_norm=None, schedule=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable,
                         max_grad_norm=max_grad_norm, schedule=schedule)


def _flat_pair(target, source):
    tb, sb = home_of(target), home_of(source)
    if tb.signature != sb.signature:
        raise _lib.DgvitError("soft_update: target and source networks do not have the same parameter layout")
    return tb, sb


@torch.no_grad()
def soft_update(target: torch.nn.Module, source: torch.nn.Module, tau: float) -> None:
    """target <- target*(1-tau) + source*tau (utils.py:31-33) as ONE HIP kernel over the two networks' flat buffers (both are
    flattened on first use; an optimiser built on either keeps working because it adopts the same home)."""
    tb, sb = _flat_pair(target, source)
    lib = _lib.load()
    with torch.cuda.device(tb.flat.device):
        rc = lib.dgvit_soft_update(ctypes.c_void_p(tb.flat.data_ptr()), ctypes.c_void_p(sb.flat.data_ptr()), tb.numel, float(tau),
                                   _stream())
    _lib.check(rc, "dgvit_soft_update")
    F_.notify_parameters_changed(target)


@torch.no_grad()
def hard_update(target: torch.nn.Module, source: torch.nn.Module) -> None:
    """target <- source (utils.py:35-37): one device copy of the flat buffer."""
    tb, sb = _flat_pair(target, source)
    tb.flat.copy_(sb.flat)
    F_.notify_parameters_changed(target)


_CLIP_SCRATCH = {}    # device -> _ClipScratch of the stand-alone clip_grad_norm_
_FLT_MAX = 3.4028234663852886e38


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite: bool = False, foreach=None) -> torch.Tensor:
    """``torch.nn.utils.clip_grad_norm_`` (attention_imitating.py:66) on the flat buffers: scales the ``.grad`` of ``parameters`` (a
    module, a tensor or an iterable of tensors; a repeated entry counts once) in place by ``min(max_norm / (norm + 1e-6), 1)`` and
    returns their total 2-norm as a 0-d device tensor.  Nothing synchronises unless ``error_if_nonfinite`` asks for the read-back.

    Gradients that are adjacent views of one flat buffer (the fused encoder backward's) form one run: one norm launch and one
    in-place scale launch over the whole run (its padding lanes are zero).  The remaining gradients (heads, log_alpha) are gathered
    by their home for the norm, as Adam gathers them, and scaled with one ``torch._foreach_mul_`` by the device coefficient.
    Parameters that have no flat home yet get one (as ``FlatAdam`` gives them).  Only ``norm_type=2`` exists here; gradients must be
    on the device -- there is no CPU path.  ``foreach`` is accepted and ignored.  ``max_norm=inf`` measures without scaling.
    ``FlatAdam(max_grad_norm=…)`` does the same without the write pass."""
    if float(norm_type) != 2.0:
        raise ValueError(f"dgvit_amd.optim.clip_grad_norm_ supports norm_type=2 only (got {norm_type!r}); use "
                         "torch.nn.utils.clip_grad_norm_ for other norms")
    max_norm = float(max_norm)
    if not (max_norm > 0):
        raise ValueError(f"clip_grad_norm_: max_norm must be greater than 0, got {max_norm!r}")
    if isinstance(parameters, torch.nn.Module):
        modules, items = [parameters], list(parameters.parameters())
    else:
        modules, items = [], [parameters] if isinstance(parameters, torch.Tensor) else list(parameters)
    params, seen = [], set()
    for p in items:
        if not isinstance(p, torch.Tensor):
            raise TypeError(f"clip_grad_norm_: expected a module, a tensor or an iterable of tensors, got {type(p).__name__}")
        if p.grad is not None and id(p) not in seen:
            seen.add(id(p))
            params.append(p)
    if not params:
        return torch.tensor(0.0)
    if not all(p.grad.is_cuda and p.is_cuda for p in params):
        raise _lib.DgvitError("clip_grad_norm_: gradients must be on a ROCm device; there is no CPU path")
    if not all(p.grad.dtype == torch.float32 and p.dtype == torch.float32 and p.is_leaf for p in params):
        raise _lib.DgvitError("clip_grad_norm_: fp32 leaf tensors with fp32 gradients only")
    lib = _lib.load()
    for m in modules:
        home_of(m)
    loose = [p for p in params if _HOME_OF.get(p) is None or not _HOME_OF[p][0].intact()]
    if loose:
        _Home(loose)
    flats, in_place, gathered = [], [], []
    for home, idx in _adjacent_runs(params, who="clip_grad_norm_"):
        view = home.grad_view(idx)
        if view is not None:
            in_place.append(view)
            flats.append(view)
        else:
            flats.append(home.grad_run(idx, count=False))
            gathered.extend(home.params[i].grad for i in idx)
    dev = flats[0].device
    scratch = _CLIP_SCRATCH.get(dev)
    if scratch is None:
        scratch = _CLIP_SCRATCH[dev] = _ClipScratch(dev)
    scratch.measure(lib, flats, min(max_norm, _FLT_MAX))
    total = scratch.norm.clone()        # the scratch is overwritten by the next call
    if error_if_nonfinite and not bool(torch.isfinite(total)):
        raise RuntimeError(f"The total norm of order {float(norm_type)} for gradients from `parameters` is non-finite, so it cannot be "
                           "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                           "`error_if_nonfinite=False`")
    with torch.cuda.device(dev):
        for g in in_place:
            rc = lib.dgvit_scale_by_device_scalar(ctypes.c_void_p(g.data_ptr()), g.numel(), ctypes.c_void_p(scratch.coef.data_ptr()), _stream())
            _lib.check(rc, "dgvit_scale_by_device_scalar")
        if gathered:
            torch._foreach_mul_(gathered, scratch.coef)
    return total
