"""Options of the flat optimiser step (``marl_optim_step``, include/marl_hip_optim.h): AdamW with decoupled weight
decay, per-module learning-rate multipliers, a learning-rate schedule and an averaged copy of the weights.

Run-time choices: nothing here reaches ``marl.json`` or a state-dict key.  ``reference_step`` is the definition in
plain torch (any dtype; the tests run it in float64); the kernel is held to it.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, List, Mapping, Optional, Sequence, Tuple, Union

import torch as th

MAX_SEGMENTS = 128  # MARL_OPTIM_MAX_SEGMENTS
KINDS = ("constant", "linear", "cosine")  # MARL_SCHED_*
GROUP_NAMES = ("map_obs", "map_pos", "encode_msg", "decode_msg", "belief_unit", "action_unit", "policy", "critic",
               "predict")
ALIASES = {"cnn": "map_obs"}
_PREFIX = "_ModelsWrapper__"


class Segment(C.Structure):
    """Mirror of ``marl_optim_segment``."""

    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("lr_mult", C.c_float), ("weight_decay", C.c_float)]


class ScheduleDesc(C.Structure):
    """Mirror of ``marl_optim_schedule``."""

    _fields_ = [("kind", C.c_int32), ("pad_", C.c_int32), ("base_lr", C.c_double), ("warmup_steps", C.c_int64),
                ("total_steps", C.c_int64), ("final_ratio", C.c_double)]


@dataclass(frozen=True)
class Schedule:
    """lr_t = ``lr_at(schedule, t)``.  ``base_lr`` None: the trainer's learning rate (``with_base``)."""

    kind: str = "constant"
    base_lr: Optional[float] = None
    warmup_steps: int = 0
    total_steps: int = 0
    final_ratio: float = 0.0

    def __post_init__(self) -> None:
        if self.kind not in KINDS:
            raise ValueError(f"schedule kind must be one of {KINDS}, got {self.kind!r}")
        if self.base_lr is not None and not (self.base_lr >= 0.0 and math.isfinite(self.base_lr)):
            raise ValueError(f"base_lr must be finite and >= 0, got {self.base_lr}")
        for k in ("warmup_steps", "total_steps"):
            v = getattr(self, k)
            if isinstance(v, bool) or not isinstance(v, int) or v < 0:
                raise ValueError(f"{k} must be an integer >= 0, got {v!r}")
        if self.kind != "constant" and self.total_steps < self.warmup_steps:
            raise ValueError(f"total_steps ({self.total_steps}) < warmup_steps ({self.warmup_steps})")
        if not 0.0 <= self.final_ratio <= 1.0:
            raise ValueError(f"final_ratio must lie in [0, 1], got {self.final_ratio}")

    def with_base(self, lr: float) -> "Schedule":
        if self.base_lr is not None:
            return self
        return Schedule(self.kind, float(lr), self.warmup_steps, self.total_steps, self.final_ratio)

    def desc(self) -> ScheduleDesc:
        if self.base_lr is None:
            raise ValueError("the schedule has no base_lr (with_base)")
        return ScheduleDesc(KINDS.index(self.kind), 0, self.base_lr, self.warmup_steps, self.total_steps,
                            self.final_ratio)


def lr_at(schedule: Schedule, step: int) -> float:
    """Learning rate of the 1-based ``step`` in Python float64: linear warm-up from base_lr / warmup_steps at step 1
    to base_lr at step warmup_steps, then constant, or a linear / cosine decay that reaches final_ratio * base_lr at
    total_steps and stays there."""
    if step < 1:
        raise ValueError(f"step must be >= 1, got {step}")
    base = schedule.base_lr
    if base is None:
        raise ValueError("the schedule has no base_lr (with_base)")
    w, total, fr = schedule.warmup_steps, schedule.total_steps, schedule.final_ratio
    if step <= w:
        return base * (float(step) / float(w))  # (exactly base at step == warmup_steps)
    if schedule.kind == "constant":
        return base
    span = float(total - w)
    x = min(1.0, (float(step) - float(w)) / span) if span > 0.0 else 1.0
    if schedule.kind == "linear":
        return base * (1.0 - (1.0 - fr) * x)
    return base * (fr + (1.0 - fr) * 0.5 * (1.0 + math.cos(math.pi * x)))


def _canonical(name: str) -> str:
    name = ALIASES.get(name, name)
    if name not in GROUP_NAMES:
        raise ValueError(f"unknown parameter group {name!r}: valid names are {', '.join(GROUP_NAMES)} "
                         f"(aliases: {', '.join(f'{a} = {b}' for a, b in ALIASES.items())})")
    return name


GroupValue = Union[float, Tuple[float, float]]


@dataclass(frozen=True)
class OptimOptions:
    """``weight_decay``: decoupled (AdamW).  ``decay``: ``"matrices"`` - tensors with ndim >= 2 decay, biases and
    LayerNorm / GroupNorm gains do not - or ``"all"``.  ``groups``: module name -> lr_mult, or (lr_mult,
    weight_decay); the names are the module names inside the state-dict keys (``GROUP_NAMES``; ``cnn`` = ``map_obs``);
    lr_mult 0 freezes the module.  ``schedule``: a ``Schedule`` (its ``base_lr`` None: the trainer's learning rate).
    ``ema_decay``: None, or the decay of the averaged weights in (0, 1)."""

    weight_decay: float = 0.0
    decay: str = "matrices"
    groups: Mapping[str, GroupValue] = field(default_factory=dict)
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    schedule: Schedule = Schedule()
    ema_decay: Optional[float] = None

    def __post_init__(self) -> None:
        if not (self.weight_decay >= 0.0 and math.isfinite(self.weight_decay)):
            raise ValueError(f"weight_decay must be finite and >= 0, got {self.weight_decay}")
        if self.decay not in ("matrices", "all"):
            raise ValueError(f"decay must be 'matrices' or 'all', got {self.decay!r}")
        betas = tuple(float(b) for b in self.betas)
        if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"betas must be two numbers in [0, 1), got {self.betas!r}")
        object.__setattr__(self, "betas", betas)
        if not (self.eps > 0.0 and math.isfinite(self.eps)):
            raise ValueError(f"eps must be finite and > 0, got {self.eps}")
        if self.ema_decay is not None and not 0.0 < self.ema_decay < 1.0:
            raise ValueError(f"ema_decay must lie in (0, 1) or be None, got {self.ema_decay}")
        if not isinstance(self.schedule, Schedule):
            raise ValueError(f"schedule must be an optim.Schedule, got {self.schedule!r}")
        norm: Dict[str, Tuple[float, Optional[float]]] = {}
        for name, val in dict(self.groups).items():
            key = _canonical(name)
            if key in norm:
                raise ValueError(f"parameter group {key!r} is given twice")
            mult, wd = (val if isinstance(val, (tuple, list)) else (val, None))
            mult = float(mult)
            wd = None if wd is None else float(wd)
            if not (mult >= 0.0 and math.isfinite(mult)):
                raise ValueError(f"lr_mult of group {name!r} must be finite and >= 0, got {mult}")
            if wd is not None and not (wd >= 0.0 and math.isfinite(wd)):
                raise ValueError(f"weight_decay of group {name!r} must be finite and >= 0, got {wd}")
            norm[key] = (mult, wd)
        object.__setattr__(self, "groups", tuple(sorted(norm.items())))  # (hashable: graph keys)

    def group_of(self, key: str) -> Tuple[float, Optional[float]]:
        return dict(self.groups).get(group_name(key), (1.0, None))

    def tensor_options(self, key: str, shape: Sequence[int]) -> Tuple[float, float]:
        """(lr_mult, weight_decay) of the parameter tensor ``key``."""
        mult, wd = self.group_of(key)
        if wd is None:
            wd = self.weight_decay
        if self.decay == "matrices" and len(shape) < 2:
            wd = 0.0
        return mult, wd

    def with_lr(self, lr: float) -> "OptimOptions":
        """These options with the schedule's ``base_lr`` filled in from the trainer's learning rate."""
        sched = self.schedule.with_base(lr)
        if sched is self.schedule:
            return self
        return OptimOptions(self.weight_decay, self.decay, {k: (m, w) for k, (m, w) in self.groups}, self.betas,
                            self.eps, sched, self.ema_decay)

    def fingerprint(self) -> str:
        """One string that identifies the update rule (resume refuses another)."""
        s = self.schedule
        g = ",".join(f"{k}={m!r}:{w!r}" for k, (m, w) in self.groups)
        return (f"adamw;wd={self.weight_decay!r};decay={self.decay};groups=[{g}];betas={self.betas!r};eps={self.eps!r};"
                f"sched={s.kind}:{s.base_lr!r}:{s.warmup_steps}:{s.total_steps}:{s.final_ratio!r};"
                f"ema={self.ema_decay!r}")


def group_name(key: str) -> str:
    """The module name inside a state-dict key (``_ModelsWrapper__policy.0.weight`` -> ``policy``)."""
    head = key.split(".", 1)[0]
    return head[len(_PREFIX):] if head.startswith(_PREFIX) else head


def segments(flat, opts: OptimOptions) -> List[Tuple[int, int, float, float]]:
    """The merged segment table [(begin, end, lr_mult, weight_decay)] over ``flat`` (``FlatParams``: ``names``,
    ``offsets``, ``shapes``, ``numel``): ascending, covering [0, numel) without gaps; adjacent tensors with equal
    (lr_mult, weight_decay) are one segment (the padding between 16-byte aligned slices belongs to the tensor in front
    of it: its gradient is zero)."""
    names = list(flat.names)
    out: List[List] = []
    for i, k in enumerate(names):
        begin = flat.offsets[k]
        end = flat.offsets[names[i + 1]] if i + 1 < len(names) else flat.numel
        if begin % 4 != 0:
            raise ValueError(f"{k}: slice starts at element {begin}, not 16-byte aligned")
        mult, wd = opts.tensor_options(k, flat.shapes[k])
        if out and out[-1][2] == mult and out[-1][3] == wd and out[-1][1] == begin:
            out[-1][1] = end
        else:
            out.append([begin, end, mult, wd])
    if len(out) > MAX_SEGMENTS:
        raise ValueError(f"{len(out)} segments after merging: the kernel takes at most {MAX_SEGMENTS}")
    return [tuple(s) for s in out]


def segment_array(table: Sequence[Tuple[int, int, float, float]]):
    return (Segment * max(len(table), 1))(*[Segment(int(b), int(e), float(m), float(w)) for b, e, m, w in table])


def frozen_ranges(table: Sequence[Tuple[int, int, float, float]]) -> List[Tuple[int, int]]:
    return [(b, e) for b, e, m, _ in table if m == 0.0]


def reference_step(p: th.Tensor, g: th.Tensor, m: th.Tensor, v: th.Tensor, ema: Optional[th.Tensor],
                   table: Sequence[Tuple[int, int, float, float]], opts: OptimOptions, step: int,
                   grad_scale: float = 1.0) -> None:
    """The definition, in place on flat tensors of any dtype (``torch.optim.AdamW``'s single-tensor order):
    per element of segment s
        g' = g * grad_scale;  p *= 1 - lr_t * mult_s * wd_s;  m += (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g'^2
        p -= (lr_t * mult_s / bc1) * m / (sqrt(v) / sqrt(bc2) + eps);  ema = d * ema + (1 - d) * p
    with lr_t = ``lr_at(opts.schedule, step)``; a segment with mult_s == 0 is left alone."""
    lr_t = lr_at(opts.schedule, step)
    b1, b2 = opts.betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    with th.no_grad():
        for begin, end, mult, wd in table:
            if mult == 0.0:
                continue
            ps, ms, vs = p[begin:end], m[begin:end], v[begin:end]
            gs = g[begin:end] * grad_scale
            if lr_t * mult * wd != 0.0:
                ps.mul_(1.0 - lr_t * mult * wd)
            ms.add_((gs - ms) * (1.0 - b1))
            vs.mul_(b2).add_(gs * gs * (1.0 - b2))
            denom = vs.sqrt() / math.sqrt(bc2) + opts.eps
            ps.sub_((lr_t * mult / bc1) * (ms / denom))
            if ema is not None:
                d = opts.ema_decay
                ema[begin:end].mul_(d).add_(ps * (1.0 - d))


def parse_groups(spec: str) -> Dict[str, GroupValue]:
    """``"cnn=0.1,policy=0,critic=1:0.01"`` -> {"cnn": 0.1, "policy": 0.0, "critic": (1.0, 0.01)}."""
    out: Dict[str, GroupValue] = {}
    for item in (s.strip() for s in spec.split(",")):
        if not item:
            continue
        name, eq, val = item.partition("=")
        name = name.strip()
        if not eq or not name or not val.strip():
            raise ValueError(f"parameter group {item!r}: expected NAME=LR_MULT or NAME=LR_MULT:WEIGHT_DECAY")
        _canonical(name)
        if name in out:
            raise ValueError(f"parameter group {name!r} is given twice")
        mult, colon, wd = val.partition(":")
        try:
            out[name] = (float(mult), float(wd)) if colon else float(mult)
        except ValueError:
            raise ValueError(f"parameter group {item!r}: LR_MULT and WEIGHT_DECAY must be numbers") from None
    return out


def parse_schedule(spec: str, warmup_steps: int = 0, total_steps: int = 0,
                   base_lr: Optional[float] = None) -> Schedule:
    """``"cosine:0.1"`` -> a cosine schedule whose final ratio is 0.1 (``constant | linear | cosine[:final_ratio]``)."""
    kind, colon, fr = spec.strip().partition(":")
    if kind not in KINDS:
        raise ValueError(f"lr schedule {spec!r}: expected constant, linear or cosine, optionally :FINAL_RATIO")
    try:
        ratio = float(fr) if colon else 0.0
    except ValueError:
        raise ValueError(f"lr schedule {spec!r}: FINAL_RATIO must be a number") from None
    return Schedule(kind, base_lr, warmup_steps, total_steps, ratio)


def parse_betas(spec: str) -> Tuple[float, float]:
    parts = spec.split(",")
    try:
        b1, b2 = (float(s) for s in parts)
    except ValueError:
        raise ValueError(f"adam betas {spec!r}: expected B1,B2") from None
    return b1, b2
