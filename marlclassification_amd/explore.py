"""Exploration controls of the action sampling: a temperature, an eps-soft mixture with the uniform distribution and
greedy (deterministic) acting - ``ModelsWrapper.set_exploration``, ``Trainer(temperature=, explore_eps=)`` and the
command line's ``--temperature`` / ``--explore-eps`` / ``--greedy``.

With z the policy's logits and nA actions the behaviour policy is

    s = softmax(z / temperature),    pi_b = (1 - eps) * s + eps / nA.

``pi_b`` is what the kernels sample from, what ``step_probs`` holds and what the log-probabilities are taken from, so an
entropy bonus, a PPO ratio and a replay see the distribution that acted.  ``greedy`` takes argmax pi_b (the lowest
index on a tie) instead of a draw.  This module holds the setting (``Exploration``), its validation, the command-line
spellings and ``behaviour_probs`` - the same map in plain torch, for users and documentation; the arithmetic of the
product runs in libmarl_hip.so (include/marl_hip_explore.h).
"""

from __future__ import annotations

import math
import re
from typing import NamedTuple, Tuple

import torch as th

MAX_EPS = 0.5  # the backward recovers softmax(z / tau) from the stored pi_b by dividing by 1 - eps

_NUM = r"[+-]?(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?"


class Exploration(NamedTuple):
    """``set_exploration``'s setting; the defaults are the plain policy softmax(z), sampled."""

    temperature: float = 1.0
    eps: float = 0.0
    greedy: bool = False

    @property
    def is_default(self) -> bool:
        return self.temperature == 1.0 and self.eps == 0.0 and not self.greedy

    def spelling(self) -> str:
        return f"temperature {self.temperature:g}, eps {self.eps:g}" + (", greedy" if self.greedy else "")


DEFAULT = Exploration()


def _number(v, what: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise ValueError(f"exploration: {what} must be a number, got {v!r}")
    return float(v)


def check(temperature=1.0, eps=0.0, greedy=False) -> Exploration:
    """The setting as an ``Exploration``; ValueError for a temperature that is not finite and > 0, an eps outside
    [0, ``MAX_EPS``] or a ``greedy`` that is not a bool."""
    t, e = _number(temperature, "the temperature"), _number(eps, "eps")
    if not math.isfinite(t) or not t > 0.0:
        raise ValueError(f"exploration: the temperature must be finite and > 0, got {temperature!r}")
    if not 0.0 <= e <= MAX_EPS:  # (NaN fails both comparisons)
        raise ValueError(f"exploration: eps must lie in [0, {MAX_EPS}], got {eps!r}")
    if not isinstance(greedy, (bool, int)) or greedy not in (0, 1):
        raise ValueError(f"exploration: greedy must be a bool, got {greedy!r}")
    return Exploration(t, e, bool(greedy))


def parse_schedule(text: str, what: str = "value") -> Tuple[float, float]:
    """The command-line spelling ``A[:B]`` of a per-epoch schedule: (start, end), end = start without ``:B``."""
    m = re.fullmatch(rf"({_NUM})(?::({_NUM}))?", text) if isinstance(text, str) else None
    if not m:
        raise ValueError(f'unknown {what} "{text}" (A or A:B, two numbers)')
    a = float(m.group(1))
    return a, a if m.group(2) is None else float(m.group(2))


def parse_temperature(text: str) -> Tuple[float, float]:
    """``--temperature T[:T_end]``: both ends checked."""
    a, b = parse_schedule(text, "temperature")
    check(temperature=a), check(temperature=b)
    return a, b


def parse_eps(text: str) -> Tuple[float, float]:
    """``--explore-eps E[:E_end]``: both ends checked."""
    a, b = parse_schedule(text, "exploration eps")
    check(eps=a), check(eps=b)
    return a, b


def schedule_value(ends: Tuple[float, float], epoch: int, nb_epoch: int) -> float:
    """Linear interpolation over the epochs: ``ends[0]`` at epoch 0, ``ends[1]`` at the last one."""
    a, b = ends
    if nb_epoch <= 1 or a == b:
        return a
    f = min(max(epoch, 0), nb_epoch - 1) / (nb_epoch - 1)
    return a + (b - a) * f


def behaviour_probs(probs: th.Tensor, temperature: float = 1.0, eps: float = 0.0) -> th.Tensor:
    """pi_b from the plain policy ``probs`` = softmax(z) ([..., nA], differentiable, any float dtype):
    softmax(log(probs) / temperature) mixed with the uniform distribution.  Probabilities of exactly 0 stay 0 before
    the mixture (log 0 = -inf)."""
    x = check(temperature, eps)
    s = probs if x.temperature == 1.0 else th.softmax(th.log(probs) / x.temperature, dim=-1)
    return s if x.eps == 0.0 else (1.0 - x.eps) * s + x.eps / probs.shape[-1]
