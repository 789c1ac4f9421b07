"""Options of the supervised term of the loss: class weights, label smoothing and step weights of the vote error, and
cost-sensitive rewards - ``Trainer(class_weights=, label_smoothing=, error_step_weights=, weight_rewards=)``,
``HipEngine.set_class_loss`` (under which ``a2c_loss`` / ``advantages`` / ``ppo_loss`` run) and the command line's
``--class-weights`` / ``--label-smoothing`` / ``--error-steps`` / ``--weight-rewards``.

With z[t,b,:] = mean_a step_preds[t,a,b,:], nll_c = -(z_c - max z - log sum exp(z - max z)), y = y[b], class weights w,
smoothing eps and step weights s:

    q_c      = (1 - eps) * w_y * 1[c == y] + (eps / nC) * w_c
    err[t,b] = s_t * sum_c q_c * nll_c

which without s_t is ``F.cross_entropy(z, y, weight=w, label_smoothing=eps, reduction="none")``.  The reference's loss
(training/trainer.py:78-87) is w == 1, eps == 0, s == 1.  With ``weight_rewards`` the rewards become
w_y * (log nC - CE) / log nC; smoothing and step weights never reach them.

This module holds the setting (``ClassLoss``), its validation, the command-line spellings and the definition in plain
differentiable torch (``vote_error``, ``rewards``) - for tests and for users of the per-step autograd API; the
arithmetic of the product runs in libmarl_hip.so (include/marl_hip_classloss.h).
"""

from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import torch as th

_NUM = r"[+-]?(?:\d+\.?\d*|\.\d+)(?:[eE][+-]?\d+)?"


def check_vector(values, what: str, length: int) -> Tuple[float, ...]:
    """``values`` (sequence, array or tensor) as a tuple of the fp32 values the kernels will read; checked: ``length``
    finite entries >= 0 that are not all zero."""
    try:
        t = th.as_tensor(values).detach().to("cpu", th.float64)
    except (TypeError, ValueError, RuntimeError) as err:
        raise ValueError(f"class loss: {what} must be numbers: {err}")
    if t.dim() != 1 or t.numel() != length:
        raise ValueError(f"class loss: {what} must be a vector of length {length}, got shape {tuple(t.shape)}")
    if not bool(th.isfinite(t).all()):
        raise ValueError(f"class loss: {what} must be finite")
    if bool((t < 0).any()):
        raise ValueError(f"class loss: {what} must be >= 0")
    t = t.to(th.float32)
    if not bool((t > 0).any()):
        raise ValueError(f"class loss: {what} must not all be zero")
    return tuple(float(v) for v in t.tolist())


@dataclass(frozen=True)
class ClassLoss:
    """The setting of one loss call, validated: hashable (the device copies of the two vectors and a captured graph
    are keyed by it) and immutable.  The vectors are kept as the fp32 values the kernels read; None = all ones."""

    nb_class: int
    nb_steps: int
    class_weights: Optional[Tuple[float, ...]] = None
    label_smoothing: float = 0.0
    step_weights: Optional[Tuple[float, ...]] = None
    weight_rewards: bool = False

    def __post_init__(self) -> None:
        for name in ("nb_class", "nb_steps"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"class loss: {name} must be an integer >= 1, got {v!r}")
        if self.class_weights is not None:
            object.__setattr__(self, "class_weights", check_vector(self.class_weights, "class weights", self.nb_class))
        if self.step_weights is not None:
            object.__setattr__(self, "step_weights", check_vector(self.step_weights, "step weights", self.nb_steps))
        object.__setattr__(self, "label_smoothing", check_label_smoothing(self.label_smoothing))
        if not isinstance(self.weight_rewards, (bool, int)) or self.weight_rewards not in (0, 1):
            raise ValueError(f"class loss: weight_rewards must be a bool, got {self.weight_rewards!r}")
        object.__setattr__(self, "weight_rewards", bool(self.weight_rewards))

    @property
    def is_default(self) -> bool:
        """Nothing given: the reference's loss through the plain kernels (neutral VALUES given explicitly are not the
        default - they run the option instances, which then reproduce the plain bits)."""
        return (self.class_weights is None and self.step_weights is None and self.label_smoothing == 0.0 and
                not self.weight_rewards)


def check_label_smoothing(eps) -> float:
    """eps as a float; ValueError unless it is a number in [0, 1) (NaN fails the comparison)."""
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= float(eps) < 1.0:
        raise ValueError(f"class loss: label_smoothing must lie in [0, 1), got {eps!r}")
    return float(eps)


def _vote(step_preds: th.Tensor, y: th.Tensor) -> Tuple[th.Tensor, th.Tensor]:
    if step_preds.dim() != 4:
        raise ValueError(f"step_preds must be [Ns, Na, Nb, nC], got {tuple(step_preds.shape)}")
    if y.dim() != 1 or y.shape[0] != step_preds.shape[2]:
        raise ValueError(f"y must be [Nb = {step_preds.shape[2]}], got {tuple(y.shape)}")
    return step_preds.mean(dim=1), y.to(step_preds.device, th.int64)


def _vector(v, n: int, like: th.Tensor, what: str) -> th.Tensor:
    t = th.as_tensor(v, dtype=like.dtype, device=like.device)
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"{what} must be a vector of length {n}, got shape {tuple(t.shape)}")
    return t


def _targets(targets: th.Tensor, nb: int, nc: int, like: th.Tensor) -> th.Tensor:
    q = targets.to(like.device, like.dtype)
    if tuple(q.shape) != (nb, nc):
        raise ValueError(f"targets must be [Nb = {nb}, nC = {nc}], got {tuple(q.shape)}")
    return q


def vote_error(step_preds: th.Tensor, y: th.Tensor, class_weights=None, label_smoothing: float = 0.0,
               step_weights=None, targets: Optional[th.Tensor] = None) -> th.Tensor:
    """err [Ns, Nb] of the module docstring from ``step_preds`` [Ns, Na, Nb, nC] and ``y`` [Nb], differentiable, in the
    dtype of ``step_preds``.  nll comes from the logits (log_softmax), never log(softmax).
    ``targets`` (include/marl_hip_softtargets.h): a target distribution Q [Nb, nC] in place of ``y`` -
    q_c = w_c ((1 - eps) Q[b,c] + eps / nC), err[t,b] = s_t sum_c q_c nll_c, which without s_t is
    ``F.cross_entropy(z, Q, weight=w, label_smoothing=eps, reduction="none")``; entries with Q[b,c] == 0 are skipped,
    not multiplied."""
    z, y = _vote(step_preds, y)
    ns, nb, nc = z.shape
    eps = check_label_smoothing(label_smoothing)
    nll = -th.log_softmax(z, dim=-1)  # [Ns, Nb, nC]
    w = z.new_ones(nc) if class_weights is None else _vector(class_weights, nc, z, "class_weights")
    if targets is not None:
        q = _targets(targets, nb, nc, z)
        err = (1.0 - eps) * th.where(q != 0, q * w * nll, th.zeros_like(nll)).sum(dim=-1)
        if eps != 0.0:
            err = err + (eps / nc) * (nll * w).sum(dim=-1)
        if step_weights is not None:
            err = err * _vector(step_weights, ns, z, "step_weights").view(ns, 1)
        return err
    wy = w[y]  # [Nb]
    err = (1.0 - eps) * wy * nll.gather(-1, y.view(1, nb, 1).expand(ns, nb, 1)).squeeze(-1)
    if eps != 0.0:
        err = err + (eps / nc) * (nll * w).sum(dim=-1)
    if step_weights is not None:
        err = err * _vector(step_weights, ns, z, "step_weights").view(ns, 1)
    return err


def rewards(step_preds: th.Tensor, y: th.Tensor, class_weights=None,
            targets: Optional[th.Tensor] = None) -> th.Tensor:
    """rew [Ns, Na, Nb] = w_y * (log nC - CE(step_preds[t, a, b, :], y[b])) / log nC (functions.py:7-32 with
    ``class_weights`` None).  ``targets``: Q [Nb, nC] in place of ``y`` -
    rew = sum_c w_c Q[b,c] (log nC - nll_c) / log nC, linear in Q; entries with Q[b,c] == 0 are skipped."""
    _, y = _vote(step_preds, y)
    ns, na, nb, nc = step_preds.shape
    if targets is not None:
        q = _targets(targets, nb, nc, step_preds)
        rnd = math.log(nc)
        per_class = (rnd - -th.log_softmax(step_preds, dim=-1)) / rnd  # [Ns, Na, Nb, nC]
        if class_weights is not None:
            per_class = per_class * _vector(class_weights, nc, step_preds, "class_weights")
        return th.where(q != 0, q * per_class, th.zeros_like(per_class)).sum(dim=-1)
    ce = -th.log_softmax(step_preds, dim=-1).gather(-1, y.view(1, 1, nb, 1).expand(ns, na, nb, 1)).squeeze(-1)
    rnd = math.log(nc)
    rew = (rnd - ce) / rnd
    if class_weights is not None:
        rew = rew * _vector(class_weights, nc, step_preds, "class_weights")[y]
    return rew


def balanced_weights(labels, nb_class: int) -> th.Tensor:
    """N / (nC * n_c) per class from a vector of integer labels (fp32 [nb_class]); a class with no sample gets 0."""
    lab = th.as_tensor(labels).reshape(-1).to("cpu", th.int64)
    if lab.numel() == 0:
        raise ValueError("balanced_weights: no labels")
    if int(lab.min()) < 0 or int(lab.max()) >= nb_class:
        raise ValueError(f"balanced_weights: labels outside [0, {nb_class})")
    n = th.bincount(lab, minlength=nb_class).to(th.float64)
    w = th.where(n > 0, lab.numel() / (nb_class * n.clamp(min=1.0)), th.zeros_like(n))
    return w.to(th.float32)


def step_schedule(spec: Union[str, Sequence[float]], nb_steps: int) -> Tuple[float, ...]:
    """Step weights [nb_steps] from ``all`` (ones), ``last`` (= ``last:1``), ``last:K`` (ones on the last K steps, zeros
    before), ``linear`` (s_t = (t + 1) / Ns) or a sequence of nb_steps floats."""
    if not isinstance(spec, str):
        return check_vector(spec, "step weights", nb_steps)
    k = parse_error_steps(spec)
    if k == "all":
        return (1.0,) * nb_steps
    if k == "linear":
        return tuple((t + 1) / nb_steps for t in range(nb_steps))
    last = 1 if k == "last" else int(k.split(":")[1])
    if last > nb_steps:
        raise ValueError(f'step weights "{spec}": the episode has {nb_steps} steps')
    return (0.0,) * (nb_steps - last) + (1.0,) * last


def parse_error_steps(text: str) -> str:
    """``--error-steps all|last[:K]|linear``: the checked spelling (K >= 1; K <= Ns is checked where Ns is known)."""
    m = re.fullmatch(r"all|linear|last(?::([1-9]\d*))?", text) if isinstance(text, str) else None
    if not m:
        raise ValueError(f'unknown error steps "{text}" (all, last, last:K with K >= 1, or linear)')
    return text


def parse_class_weights(text: str):
    """``--class-weights balanced|FILE.npy|w0,w1,...``: "balanced", the path, or the tuple of floats (finite, >= 0, not
    all zero; the length is checked against --nb-class where it is known)."""
    if not isinstance(text, str) or not text:
        raise ValueError("class weights: balanced, FILE.npy or w0,w1,...")
    if text == "balanced" or text.endswith(".npy"):
        return text
    parts = text.split(",")
    if not all(re.fullmatch(_NUM, p.strip()) for p in parts):
        raise ValueError(f'unknown class weights "{text}" (balanced, FILE.npy or w0,w1,...)')
    return check_vector([float(p) for p in parts], "class weights", len(parts))


def resolve_class_weights(spec, nb_class: int, labels=None) -> Optional[Tuple[float, ...]]:
    """What ``parse_class_weights`` returned as the checked vector: ``balanced`` from ``labels`` (the whole training
    split), a .npy file loaded, a tuple checked for its length; None stays None."""
    if spec is None:
        return None
    if isinstance(spec, str) and spec == "balanced":
        if labels is None:
            raise ValueError("class weights: balanced needs the training labels")
        return check_vector(balanced_weights(labels, nb_class), "class weights", nb_class)
    if isinstance(spec, str):
        import numpy as np

        return check_vector(np.load(spec).reshape(-1), f'class weights of "{spec}"', nb_class)
    return check_vector(spec, "class weights", nb_class)


def from_options(nb_class: int, nb_steps: int, class_weights=None, label_smoothing: float = 0.0,
                 error_step_weights=None, weight_rewards: bool = False) -> Optional[ClassLoss]:
    """The ``ClassLoss`` of ``Trainer`` / ``FusedA2C`` keywords for an episode of ``nb_steps`` steps
    (``error_step_weights``: a ``step_schedule`` spec or a sequence); None when all four are at their defaults - the
    caller then makes today's sequence of library calls, verbatim."""
    if class_weights is None and error_step_weights is None and label_smoothing == 0.0 and not weight_rewards:
        return None
    sw = None if error_step_weights is None else step_schedule(error_step_weights, nb_steps)
    return ClassLoss(nb_class, nb_steps, class_weights, label_smoothing, sw, weight_rewards)
