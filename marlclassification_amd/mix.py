"""CutMix and Mixup fused into the augmenting batch gather, and the target distributions that go with them:
``data.ResidentLoader`` / ``data.DevicePrefetcher`` (``mix=``), the command line's ``train --mix SPEC`` and
``Trainer.train_step(..., targets=Q)``.

``rows`` and ``ops`` mean what they mean in ``augment``; VIEW ``i`` is ``augment.reference_apply`` of
``(rows[i], ops[i])``.  Per output image ``b`` eight int32 values ``mix[b] = (partner, mode, by, bx, bh, bw, k, 0)``;
with ``p = partner``, output pixel ``(c, y, x)`` of image ``b`` is

* mode 0: view ``b``;
* mode 1 (CutMix): view ``p`` where ``by <= y < by + bh and bx <= x < bx + bw``, else view ``b``;
* mode 2 (Mixup): uint8 ``(k * view_b + (256 - k) * view_p + 128) >> 8`` in integer arithmetic, ``k`` in ``[0, 256]``;
  float ``(k / 256) * view_b + ((256 - k) / 256) * view_p``, each product and the sum rounded on its own (both factors
  are exact in fp32).

The partner's view is taken under the partner's OWN row and ops: the batch mixed with a permutation of itself.  Nothing
in ``mix`` is trusted (a device tensor nobody inspects): ``partner`` clamped to ``[0, B)``, ``mode & 3`` with 3 read as
0, the box intersected with the image, ``k`` clamped to ``[0, 256]``.  ``reference_apply`` is this definition in plain
torch, on any device; ``apply`` is the product: one kernel of libmarl_hip.so (include/marl_hip_mix.h), bit for bit the
same.

The share of image ``b``'s own label is ``lam`` = 1 (mode 0), ``(H W - clipped box area) / (H W)`` (CutMix), ``k / 256``
(Mixup): ``label_weights``; ``soft_targets`` makes ``Q[b] = lam e_{y_b} + (1 - lam) e_{y_p}`` for the fused loss
(include/marl_hip_softtargets.h) and ``primary_labels`` the hard label of the larger share, for the meters.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch as th

from . import augment as _augment

MIX_WIDTH = 8
MODE_NONE, MODE_CUTMIX, MODE_MIXUP = 0, 1, 2  # MARL_MIX_* of include/marl_hip_mix.h


# ---- the definition -----------------------------------------------------------------------------------------------
def _sanitised(mix: th.Tensor, batch: int, h: int, w: int):
    """``mix`` [B, 8] as the kernel uses it: (partner, mode, by0, by1, bx0, bx1, k), int64 [B] each"""
    if mix.dim() != 2 or tuple(mix.shape) != (batch, MIX_WIDTH):
        raise ValueError(f"mix: {tuple(mix.shape)} does not describe {batch} images ([B, {MIX_WIDTH}] integers)")
    m = mix.to(th.int64)
    partner = m[:, 0].clamp(0, batch - 1)
    mode = m[:, 1] & 3
    mode = th.where(mode == 3, th.zeros_like(mode), mode)
    by0, by1 = m[:, 2].clamp(0, h), (m[:, 2] + m[:, 4]).clamp(0, h)
    bx0, bx1 = m[:, 3].clamp(0, w), (m[:, 3] + m[:, 5]).clamp(0, w)
    return partner, mode, by0, by1, bx0, bx1, m[:, 6].clamp(0, 256)


def reference_apply(src: th.Tensor, rows: Optional[th.Tensor] = None, ops: Optional[th.Tensor] = None,
                    mix: Optional[th.Tensor] = None, pad_mode: str = "reflect", fill=0) -> th.Tensor:
    """The mix of the module docstring in plain torch: ``src`` ``[N, C, H, W]`` (any device), ``rows`` ``[B]`` integers
    (None: ``rows[b] = b``), ``ops`` ``[B, 8]`` integers (None: zeros), ``mix`` ``[B, 8]`` integers (None: zeros) ->
    ``[B, C, H, W]``."""
    if rows is None and ops is None and mix is not None:
        rows = th.arange(mix.shape[0], device=src.device)
    views = _augment.reference_apply(src, rows, ops, pad_mode, fill)
    if mix is None:
        return views
    nb, _, h, w = views.shape
    dev = views.device
    partner, mode, by0, by1, bx0, bx1, k = _sanitised(mix.to(dev), nb, h, w)
    other = views.index_select(0, partner)

    def b3(t):
        return t.view(nb, 1, 1)

    ys, xs = th.arange(h, device=dev).view(1, h, 1), th.arange(w, device=dev).view(1, 1, w)
    inbox = ((ys >= b3(by0)) & (ys < b3(by1))) & ((xs >= b3(bx0)) & (xs < b3(bx1)))
    cut = th.where(inbox.unsqueeze(1), other, views)
    k4 = k.view(nb, 1, 1, 1)
    if views.dtype == th.uint8:
        blend = ((k4 * views.to(th.int64) + (256 - k4) * other.to(th.int64) + 128) >> 8).to(th.uint8)
    else:
        fb, fp = (k4.to(views.dtype) / 256), ((256 - k4).to(views.dtype) / 256)
        blend = (fb * views) + (fp * other)  # two products and a sum, each rounded: no fused multiply-add
    m4 = mode.view(nb, 1, 1, 1)
    return th.where(m4 == MODE_CUTMIX, cut, th.where(m4 == MODE_MIXUP, blend, views))


def _shares(mix: th.Tensor, h: int, w: int):
    """(own numerator, partner's numerator, denominator, partner) as int64 [B]: the two shares are exact integer
    fractions, the complement taken from the integers too"""
    partner, mode, by0, by1, bx0, bx1, k = _sanitised(mix, mix.shape[0], h, w)
    area = (by1 - by0).clamp(min=0) * (bx1 - bx0).clamp(min=0)
    hw = th.full_like(area, h * w)
    one, zero = th.ones_like(area), th.zeros_like(area)
    cutmix, mixup = mode == MODE_CUTMIX, mode == MODE_MIXUP
    own = th.where(cutmix, hw - area, th.where(mixup, k, one))
    par = th.where(cutmix, area, th.where(mixup, 256 - k, zero))
    den = th.where(cutmix, hw, th.where(mixup, th.full_like(area, 256), one))
    return own, par, den, partner


def label_weights(mix: th.Tensor, h: int, w: int) -> th.Tensor:
    """``lam`` fp32 ``[B]``: 1 (mode 0), ``(h w - clipped box area) / (h w)`` (CutMix), ``k / 256`` (Mixup).  Torch ops
    on ``mix``'s device, no host synchronisation."""
    own, _, den, _ = _shares(mix, h, w)
    return own.to(th.float32) / den.to(th.float32)


def soft_targets(y: th.Tensor, mix: th.Tensor, h: int, w: int, nb_class: int) -> th.Tensor:
    """``Q`` fp32 ``[B, nb_class]`` = ``lam e_{y_b} + (1 - lam) e_{y_p}`` (both shares from their integer numerators:
    a row sums to 1 within one fp32 ulp, and is exactly one-hot where the mode is 0).  Torch ops on ``mix``'s device,
    no host synchronisation."""
    own, par, den, partner = _shares(mix, h, w)
    y = y.to(mix.device, th.int64)
    if y.shape != (mix.shape[0],):
        raise ValueError(f"mix: labels {tuple(y.shape)} for {mix.shape[0]} images")
    den = den.to(th.float32)
    q = th.zeros(mix.shape[0], nb_class, dtype=th.float32, device=mix.device)
    q.scatter_add_(1, y.view(-1, 1), (own.to(th.float32) / den).view(-1, 1))
    q.scatter_add_(1, y.index_select(0, partner).view(-1, 1), (par.to(th.float32) / den).view(-1, 1))
    return q


def primary_labels(y: th.Tensor, mix: th.Tensor, h: int, w: int) -> th.Tensor:
    """``y_b`` where ``lam >= 0.5`` (decided on the integers), else ``y_p``: the hard label the confusion meters take."""
    own, _, den, partner = _shares(mix, h, w)
    y = y.to(mix.device)
    return th.where(2 * own >= den, y, y.index_select(0, partner))


# ---- the policy and its command-line spelling ---------------------------------------------------------------------
@dataclass(frozen=True)
class Policy:
    """What ``parse`` returns: per image, CutMix with probability ``cutmix_p`` (``lam' ~ Beta(cutmix_alpha,
    cutmix_alpha)``), Mixup with ``mixup_p`` (``Beta(mixup_alpha, mixup_alpha)``), else nothing."""

    cutmix_alpha: float = 1.0
    cutmix_p: float = 0.0
    mixup_alpha: float = 1.0
    mixup_p: float = 0.0
    spec: str = ""

    def __post_init__(self) -> None:
        for name in ("cutmix_alpha", "mixup_alpha"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and math.isfinite(v) and v > 0):
                raise ValueError(f"mix: {name} must be a finite number > 0, got {v!r}")
        for name in ("cutmix_p", "mixup_p"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and 0.0 <= v <= 1.0):
                raise ValueError(f"mix: {name} must lie in [0, 1], got {v!r}")
        if self.cutmix_p + self.mixup_p > 1.0:
            raise ValueError(f"mix: the probabilities {self.cutmix_p} + {self.mixup_p} sum to more than 1")

    @staticmethod
    def beta(alpha: float, batch: int, generator: th.Generator) -> th.Tensor:
        """``lam' ~ Beta(alpha, alpha)`` fp32 ``[batch]`` on the generator's device, as the ratio of two gamma draws from
        the generator (where both underflow to 0 - alpha far below 0.01 - the draw is 1/2)."""
        shape = th.full((2, batch), float(alpha), dtype=th.float32, device=generator.device)
        g = th._standard_gamma(shape, generator=generator)
        total = g[0] + g[1]
        return th.where(total > 0, g[0] / total, th.full_like(total, 0.5))

    def draw(self, batch: int, generator: th.Generator, size: Tuple[int, int]) -> th.Tensor:
        """``mix`` ``[batch, 8]`` int32 on the generator's device, from the generator only, torch ops only (no host
        synchronisation): ``partner`` a permutation of the batch, the mode by the two probabilities, the CutMix box
        with sides ``round(sqrt(1 - lam') (H, W))`` around a uniform centre, clipped to the image, and
        ``k = round(256 lam')``.  Images with mode 0 get a zero box and ``k = 256``."""
        h, w = size
        dev = generator.device
        mix = th.zeros(batch, MIX_WIDTH, dtype=th.int32, device=dev)
        mix[:, 0] = th.randperm(batch, generator=generator, device=dev).to(th.int32)
        u = th.rand(batch, generator=generator, device=dev)
        cut = u < self.cutmix_p
        mup = (~cut) & (u < self.cutmix_p + self.mixup_p)
        mix[:, 1] = cut.to(th.int32) * MODE_CUTMIX + mup.to(th.int32) * MODE_MIXUP
        lam_c = self.beta(self.cutmix_alpha, batch, generator)
        lam_m = self.beta(self.mixup_alpha, batch, generator)
        centre = th.rand(batch, 2, generator=generator, device=dev)
        ratio = th.sqrt(1.0 - lam_c)
        for col, n, j in ((2, h, 0), (3, w, 1)):
            side = th.round(ratio * n).to(th.int64)
            c = (centre[:, j] * n).to(th.int64).clamp(max=n - 1)
            lo = (c - side // 2).clamp(0, n)
            hi = (c - side // 2 + side).clamp(0, n)
            mix[:, col] = (lo * cut).to(th.int32)
            mix[:, col + 2] = ((hi - lo) * cut).to(th.int32)
        k = th.round(256.0 * lam_m).to(th.int32).clamp(0, 256)
        mix[:, 6] = th.where(mup, k, th.full_like(k, 256))
        return mix


def _number(text: str, token: str) -> float:
    try:
        v = float(text)
    except ValueError:
        v = float("nan")
    if not math.isfinite(v):
        raise ValueError(f'mix: bad token "{token}" (a number is expected, got "{text}")')
    return v


def parse(spec: str) -> Policy:
    """``cutmix[:alpha[:p]]`` and ``mixup[:alpha[:p]]`` (defaults alpha = 1, p = 0.5), comma-separated, each at most
    once; the two probabilities must sum to at most 1.  Anything else: ValueError naming the token."""
    if not isinstance(spec, str):
        raise ValueError(f"mix: the spec must be a string, got {spec!r}")
    kw = {}
    for token in (t.strip() for t in spec.split(",")):
        head, *rest = token.split(":")
        if head not in ("cutmix", "mixup") or len(rest) > 2:
            raise ValueError(f'mix: unknown token "{token}" (cutmix[:alpha[:p]], mixup[:alpha[:p]])')
        if head + "_p" in kw:
            raise ValueError(f'mix: "{head}" is given twice in "{spec}"')
        alpha = _number(rest[0], token) if len(rest) >= 1 else 1.0
        p = _number(rest[1], token) if len(rest) == 2 else 0.5
        if not alpha > 0:
            raise ValueError(f'mix: bad token "{token}" (alpha must be > 0)')
        if not 0.0 <= p <= 1.0:
            raise ValueError(f'mix: bad token "{token}" (the probability lies in [0, 1])')
        kw[head + "_alpha"], kw[head + "_p"] = alpha, p
    return Policy(spec=spec, **kw)


# ---- the product: one kernel of libmarl_hip.so ----------------------------------------------------------------------
class MixPlan(C.Structure):
    """Mirror of ``marl_mix_plan_info`` (include/marl_hip_mix.h)."""

    _fields_ = [(name, C.c_int32) for name in "store_bytes band_vectors blocks_per_image lds_bytes".split()]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


def plan(src: th.Tensor, out: th.Tensor) -> dict:
    """What ``apply(src, ..., out=out)`` launches (``marl_batch_mix_plan``): store width, band size, workgroups."""
    from . import _lib

    info = MixPlan()
    _, c, h, w = src.shape
    _lib.check(_lib.load().marl_batch_mix_plan(c, h, w, src.element_size(), src.data_ptr(), out.data_ptr(),
                                               C.byref(info)))
    return info.as_dict()


def apply(src: th.Tensor, rows: Optional[th.Tensor] = None, ops: Optional[th.Tensor] = None,
          mix: Optional[th.Tensor] = None, pad_mode: str = "reflect", fill=0,
          out: Optional[th.Tensor] = None) -> th.Tensor:
    """``reference_apply`` on GPU tensors, as one launch on the current stream: ``src`` contiguous ``[N, C, H, W]``
    uint8 or float32, ``rows`` int64 ``[B]`` (None: row b for image b), ``ops`` int32 ``[B, 8]`` (None: zeros), ``mix``
    int32 ``[B, 8]`` (None: zeros - then byte for byte ``augment.apply``), ``out`` (None: a fresh tensor) must not
    overlap ``src``."""
    mode = _augment._check_pad(pad_mode)
    _augment._need_images(src, "mix.apply: src")
    if rows is not None:
        nb = int(rows.shape[0])
    elif ops is not None:
        nb = int(ops.shape[0])
    else:
        nb = int(mix.shape[0]) if mix is not None else int(src.shape[0])
    return _augment._launch("mix.apply", "marl_batch_mix", src, nb, rows,
                            [("ops", ops, _augment.OPS_WIDTH), ("mix", mix, MIX_WIDTH)], mode, fill, out)
