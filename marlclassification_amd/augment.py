"""Device-side augmentation fused into the batch gather: random flips, quarter-turn rotations, small shifts and random
erasing of images that already live in HBM (``data.ResidentLoader``, ``data.DevicePrefetcher``), the command line's
``train --augment SPEC`` and test-time augmentation ``test --tta SPEC``.

Per output image ``b`` the transform is a source row ``rows[b]`` and eight int32 values
``ops[b] = (d4, dy, dx, ey, ex, eh, ew, 0)``.  Output pixel ``(c, y, x)`` of an ``H x W`` image is

1. ``fill`` if ``ey <= y < ey + eh and ex <= x < ex + ew`` (random erasing; ``eh == 0`` or ``ew == 0``: none);
2. else with ``y' = y - dy, x' = x - dx``: pad mode ``zero`` gives ``fill`` outside the image, ``reflect`` folds like
   ``torch.nn.functional.pad(mode="reflect")`` (the edge is not repeated);
3. then the dihedral code: ``d4 & 1`` swaps ``(y', x')``, ``d4 & 2`` sets ``x' = W-1-x'``, ``d4 & 4`` sets ``y' = H-1-y'``;
4. ``src[rows[b], c, y', x']``.

So ``d4`` = 0 identity, 2 ``flip(-1)``, 4 ``flip(-2)``, 6 ``rot90(k=2)``, 1 transpose, 3 ``rot90(k=1)``, 5 ``rot90(k=-1)``,
7 the anti-transpose.  Nothing in ``ops`` / ``rows`` is trusted (they are device tensors nobody inspects): ``d4 & 7``
(bit 0 dropped where ``H != W``), rows clamped to ``[0, N)``, ``|dy| <= H-1`` and ``|dx| <= W-1`` by clamping, the
rectangle intersected with the image.  ``reference_apply`` is this definition in plain torch, on any device; ``apply``
is the product: one kernel of libmarl_hip.so (include/marl_hip_augment.h), bit for bit the same.

Rotation by any angle, zoom and aspect stretch (``rotate:DEG``, ``scale:LO:HI``, ``stretch:R``, the test-time
``zoom:Z1/Z2/...``) are no index remapping: a policy with one of them (``Policy.has_warp``) draws a matrix per image
besides the ops (``Policy.draw_warp``, ``Policy.warp_views``) and its batches go through the resampling gather of
``warp.py``.
"""

from __future__ import annotations

import ctypes as C
import math
import struct
from dataclasses import dataclass
from typing import Optional, Tuple

import torch as th

PAD_MODES = {"zero": 0, "reflect": 1}  # MARL_AUGMENT_PAD_* of include/marl_hip_augment.h
OPS_WIDTH = 8


# ---- the definition -----------------------------------------------------------------------------------------------
def _batch_of(src: th.Tensor, rows, ops) -> int:
    if rows is not None:
        return int(rows.shape[0])
    return int(ops.shape[0]) if ops is not None else int(src.shape[0])


def _check_pad(pad_mode: str) -> int:
    if pad_mode not in PAD_MODES:
        raise ValueError(f'augment: unknown pad mode "{pad_mode}" (reflect or zero)')
    return PAD_MODES[pad_mode]


def reference_apply(src: th.Tensor, rows: Optional[th.Tensor] = None, ops: Optional[th.Tensor] = None,
                    pad_mode: str = "reflect", fill=0) -> th.Tensor:
    """The transform of the module docstring in plain torch: ``src`` ``[N, C, H, W]`` (any dtype, any device), ``rows``
    ``[B]`` integers (None: ``rows[b] = b``), ``ops`` ``[B, 8]`` integers (None: zeros) -> ``[B, C, H, W]``."""
    reflect = _check_pad(pad_mode) == 1
    n, c, h, w = src.shape
    nb = _batch_of(src, rows, ops)
    dev = src.device
    rows = th.arange(nb, device=dev) if rows is None else rows.to(dev, th.int64)
    ops = th.zeros(nb, OPS_WIDTH, dtype=th.int64, device=dev) if ops is None else ops.to(dev, th.int64)
    if rows.shape != (nb,) or ops.shape != (nb, OPS_WIDTH):
        raise ValueError(f"augment: rows {tuple(rows.shape)} / ops {tuple(ops.shape)} do not describe {nb} images")
    rows = rows.clamp(0, n - 1)
    d4 = ops[:, 0] & (7 if h == w else 6)
    dy, dx = ops[:, 1].clamp(-(h - 1), h - 1), ops[:, 2].clamp(-(w - 1), w - 1)
    ey0, ey1 = ops[:, 3].clamp(0, h), (ops[:, 3] + ops[:, 5]).clamp(0, h)
    ex0, ex1 = ops[:, 4].clamp(0, w), (ops[:, 4] + ops[:, 6]).clamp(0, w)

    def b3(t):
        return t.view(nb, 1, 1)

    ys, xs = th.arange(h, device=dev).view(1, h, 1), th.arange(w, device=dev).view(1, 1, w)
    vy, vx = ys - b3(dy), xs - b3(dx)  # [B, H, 1], [B, 1, W]
    if reflect:
        vy, vx = vy.abs(), vx.abs()
        vy, vx = th.where(vy >= h, 2 * (h - 1) - vy, vy), th.where(vx >= w, 2 * (w - 1) - vx, vx)
        outside = th.zeros(nb, h, w, dtype=th.bool, device=dev)
    else:
        outside = ((vy < 0) | (vy >= h)) | ((vx < 0) | (vx >= w))
        vy, vx = vy.clamp(0, h - 1), vx.clamp(0, w - 1)
    yy, xx = vy.expand(nb, h, w), vx.expand(nb, h, w)
    swap = b3((d4 & 1) != 0)
    yy, xx = th.where(swap, xx, yy), th.where(swap, yy, xx)
    xx = th.where(b3((d4 & 2) != 0), w - 1 - xx, xx)
    yy = th.where(b3((d4 & 4) != 0), h - 1 - yy, yy)
    lin = (yy * w + xx).view(nb, 1, h * w).expand(nb, c, h * w)
    out = src.index_select(0, rows).reshape(nb, c, h * w).gather(2, lin).view(nb, c, h, w)
    erased = ((ys >= b3(ey0)) & (ys < b3(ey1))) & ((xs >= b3(ex0)) & (xs < b3(ex1)))
    return th.where((erased | outside).unsqueeze(1), th.as_tensor(fill, dtype=src.dtype, device=dev), out)


# ---- the policy and its command-line spelling ---------------------------------------------------------------------
@dataclass(frozen=True)
class Policy:
    """What ``parse`` returns: which dihedral codes may be drawn, the shift range, the erased square."""

    hflip: bool = False
    vflip: bool = False
    rot90: bool = False
    d4: bool = False
    shift: int = 0
    pad_mode: str = "reflect"
    erase: int = 0
    erase_p: float = 0.5
    fill: int = 0
    spec: str = ""
    rotate: float = 0.0                        # rotate:DEG - theta uniform in [-DEG, DEG]; 0: off
    scale: Tuple[float, float] = (1.0, 1.0)    # scale:LO:HI - zoom log-uniform in [LO, HI]
    stretch: float = 1.0                       # stretch:R - aspect log-uniform in [1/R, R]
    zooms: Tuple[float, ...] = ()              # zoom:Z1/Z2/... - test-time views only (parse_tta)

    @property
    def has_warp(self) -> bool:
        """The policy resamples (``warp.apply`` with ``draw_warp`` / ``warp_views``) rather than remaps indices."""
        return self.rotate > 0 or self.scale != (1.0, 1.0) or self.stretch != 1.0 or len(self.zooms) > 0

    def group(self) -> Tuple[int, ...]:
        """The ``d4`` codes the spec allows."""
        if self.d4 or (self.rot90 and (self.hflip or self.vflip)):
            return (0, 1, 2, 3, 4, 5, 6, 7)
        if self.rot90:
            return (0, 3, 6, 5)
        if self.hflip and self.vflip:
            return (0, 2, 4, 6)
        if self.hflip:
            return (0, 2)
        if self.vflip:
            return (0, 4)
        return (0,)

    def check_size(self, h: int, w: int) -> None:
        """Codes with bit 0 (transposes, quarter turns) need square images."""
        if h != w and any(code & 1 for code in self.group()):
            raise ValueError(f'augment "{self.spec}": quarter turns and transposes need square images, got {h} x {w}')

    def draw(self, batch: int, generator: th.Generator, size: Optional[Tuple[int, int]] = None) -> th.Tensor:
        """``ops`` ``[batch, 8]`` int32 on the generator's device, torch ops only (no host synchronisation): ``d4``
        uniform over the group, ``dy, dx`` uniform in ``[-shift, shift]``, and with probability ``erase_p`` an
        ``erase x erase`` square at a uniform position inside the ``size = (H, W)`` image (needed with erasing only)."""
        dev = generator.device
        ops = th.zeros(batch, OPS_WIDTH, dtype=th.int32, device=dev)
        group = self.group()
        if len(group) > 1:
            # (pick -> code by comparisons: a code table would be a host tensor, and its upload a synchronisation)
            pick = th.randint(0, len(group), (batch,), generator=generator, device=dev, dtype=th.int32)
            for i, code in enumerate(group):
                if code:
                    ops[:, 0] += (pick == i).to(th.int32) * code
        if self.shift > 0:
            ops[:, 1:3] = th.randint(-self.shift, self.shift + 1, (batch, 2), generator=generator, device=dev,
                                     dtype=th.int32)
        if self.erase > 0:
            if size is None:
                raise ValueError("augment: draw(..., size=(H, W)) is needed to place the erased square")
            h, w = size
            on = th.rand(batch, generator=generator, device=dev) < self.erase_p
            ops[:, 3] = th.randint(0, max(h - self.erase, 0) + 1, (batch,), generator=generator, device=dev,
                                   dtype=th.int32)
            ops[:, 4] = th.randint(0, max(w - self.erase, 0) + 1, (batch,), generator=generator, device=dev,
                                   dtype=th.int32)
            ops[:, 5:7] = (on.to(th.int32) * self.erase).unsqueeze(1)
        return ops

    def draw_warp(self, batch: int, generator: th.Generator,
                  size: Optional[Tuple[int, int]] = None) -> Tuple[th.Tensor, th.Tensor]:
        """``(ops, mats)`` on the generator's device, torch ops only (no host synchronisation).  The ops are drawn FIRST
        through ``draw`` (a policy without warp tokens consumes the generator exactly as ``draw`` does), then one
        uniform per image for each of ``rotate`` / ``scale`` / ``stretch`` the spec has, in this order; ``mats`` are
        ``warp.matrices`` of them (``[batch, 8]`` int32)."""
        from . import warp as _warp

        ops = self.draw(batch, generator, size)
        dev = generator.device

        def uniform():
            return th.rand(batch, generator=generator, device=dev)

        angle = (2.0 * uniform() - 1.0) * self.rotate if self.rotate > 0 else th.zeros(batch, device=dev)
        lo, hi = math.log(self.scale[0]), math.log(self.scale[1])
        zoom = th.exp(lo + uniform() * (hi - lo)) if self.scale != (1.0, 1.0) else th.ones(batch, device=dev)
        ratio = (th.exp((2.0 * uniform() - 1.0) * math.log(self.stretch)) if self.stretch != 1.0
                 else th.ones(batch, device=dev))
        return ops, _warp.matrices(angle, zoom, ratio)

    def warp_views(self) -> Tuple[th.Tensor, th.Tensor]:
        """Test-time augmentation under ``zoom:Z1/Z2/...``: ``(ops, mats)`` on the CPU, one row per (zoom, code) - the
        zooms in the spec's order (none: 1), under each the codes of the group in ``views``' order."""
        from . import warp as _warp

        codes = self.views()
        zooms = th.tensor(self.zooms or (1.0,), dtype=th.float32)
        mats = _warp.matrices(th.zeros_like(zooms), zooms, th.ones_like(zooms))
        return codes.repeat(zooms.shape[0], 1), mats.repeat_interleave(codes.shape[0], dim=0)

    def views(self) -> th.Tensor:
        """Test-time augmentation: one op row per code of the group, in the group's order (``[len(group), 8]`` int32
        on the CPU).  Random parts have no deterministic view: a spec with ``shift`` / ``erase`` is refused."""
        if self.shift > 0 or self.erase > 0:
            raise ValueError(f'augment "{self.spec}": shift / erase have no test-time views (flips and rotations do)')
        if self.rotate > 0 or self.scale != (1.0, 1.0) or self.stretch != 1.0:
            raise ValueError(f'augment "{self.spec}": rotate / scale / stretch are random and have no test-time views '
                             "(zoom:Z1/Z2/... has)")
        ops = th.zeros(len(self.group()), OPS_WIDTH, dtype=th.int32)
        ops[:, 0] = th.tensor(self.group(), dtype=th.int32)
        return ops


def _int(text: str, token: str, lo: int) -> int:
    if not text.isdigit() or int(text) < lo:
        raise ValueError(f'augment: bad token "{token}" (an integer >= {lo} is expected)')
    return int(text)


def _floats(texts, token: str, lo: float, hi: float, what: str):
    try:
        values = [float(t) for t in texts]
    except ValueError:
        values = [float("nan")]
    if not values or not all(lo <= v <= hi for v in values):  # (NaN fails too)
        raise ValueError(f'augment: bad token "{token}" ({what})')
    return values


def parse(spec: str) -> Policy:
    """``hflip``, ``vflip``, ``rot90``, ``d4``, ``shift:T[:reflect|zero]`` (default reflect), ``erase:S[:p]`` (default
    p = 0.5, fill 0), ``rotate:DEG`` (0 < DEG <= 180), ``scale:LO:HI`` (1/16 <= LO <= HI <= 16), ``stretch:R``
    (1 <= R <= 4), comma-separated.  Anything else: ValueError naming the token."""
    return _parse(spec, tta=False)


def _parse(spec: str, tta: bool) -> Policy:
    if not isinstance(spec, str):
        raise ValueError(f"augment: the spec must be a string, got {spec!r}")
    kw = {}
    for token in (t.strip() for t in spec.split(",")):
        head, *rest = token.split(":")
        if head in ("hflip", "vflip", "rot90", "d4") and not rest:
            kw[head] = True
        elif head == "shift" and 1 <= len(rest) <= 2:
            kw["shift"] = _int(rest[0], token, 0)
            if len(rest) == 2:
                if rest[1] not in PAD_MODES:
                    raise ValueError(f'augment: bad token "{token}" (the pad mode is reflect or zero)')
                kw["pad_mode"] = rest[1]
        elif head == "erase" and 1 <= len(rest) <= 2:
            kw["erase"] = _int(rest[0], token, 1)
            if len(rest) == 2:
                try:
                    p = float(rest[1])
                except ValueError:
                    p = -1.0
                if not 0.0 <= p <= 1.0:  # (NaN fails too)
                    raise ValueError(f'augment: bad token "{token}" (the probability lies in [0, 1])')
                kw["erase_p"] = p
        elif head == "rotate" and len(rest) == 1:
            kw["rotate"] = _floats(rest, token, 0.0, 180.0, "an angle in (0, 180] degrees is expected")[0]
            if kw["rotate"] == 0.0:
                raise ValueError(f'augment: bad token "{token}" (an angle in (0, 180] degrees is expected)')
        elif head == "scale" and len(rest) == 2:
            lo, hi = _floats(rest, token, 1.0 / 16, 16.0, "1/16 <= LO <= HI <= 16 is expected")
            if lo > hi:
                raise ValueError(f'augment: bad token "{token}" (1/16 <= LO <= HI <= 16 is expected)')
            kw["scale"] = (lo, hi)
        elif head == "stretch" and len(rest) == 1:
            kw["stretch"] = _floats(rest, token, 1.0, 4.0, "an aspect ratio in [1, 4] is expected")[0]
        elif head == "zoom" and len(rest) == 1:
            if not tta:
                raise ValueError(f'augment: bad token "{token}" (zoom views exist at test time only: test --tta; '
                                 "scale:LO:HI draws zooms in training)")
            kw["zooms"] = tuple(_floats(rest[0].split("/"), token, 1.0 / 16, 16.0,
                                        "zoom factors Z1/Z2/... in [1/16, 16] are expected"))
        else:
            raise ValueError(f'augment: unknown token "{token}" (hflip, vflip, rot90, d4, shift:T[:reflect|zero], '
                             "erase:S[:p], rotate:DEG, scale:LO:HI, stretch:R; test --tta also zoom:Z1/Z2/...)")
    return Policy(spec=spec, **kw)


def parse_tta(spec: str) -> Policy:
    """``test --tta SPEC``: a spec with deterministic views only - the flips and rotations, and ``zoom:Z1/Z2/...``
    (every code of the group under every zoom factor: ``Policy.warp_views``)."""
    policy = _parse(spec, tta=True)
    policy.views()
    return policy


# ---- the product: one kernel of libmarl_hip.so ----------------------------------------------------------------------
class AugmentPlan(C.Structure):
    """Mirror of ``marl_augment_plan_info`` (include/marl_hip_augment.h)."""

    _fields_ = [(name, C.c_int32) for name in
                "store_bytes band_vectors tile_h tile_w tr_tile lds_bytes blocks_per_image reserved".split()]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


def _fill_bits(fill, dtype: th.dtype) -> int:
    if dtype == th.uint8:
        if int(fill) != fill or not 0 <= int(fill) <= 255:
            raise ValueError(f"augment: fill {fill!r} is no uint8 value")
        return int(fill)
    return struct.unpack("<I", struct.pack("<f", float(fill)))[0]


def _need_images(t: th.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} lives on {t.device}: the HIP path only runs on a GPU "
                           "(there is no CPU implementation in this package; augment.reference_apply is the definition)")
    if t.dtype not in (th.uint8, th.float32):
        raise TypeError(f"{name} must be uint8 or float32, got {t.dtype}")
    if t.dim() != 4 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [N, C, H, W] tensor, got {tuple(t.shape)}")


def _launch(who: str, entry: str, src: th.Tensor, nb: int, rows: Optional[th.Tensor], tables, mode: int, fill,
            out: Optional[th.Tensor], rows_shape: str = "B", ready=None) -> th.Tensor:
    """What the ``apply`` of ``augment``, ``mix`` and ``warp`` share, behind their pad-mode, ``src`` and batch-size
    checks: ``rows``, the int32 ``[nb, width]`` ``tables`` (``(name, tensor or None, width)`` in the order ``entry``
    takes them) and ``out`` are checked (``out`` allocated if None), then ``entry`` of libmarl_hip.so is called on the
    current stream.  ``ready()``, if given, is called once everything is checked and returns the tensors to pass in
    place of the tables."""
    from . import _lib

    dev = src.device
    if rows is not None and (rows.device != dev or rows.dtype != th.int64 or tuple(rows.shape) != (nb,)
                             or not rows.is_contiguous()):
        raise ValueError(f"{who}: rows must be a contiguous int64 [{rows_shape}] tensor on {dev}")
    for name, t, width in tables:
        if t is not None and (t.device != dev or t.dtype != th.int32 or tuple(t.shape) != (nb, width)
                              or not t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be a contiguous int32 [{nb}, {width}] tensor on {dev}")
    shape = (nb,) + tuple(src.shape[1:])
    if out is None:
        out = th.empty(shape, dtype=src.dtype, device=dev)
    else:
        _need_images(out, f"{who}: out")
        if out.device != dev or out.dtype != src.dtype or tuple(out.shape) != shape:
            raise ValueError(f"{who}: out must be a {src.dtype} {shape} tensor on {dev}")
    if nb == 0:
        return out
    bits = _fill_bits(fill, src.dtype)
    tensors = ready() if ready is not None else [t for _, t, _ in tables]
    with th.cuda.device(dev):
        _lib.check(getattr(_lib.load(), entry)(
            src.data_ptr(), src.shape[0], out.data_ptr(), None if rows is None else rows.data_ptr(),
            *(None if t is None else t.data_ptr() for t in tensors), nb, src.shape[1], src.shape[2], src.shape[3],
            src.element_size(), mode, bits, th.cuda.current_stream(dev).cuda_stream))
    return out


def plan(src: th.Tensor, out: th.Tensor) -> dict:
    """What ``apply(src, ..., out=out)`` launches (``marl_batch_augment_plan``): store width, tiles, LDS bytes."""
    from . import _lib

    info = AugmentPlan()
    _, c, h, w = src.shape
    _lib.check(_lib.load().marl_batch_augment_plan(c, h, w, src.element_size(), src.data_ptr(), out.data_ptr(),
                                                   C.byref(info)))
    return info.as_dict()


def apply(src: th.Tensor, rows: Optional[th.Tensor] = None, ops: Optional[th.Tensor] = None,
          pad_mode: str = "reflect", fill=0, out: Optional[th.Tensor] = None) -> th.Tensor:
    """``reference_apply`` on GPU tensors, as one launch on the current stream: ``src`` contiguous ``[N, C, H, W]``
    uint8 or float32, ``rows`` int64 ``[B]`` (None: row b for image b), ``ops`` int32 ``[B, 8]`` (None: a plain
    gather), ``out`` (None: a fresh tensor) must not overlap ``src``."""
    mode = _check_pad(pad_mode)
    _need_images(src, "augment.apply: src")
    return _launch("augment.apply", "marl_batch_augment", src, _batch_of(src, rows, ops), rows,
                   [("ops", ops, OPS_WIDTH)], mode, fill, out)
