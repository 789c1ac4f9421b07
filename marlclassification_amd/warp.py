"""The resampling batch gather: rotation by any angle, zoom, aspect stretch and translation of images that already live
in HBM, sampled bilinearly inside the gather itself (``data.ResidentLoader``, ``data.DevicePrefetcher``, the command
line's ``train --augment ...,rotate:15,scale:0.8:1.25`` and ``test --tta d4,zoom:0.8/1/1.25``).

Per output image ``b`` the transform is a source row ``rows[b]`` and eight int32 values
``mats[b] = (a00, a01, a10, a11, ty, tx, 0, 0)``: a Q16 matrix (``65536`` = 1.0) that maps OUTPUT pixels to SOURCE
positions (the inverse warp) and a translation in Q16 half pixels.  Nothing is trusted: rows are clamped to ``[0, N)``,
each ``a`` to ``[-2^20, 2^20]``, each ``t`` to ``[-2^30, 2^30]``.  For output pixel ``(y, x)`` of an ``H x W`` image, in
int64::

    yc = 2y - (H-1)            xc = 2x - (W-1)                 (doubled, centred: integers)
    Sy = a00*yc + a01*xc + ty  Sx = a10*yc + a11*xc + tx
    py = (Sy + (H-1)*65536) >> 1      px likewise with W        (arithmetic shift; Q16 source pixels)
    py8 = (py + 128) >> 8 ; y0 = py8 >> 8 ; fy = py8 & 255      (x likewise: x0, fx)   weights in 1/256

The taps are ``(y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1)``.  Outside the image pad mode ``zero`` gives ``fill``,
``reflect`` folds the index, ``m = floormod(v, 2(n-1)); m >= n ? 2(n-1)-m : m`` (``n == 1``: 0) - ``augment``'s fold at
any distance.  uint8 blends in exact integers, ``top = v00*(256-fx) + v01*fx``, ``bot`` likewise,
``out = (top*(256-fy) + bot*fy + 32768) >> 16``; floating point blends as ``top = fl(fl(v00*(1-wx)) + fl(v01*wx))``,
``out = fl(fl(top*(1-wy)) + fl(bot*wy))`` with ``wx = fx/256``, every product and sum rounded on its own, and a tap of
weight 0 is skipped, not multiplied (``fx == 0``: ``top = v00`` exactly; a NaN behind a zero weight stays out).  An
erased rectangle in output space (fields 3..6 of an ``augment`` op row) comes last; ``fill`` wins inside it.

So the identity matrix is a plain gather, and every ``augment`` view ``(d4, dy, dx)`` is a matrix of entries
``0 / +-65536`` with ``t = -+2*65536*d`` (``from_ops``) whose warp equals ``augment.reference_apply`` bit for bit.
``reference_apply`` is this definition in plain torch, on any device; ``apply`` is the product: one kernel of
libmarl_hip.so (include/marl_hip_warp.h), bit for bit the same for uint8 and float32.
"""

from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch as th

from .augment import OPS_WIDTH, _check_pad, _launch, _need_images

MATS_WIDTH = 8
ONE = 65536  # 1.0 in Q16
A_MAX = 1 << 20  # |a| <= 16.0
T_MAX = 1 << 30  # |t| <= 8192 pixels


# ---- matrices -------------------------------------------------------------------------------------------------------
def identity(batch: int, device=None) -> th.Tensor:
    """``[batch, 8]`` int32 identity matrices."""
    mats = th.zeros(batch, MATS_WIDTH, dtype=th.int32, device=device)
    mats[:, 0] = ONE
    mats[:, 3] = ONE
    return mats


def _sanitised(mats: th.Tensor):
    m = mats.to(th.int64)
    return m[:, :4].clamp(-A_MAX, A_MAX), m[:, 4:6].clamp(-T_MAX, T_MAX)


def from_ops(ops: th.Tensor, h: int, w: int) -> th.Tensor:
    """The exact matrices ``[B, 8]`` int32 of the ``augment`` views ``(d4, dy, dx)`` in fields 0..2 of ``ops``
    (sanitised as ``augment`` does: ``d4 & 7``, shifts clamped to the image).  A transposing code on ``h != w`` is
    refused, as ``Policy.check_size`` refuses it; ops on a GPU are not inspected (that would be a host
    synchronisation): bit 0 is dropped there, as ``marl_batch_augment`` drops it."""
    o = ops.to(th.int64)
    if o.dim() != 2 or o.shape[1] != OPS_WIDTH:
        raise ValueError(f"warp: ops {tuple(ops.shape)} is no [B, {OPS_WIDTH}] tensor")
    d4 = o[:, 0] & 7
    if h != w:
        if not ops.is_cuda and bool((d4 & 1).any()):
            raise ValueError(f"warp: quarter turns and transposes need square images, got {h} x {w}")
        d4 = d4 & 6
    dy, dx = o[:, 1].clamp(-(h - 1), h - 1), o[:, 2].clamp(-(w - 1), w - 1)
    swap = (d4 & 1) != 0
    sx = 1 - (d4 & 2)       # +-1: d4 & 2 mirrors the source's x
    sy = 1 - ((d4 & 4) >> 1)  # +-1: d4 & 4 mirrors the source's y
    zero = th.zeros_like(d4)
    # source y is sy * (swap ? x - dx : y - dy), source x is sx * (swap ? y - dy : x - dx), in centred coordinates
    mats = th.stack([th.where(swap, zero, sy * ONE), th.where(swap, sy * ONE, zero),
                     th.where(swap, sx * ONE, zero), th.where(swap, zero, sx * ONE),
                     -2 * ONE * sy * th.where(swap, dx, dy), -2 * ONE * sx * th.where(swap, dy, dx),
                     zero, zero], dim=1)
    return mats.to(th.int32)


def compose_ops(mats: th.Tensor, ops: th.Tensor, h: int, w: int) -> th.Tensor:
    """"Warp, then view": the matrices of ``view(warp(image))`` for the ``augment`` views in fields 0..2 of ``ops`` -
    ``A = A_mats A_view``, ``t = A_mats t_view + t_mats``.  Exact in integers, because a view's matrix is a signed
    permutation (entries ``0 / +-65536``) and its ``t`` a multiple of ``2 * 65536``.  Inputs are sanitised as the kernel
    sanitises them, and the result saturates at the kernel's bounds."""
    a, t = _sanitised(mats)
    v = from_ops(ops, h, w).to(a.device, th.int64)
    if v.shape[0] != a.shape[0]:
        raise ValueError(f"warp: {a.shape[0]} matrices and {v.shape[0]} op rows")
    s = v[:, :4] // ONE                       # 0 / +-1
    d = v[:, 4:6] // ONE                      # t_view / 65536: -+2 d, integers
    out = th.zeros(a.shape[0], MATS_WIDTH, dtype=th.int64, device=a.device)
    out[:, 0] = a[:, 0] * s[:, 0] + a[:, 1] * s[:, 2]
    out[:, 1] = a[:, 0] * s[:, 1] + a[:, 1] * s[:, 3]
    out[:, 2] = a[:, 2] * s[:, 0] + a[:, 3] * s[:, 2]
    out[:, 3] = a[:, 2] * s[:, 1] + a[:, 3] * s[:, 3]
    out[:, 4] = a[:, 0] * d[:, 0] + a[:, 1] * d[:, 1] + t[:, 0]
    out[:, 5] = a[:, 2] * d[:, 0] + a[:, 3] * d[:, 1] + t[:, 1]
    out[:, :4] = out[:, :4].clamp(-A_MAX, A_MAX)
    out[:, 4:6] = out[:, 4:6].clamp(-T_MAX, T_MAX)
    return out.to(th.int32)


def matrices(angle_deg: th.Tensor, zoom: th.Tensor, stretch: th.Tensor) -> th.Tensor:
    """fp32 tensors ``[B]`` (rotation angle in degrees, zoom factor, aspect ratio ``r``) -> ``[B, 8]`` int32 on their
    device: ``A = (1/zoom) R(theta) diag(sqrt(r), 1/sqrt(r))`` in Q16 (``torch.round``), ``t = 0``.  ``zoom > 1``
    magnifies (the output shows a smaller part of the source), ``r > 1`` compresses the image vertically."""
    theta = angle_deg.to(th.float32) * (math.pi / 180.0)
    inv = 1.0 / zoom.to(th.float32)
    sr = th.sqrt(stretch.to(th.float32))
    cos, sin = th.cos(theta) * inv, th.sin(theta) * inv
    zero = th.zeros_like(cos)
    a = th.stack([cos * sr, -sin / sr, sin * sr, cos / sr, zero, zero, zero, zero], dim=1)
    return th.round(a * float(ONE)).clamp(-A_MAX, A_MAX).to(th.int32)


# ---- the definition -----------------------------------------------------------------------------------------------
def _axis(s: th.Tensor, n: int, reflect: bool):
    """``S`` (int64) of one axis -> (index of tap 0, index of tap 1, tap 0 outside, tap 1 outside, weight of tap 1)"""
    p8 = (((s + (n - 1) * ONE) >> 1) + 128) >> 8
    v0, f = p8 >> 8, p8 & 255
    v1 = v0 + 1
    if reflect:
        if n == 1:
            i0 = i1 = th.zeros_like(v0)
        else:
            p = 2 * (n - 1)
            m0, m1 = th.remainder(v0, p), th.remainder(v1, p)
            i0, i1 = th.where(m0 >= n, p - m0, m0), th.where(m1 >= n, p - m1, m1)
        return i0, i1, th.zeros_like(v0, dtype=th.bool), th.zeros_like(v0, dtype=th.bool), f
    return v0.clamp(0, n - 1), v1.clamp(0, n - 1), (v0 < 0) | (v0 >= n), (v1 < 0) | (v1 >= n), f


def reference_apply(src: th.Tensor, rows: Optional[th.Tensor], mats: th.Tensor, ops: Optional[th.Tensor] = None,
                    pad_mode: str = "reflect", fill=0) -> th.Tensor:
    """The transform of the module docstring in plain torch: ``src`` ``[N, C, H, W]`` (any dtype, any device: integer
    types blend in integers, floating types in their own precision), ``rows`` ``[B]`` integers (None:
    ``rows[b] = b``), ``mats`` ``[B, 8]`` integers, ``ops`` ``[B, 8]`` integers or None -> ``[B, C, H, W]``.  As in
    ``apply``, fields 0..2 of ``ops`` are folded into the matrices with ``compose_ops`` and fields 3..6 are the erased
    rectangle."""
    reflect = _check_pad(pad_mode) == 1
    n, c, h, w = src.shape
    dev = src.device
    if mats.dim() != 2 or mats.shape[1] != MATS_WIDTH:
        raise ValueError(f"warp: mats {tuple(mats.shape)} is no [B, {MATS_WIDTH}] tensor")
    nb = int(mats.shape[0])
    rows = th.arange(nb, device=dev) if rows is None else rows.to(dev, th.int64)
    if rows.shape != (nb,) or (ops is not None and tuple(ops.shape) != (nb, OPS_WIDTH)):
        raise ValueError(f"warp: rows {tuple(rows.shape)} / ops do not describe {nb} images")
    rows = rows.clamp(0, n - 1)
    mats = mats.to(dev)
    if ops is not None:
        ops = ops.to(dev, th.int64)
        mats = compose_ops(mats, ops, h, w)
    a, t = _sanitised(mats)

    def b3(v):
        return v.reshape(nb, 1, 1)

    ys, xs = th.arange(h, device=dev).view(1, h, 1), th.arange(w, device=dev).view(1, 1, w)
    yc, xc = 2 * ys - (h - 1), 2 * xs - (w - 1)
    sy = b3(a[:, 0]) * yc + b3(a[:, 1]) * xc + b3(t[:, 0])  # [B, H, W] int64
    sx = b3(a[:, 2]) * yc + b3(a[:, 3]) * xc + b3(t[:, 1])
    y0, y1, oy0, oy1, fy = _axis(sy, h, reflect)
    x0, x1, ox0, ox1, fx = _axis(sx, w, reflect)
    planes = src.index_select(0, rows).reshape(nb, c, h * w)
    integer = not src.dtype.is_floating_point
    fill_t = th.as_tensor(fill, dtype=src.dtype, device=dev)

    def tap(yi, xi, outside):
        lin = (yi * w + xi).view(nb, 1, h * w).expand(nb, c, h * w)
        v = planes.gather(2, lin).view(nb, c, h, w)
        v = th.where(outside.unsqueeze(1), fill_t, v)
        return v.to(th.int64) if integer else v

    v00, v01 = tap(y0, x0, oy0 | ox0), tap(y0, x1, oy0 | ox1)
    v10, v11 = tap(y1, x0, oy1 | ox0), tap(y1, x1, oy1 | ox1)
    fx, fy = fx.unsqueeze(1), fy.unsqueeze(1)
    if integer:
        top, bot = v00 * (256 - fx) + v01 * fx, v10 * (256 - fx) + v11 * fx
        out = ((top * (256 - fy) + bot * fy + 32768) >> 16).to(src.dtype)
    else:
        wx, wy = fx.to(src.dtype) / 256, fy.to(src.dtype) / 256

        def lerp(p, q, f, wgt):  # separately rounded products and sum; weight 0 is skipped, not multiplied
            return th.where(f == 0, p, p * (1 - wgt) + q * wgt)

        out = lerp(lerp(v00, v01, fx, wx), lerp(v10, v11, fx, wx), fy, wy)
    if ops is not None:
        ey0, ey1 = ops[:, 3].clamp(0, h), (ops[:, 3] + ops[:, 5]).clamp(0, h)
        ex0, ex1 = ops[:, 4].clamp(0, w), (ops[:, 4] + ops[:, 6]).clamp(0, w)
        erased = ((ys >= b3(ey0)) & (ys < b3(ey1))) & ((xs >= b3(ex0)) & (xs < b3(ex1)))
        out = th.where(erased.unsqueeze(1), fill_t, out)
    return out


# ---- the product: one kernel of libmarl_hip.so ----------------------------------------------------------------------
class WarpPlan(C.Structure):
    """Mirror of ``marl_warp_plan_info`` (include/marl_hip_warp.h)."""

    _fields_ = ([(name, C.c_int32) for name in
                 "store_bytes pixels_per_thread vectors_per_row threads blocks_per_image lds_bytes".split()] +
                [("reserved", C.c_int32 * 2)])

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


def plan(src: th.Tensor, out: th.Tensor) -> dict:
    """What ``apply(src, ..., out=out)`` launches (``marl_batch_warp_plan``): store width, pixels per thread, grid."""
    from . import _lib

    info = WarpPlan()
    _, c, h, w = src.shape
    _lib.check(_lib.load().marl_batch_warp_plan(c, h, w, src.element_size(), src.data_ptr(), out.data_ptr(),
                                                C.byref(info)))
    return info.as_dict()


def apply(src: th.Tensor, rows: Optional[th.Tensor], mats: th.Tensor, ops: Optional[th.Tensor] = None,
          pad_mode: str = "reflect", fill=0, out: Optional[th.Tensor] = None) -> th.Tensor:
    """``reference_apply`` on GPU tensors, as one launch on the current stream: ``src`` contiguous ``[N, C, H, W]``
    uint8 or float32, ``rows`` int64 ``[B]`` (None: row b for image b), ``mats`` int32 ``[B, 8]``, ``ops`` int32
    ``[B, 8]`` or None, ``out`` (None: a fresh tensor) must not overlap ``src``.  With ``ops``, its fields 0..2 (a
    dihedral code and a shift: "warp, then view") are folded into the matrices by ``compose_ops`` - a few torch ops on
    the device, no host synchronisation - and its rectangle goes to the kernel."""
    mode = _check_pad(pad_mode)
    _need_images(src, "warp.apply: src")
    dev = src.device
    if (not isinstance(mats, th.Tensor) or mats.device != dev or mats.dtype != th.int32 or mats.dim() != 2
            or mats.shape[1] != MATS_WIDTH or not mats.is_contiguous()):
        raise ValueError(f"warp.apply: mats must be a contiguous int32 [B, {MATS_WIDTH}] tensor on {dev}")
    nb = int(mats.shape[0])

    def composed():  # "warp, then view", once ops is known to be what compose_ops takes
        return [mats if ops is None else compose_ops(mats, ops, src.shape[2], src.shape[3]).contiguous(), ops]

    return _launch("warp.apply", "marl_batch_warp", src, nb, rows, [("ops", ops, OPS_WIDTH)], mode, fill, out,
                   rows_shape=str(nb), ready=composed)
