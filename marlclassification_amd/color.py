"""Colour jitter on the device: brightness, contrast, saturation, hue and random greyscale of every image of a batch
as ONE per-image colour matrix applied in one launch - ``data.ResidentLoader`` / ``data.DevicePrefetcher``
(``color=``) and the command line's ``train --color SPEC``.

Per output image ``b`` a source row ``rows[b]`` and eight int32 values ``params[b] = (beta, kappa, sigma, hcos, hsin,
0, 0, 0)``: the brightness, contrast and saturation factors in Q12 (4096 = 1.0) and the cosine and sine of the hue angle
in Q14.  Nothing in ``params`` or ``rows`` is trusted (device tensors nobody inspects): factors are clamped to
``[0, 4 * 4096]``, ``hcos`` / ``hsin`` to ``[-16384, 16384]``, rows to ``[0, n_src)``.

With ``g = (77, 150, 29) / 256`` the grey weights (one channel: ``g = (1)``), ``G = 1 g^T``, ``K`` the generator of the
YIQ chroma rotation (``T^-1 J T`` for the NTSC matrix ``T``; every row sums to exactly 0, so grey is a fixed point) and
``m[c]`` the mean of plane ``c`` - uint8: ``((256 S1[c]) // N) / 256`` from the integer records of
``transforms.stats`` (``S1`` clamped to ``[0, 255 N]``: records are device memory too); fp32: ``S1[c] / N`` in
float64 - the matrix is composed in float64 with ``+ - *`` only, every operation rounded, products of matrices accumulated left to right, in this fixed order::

    M = I, o = 0
    brightness: M = beta M;  o = beta o
    contrast:   mu = g . (M m + o);  M = kappa M;  o = kappa o + (1 - kappa) mu 1     (no records: skipped)
    saturation: S = sigma I + (1 - sigma) G;  M = S M;  o = S o                       (three channels only)
    hue:        H = (G + hcos (I - G)) + hsin K;  M = H M;  o = H o                   (three channels only)

Stated deviations from torchvision's ``ColorJitter``: the order is fixed, and nothing is clamped or rounded between the
stages.

uint8 pixels: ``A_q = clamp(rint(4096 M), +-2^19)``, ``o_q = clamp(rint(4096 o), +-2^30)`` (``o`` in grey levels),
``acc_i = sum_j A_q[i][j] x_j + o_q[i]`` in int32 and ``y_i = clamp((acc_i + 2048) >> 12, 0, 255)``.  fp32 pixels:
``M`` and ``o`` rounded once to fp32, ``y_i = ((a0 x0 (+) a1 x1) (+) a2 x2) (+) o_i`` with every product and sum rounded
separately; terms whose coefficient or offset is exactly 0 are skipped (a NaN behind a zero stays where it is, the
identity is a bit copy), no clamp.

``reference_matrix`` / ``reference_apply`` are this definition in plain torch and Python numbers, on any device;
``apply`` is the product: one launch of libmarl_hip.so (include/marl_hip_color.h), whose uint8 matrices equal
``reference_matrix`` integer for integer.
"""

from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import torch as th

from . import transforms as _transforms

PARAMS_WIDTH = 8
Q12, Q14 = 4096, 16384          # MARL_COLOR_Q12 / MARL_COLOR_Q14
MAX_FACTOR = 4 * Q12            # MARL_COLOR_MAX_FACTOR
OUT_FORMS = {"same": 0, "norm": 1}  # MARL_COLOR_OUT_*
GREY = (77, 150, 29)            # MARL_COLOR_G*, in 256ths
_K2 = ((0.168622, 0.329805), (-0.327963, 0.034611), (1.246461, -1.043229))  # MARL_COLOR_K*
K = tuple((a, b, -(a + b)) for a, b in _K2)  # the last entry of a row: minus the float64 sum of the other two
IDENTITY = (Q12, Q12, Q12, Q14, 0, 0, 0, 0)


# ---- the definition -----------------------------------------------------------------------------------------------
def _dot(x: Sequence[float], y: Sequence[float]) -> float:
    acc = x[0] * y[0]
    for j in range(1, len(x)):
        acc = acc + x[j] * y[j]
    return acc


def _left_mul(left, m, o):
    c = len(o)
    return ([[_dot(left[i], [m[k][j] for k in range(c)]) for j in range(c)] for i in range(c)],
            [_dot(left[i], o) for i in range(c)])


def _clamp(v: int, lo: int, hi: int) -> int:
    return lo if v < lo else (hi if v > hi else v)


def _compose(p: Sequence[int], mean: Optional[Sequence[float]], c: int):
    """(M, o) of one image as Python floats: the four stages of the module docstring"""
    beta = _clamp(p[0], 0, MAX_FACTOR) * (1.0 / Q12)
    kappa = _clamp(p[1], 0, MAX_FACTOR) * (1.0 / Q12)
    g = [v / 256.0 for v in GREY] if c == 3 else [1.0]
    m = [[beta if i == j else 0.0 for j in range(c)] for i in range(c)]
    o = [0.0] * c
    if mean is not None:
        v = [_dot(m[i], mean) + o[i] for i in range(c)]
        shift = (1.0 - kappa) * _dot(g, v)
        m = [[kappa * m[i][j] for j in range(c)] for i in range(c)]
        o = [kappa * o[i] + shift for i in range(c)]
    if c == 3:
        sigma = _clamp(p[2], 0, MAX_FACTOR) * (1.0 / Q12)
        hc = _clamp(p[3], -Q14, Q14) * (1.0 / Q14)
        hs = _clamp(p[4], -Q14, Q14) * (1.0 / Q14)
        rest = 1.0 - sigma
        m, o = _left_mul([[(sigma if i == j else 0.0) + rest * g[j] for j in range(3)] for i in range(3)], m, o)
        m, o = _left_mul([[(g[j] + hc * ((1.0 if i == j else 0.0) - g[j])) + hs * K[i][j] for j in range(3)]
                          for i in range(3)], m, o)
    return m, o


def _quantise(v: float, bound: int) -> int:
    return _clamp(round(4096.0 * v), -bound, bound)  # (round of a float: to nearest, ties to even - rint)


def _means(records: Optional[th.Tensor], plane: int, uint8: bool):
    if records is None:
        return None
    s1 = records[:, :, 0].cpu().tolist()
    if uint8:
        return [[((256 * _clamp(int(s), 0, 255 * plane)) // plane) * (1.0 / 256.0) for s in row] for row in s1]
    return [[float(s) / float(plane) for s in row] for row in s1]


def reference_matrix(params: th.Tensor, records: Optional[th.Tensor], shape: Sequence[int], uint8: bool) -> th.Tensor:
    """``[B, C, C + 1]`` (row ``i``: ``A[i][0..C)``, ``o[i]``) for images of ``shape = (C, H, W)``: int32 ``A_q`` /
    ``o_q`` for uint8 sources, the float32 matrix for fp32 sources.  ``records``: ``transforms.reference_stats``' or
    ``stats``' (None: no contrast).  Python ints and floats throughout."""
    c, h, w = (int(v) for v in shape)
    if c not in (1, 3):
        raise ValueError(f"color: images have 1 or 3 channels, got {c}")
    if params.dim() != 2 or params.shape[1] != PARAMS_WIDTH:
        raise ValueError(f"color: params {tuple(params.shape)} is no [B, {PARAMS_WIDTH}] table")
    rows = params.cpu().tolist()
    if records is not None and tuple(records.shape) != (len(rows), c, _transforms.RECORD_WIDTH):
        raise ValueError(f"color: records {tuple(records.shape)} do not describe {len(rows)} images of {c} channels")
    means = _means(records, h * w, uint8)
    out = th.zeros(len(rows), c, c + 1, dtype=th.int32 if uint8 else th.float64)
    for b, p in enumerate(rows):
        m, o = _compose([int(v) for v in p], None if means is None else means[b], c)
        for i in range(c):
            for j in range(c):
                out[b, i, j] = _quantise(m[i][j], 1 << 19) if uint8 else m[i][j]
            out[b, i, c] = _quantise(o[i], 1 << 30) if uint8 else o[i]
    return out if uint8 else out.to(th.float32)


def apply_matrix(x: th.Tensor, coef: th.Tensor) -> th.Tensor:
    """The pixel rule of the module docstring: ``x`` ``[B, C, H, W]`` uint8 under int32 ``coef`` or fp32 under fp32
    ``coef`` (``[B, C, C + 1]``) -> the jittered batch in ``x``'s dtype, on ``x``'s device."""
    nb, c = x.shape[:2]
    if x.dtype == th.uint8:
        k = coef.to(x.device, th.int64)
        xi = x.to(th.int64)
        acc = k[:, :, c].view(nb, c, 1, 1).expand(nb, c, *x.shape[2:]).clone()
        for j in range(c):
            acc += k[:, :, j].view(nb, c, 1, 1) * xi[:, j: j + 1]
        return ((acc + 2048) >> 12).clamp(0, 255).to(th.uint8)
    out = th.zeros_like(x)
    table = coef.cpu().tolist()
    for b in range(nb):
        for i in range(c):
            acc = None
            for j in range(c):
                if table[b][i][j] == 0.0:
                    continue
                term = x[b, j] * coef[b, i, j].to(x.device)  # (one rounded fp32 product)
                acc = term if acc is None else acc + term
            if table[b][i][c] != 0.0:
                off = coef[b, i, c].to(x.device)
                acc = off.expand_as(x[b, i]) if acc is None else acc + off
            if acc is not None:
                out[b, i] = acc
    return out


def reference_apply(src: th.Tensor, rows: Optional[th.Tensor], params: th.Tensor, records: Optional[th.Tensor] = None,
                    normalize=None) -> th.Tensor:
    """The definition in plain torch, on any device: ``src`` ``[N, C, H, W]`` uint8 or fp32, ``rows`` ``[B]`` integers
    (None: every image; clamped), ``params`` ``[B, 8]`` integers, ``records`` those of ``src[rows]`` (None: no
    contrast) -> ``[B, C, H, W]`` in ``src``'s dtype.  ``normalize`` (a user ``transforms.Spec``, uint8 sources): the
    fp32 batch ``transforms.reference_apply`` makes of the jittered one."""
    _transforms._check_images(src, "color.reference_apply")
    x = _transforms._selected(src, rows)
    out = apply_matrix(x, reference_matrix(params, records, x.shape[1:], src.dtype == th.uint8))
    if normalize is None:
        return out
    return _transforms.reference_apply(out, None, _user_spec(normalize, src))


def _user_spec(normalize, src: th.Tensor):
    spec = _transforms.resolve(normalize)
    if spec is None or not spec.is_user:
        raise ValueError("color: the fused output form takes a user-normal / user-minmax transform; statistic modes are "
                         "two steps (their statistics are those of the jittered image)")
    if src.dtype != th.uint8:
        raise ValueError("color: the fused output form takes uint8 sources only")
    return spec


# ---- the policy and its command-line spelling ---------------------------------------------------------------------
@dataclass(frozen=True)
class Policy:
    """What ``parse`` returns: the half-widths of the three factor ranges (0: off), the hue range in turns and the
    probability of a grey image."""

    brightness: float = 0.0
    contrast: float = 0.0
    saturation: float = 0.0
    hue: float = 0.0
    gray: float = 0.0
    spec: str = ""

    def __post_init__(self) -> None:
        for name in ("brightness", "contrast", "saturation"):
            v = getattr(self, name)
            if not (isinstance(v, (int, float)) and 0.0 <= v <= 3.0):
                raise ValueError(f"color: {name} must lie in [0, 3], got {v!r}")
        if not (isinstance(self.hue, (int, float)) and 0.0 <= self.hue <= 0.5):
            raise ValueError(f"color: hue must lie in [0, 0.5] turns, got {self.hue!r}")
        if not (isinstance(self.gray, (int, float)) and 0.0 <= self.gray <= 1.0):
            raise ValueError(f"color: gray must lie in [0, 1], got {self.gray!r}")

    @property
    def needs_stats(self) -> bool:
        """contrast pivots on the image's grey mean: the records of ``transforms.stats``"""
        return self.contrast > 0.0

    def draw(self, batch: int, generator: th.Generator) -> th.Tensor:
        """``params`` ``[batch, 8]`` int32 on the generator's device, from one ``[batch, 5]`` uniform draw of the
        generator, torch ops only (no host synchronisation): each factor uniform in ``[max(0, 1 - v), 1 + v]``, the hue
        angle uniform in ``[-hue, hue]`` turns, ``sigma = 0`` with probability ``gray``.  A stage that is off gets its
        identity."""
        dev = generator.device
        u = th.rand(batch, 5, generator=generator, device=dev)
        params = th.zeros(batch, PARAMS_WIDTH, dtype=th.int32, device=dev)
        for col, v in enumerate((self.brightness, self.contrast, self.saturation)):
            lo, hi = max(0.0, 1.0 - v), 1.0 + v
            params[:, col] = th.round((lo + (hi - lo) * u[:, col]) * Q12).to(th.int32).clamp(0, MAX_FACTOR)
        angle = (2.0 * math.pi * self.hue) * (2.0 * u[:, 3] - 1.0)
        params[:, 3] = th.round(th.cos(angle) * Q14).to(th.int32).clamp(-Q14, Q14)
        params[:, 4] = th.round(th.sin(angle) * Q14).to(th.int32).clamp(-Q14, Q14)
        params[:, 2] = th.where(u[:, 4] < self.gray, th.zeros_like(params[:, 2]), params[:, 2])
        return params


_TOKENS = {"brightness": 3.0, "contrast": 3.0, "saturation": 3.0, "hue": 0.5, "gray": 1.0}


def parse(spec) -> Policy:
    """``brightness:B``, ``contrast:C``, ``saturation:S`` (``0 < v <= 3``), ``hue:H`` (``0 < H <= 0.5`` turns) and
    ``gray:p`` (``0 < p <= 1``), comma-separated, each at most once.  Anything else: ValueError naming the token."""
    if isinstance(spec, Policy):
        return spec
    if not isinstance(spec, str):
        raise ValueError(f"color: the spec must be a string, got {spec!r}")
    kw = {}
    for token in (t.strip() for t in spec.split(",")):
        head, *rest = token.split(":")
        if head not in _TOKENS or len(rest) != 1:
            raise ValueError(f'color: unknown token "{token}" (brightness:B, contrast:C, saturation:S, hue:H, gray:p)')
        if head in kw:
            raise ValueError(f'color: "{head}" is given twice in "{spec}"')
        try:
            v = float(rest[0])
        except ValueError:
            v = float("nan")
        if not (math.isfinite(v) and 0.0 < v <= _TOKENS[head]):
            raise ValueError(f'color: bad token "{token}" (a number in (0, {_TOKENS[head]:g}] is expected)')
        kw[head] = v
    return Policy(spec=spec, **kw)


# ---- the product: one launch of libmarl_hip.so ----------------------------------------------------------------------
class ColorPlan(C.Structure):
    """Mirror of ``marl_color_plan_info`` (include/marl_hip_color.h)."""

    _fields_ = ([(name, C.c_int32) for name in "load_bytes store_bytes pixels_per_vector vectors_per_thread "
                                               "blocks_per_image lds_bytes".split()] + [("reserved", C.c_int32 * 2)])

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


def plan(src: th.Tensor, out: Optional[th.Tensor] = None, out_form: str = "same") -> dict:
    """What ``apply`` launches for images like ``src`` (``marl_batch_color_plan``): load and store bytes per thread and
    plane, pixels per vector, vectors per thread, workgroups per image.  ``src`` may live anywhere (only its shape, element size and - on a
    GPU - address are read)."""
    from . import _lib

    info = ColorPlan()
    _, c, h, w = src.shape
    _lib.check(_lib.load().marl_batch_color_plan(c, h, w, src.element_size(), _out_form(out_form),
                                                 src.data_ptr() if src.is_cuda else None,
                                                 None if out is None else out.data_ptr(), C.byref(info)))
    return info.as_dict()


def _out_form(out_form: str) -> int:
    if out_form not in OUT_FORMS:
        raise ValueError(f'color: unknown output form "{out_form}" (same or norm)')
    return OUT_FORMS[out_form]


def apply(src: th.Tensor, rows: Optional[th.Tensor], params: th.Tensor, records: Optional[th.Tensor] = None,
          out_form: str = "same", normalize=None, return_coef: bool = False, out: Optional[th.Tensor] = None):
    """``reference_apply`` on GPU tensors, one launch on the current stream: ``src`` contiguous ``[N, C, H, W]`` uint8
    or float32 with 1 or 3 channels, ``rows`` int64 ``[B]`` (None: every image), ``params`` int32 ``[B, 8]``,
    ``records`` those of ``transforms.stats(src, rows)`` (None: no contrast).  ``out_form="norm"`` with ``normalize`` a
    user ``transforms.Spec`` (uint8 sources): the normalised fp32 batch in the same launch.  ``return_coef``: also the
    ``[B, C, C + 1]`` matrix the kernel derived (int32 for uint8 sources, fp32 for fp32).  ``out`` (None: a fresh
    tensor) must not overlap ``src``."""
    from . import _lib

    form = _out_form(out_form)
    nb = _transforms._need_source(src, rows, "color.apply")
    _, c, h, w = src.shape
    dev = src.device
    if params.device != dev or params.dtype != th.int32 or tuple(params.shape) != (nb, PARAMS_WIDTH) \
            or not params.is_contiguous():
        raise ValueError(f"color.apply: params must be a contiguous int32 [{nb}, {PARAMS_WIDTH}] tensor on {dev}")
    rec_dtype = th.int64 if src.dtype == th.uint8 else th.float64
    if records is not None and (records.device != dev or records.dtype != rec_dtype or not records.is_contiguous()
                                or tuple(records.shape) != (nb, c, _transforms.RECORD_WIDTH)):
        raise ValueError(f"color.apply: records must be a contiguous {rec_dtype} [{nb}, {c}, "
                         f"{_transforms.RECORD_WIDTH}] tensor on {dev}")
    user, mode = None, 0
    if form == OUT_FORMS["norm"]:
        spec = _user_spec(normalize, src)
        user = _transforms._user_array(spec, c)
        mode = _transforms.MODES[spec.mode]
    elif normalize is not None:
        raise ValueError('color.apply: normalize goes with out_form="norm"')
    out = _transforms._need_out(out, "color.apply", (nb, c, h, w), th.float32 if form else src.dtype, dev)
    coef = None
    if return_coef:
        coef = th.empty(nb, c, c + 1, dtype=th.int32 if src.dtype == th.uint8 else th.float32, device=dev)
    if nb > 0:
        with th.cuda.device(dev):
            _lib.check(_lib.load().marl_batch_color(
                src.data_ptr(), src.shape[0], None if rows is None else rows.data_ptr(),
                None if records is None else records.data_ptr(), params.data_ptr(), form, mode, user, nb, c, h, w,
                src.element_size(), out.data_ptr(), None if coef is None else coef.data_ptr(),
                th.cuda.current_stream(dev).cuda_stream))
    return (out, coef) if return_coef else out
