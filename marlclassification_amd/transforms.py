"""Per-image input normalisation: the reference's six input transforms (``data/transforms.py``: ``UserNormalNorm``,
``ChannelNormalNorm``, ``NormalNorm``, ``UserMinMaxNorm``, ``MinMaxNorm``, ``ChannelMinMaxNorm``) as a choice of the
model - ``train --normalize SPEC``, kept in ``marl.json`` and read back by ``test`` and ``infer`` - that runs on images
which already live in HBM (``data.ResidentLoader`` / ``data.DevicePrefetcher(..., normalize=)``).

Definition.  With ``x`` the pixel as stored (uint8 0..255, or fp32), ``N`` the number of pixels a statistic covers,
``S1 = sum x``, ``S2 = sum x^2``, ``mean = S1 / N`` and ``std = sqrt((N S2 - S1^2) / (N (N - 1)))`` (unbiased, as
``torch.std``)::

    mode                                 statistic over          scale64                 offset64
    normal          (NormalNorm)         the image, N = C H W    1 / std                 -mean / std
    channel-normal  (ChannelNormalNorm)  a plane, N = H W        the same, per channel
    minmax          (MinMaxNorm)         the image               1 / (max - min)         -min / (max - min)
    channel-minmax  (ChannelMinMaxNorm)  a plane                 the same, per channel
    user-normal:m..:s..  (UserNormalNorm)    none                1 / (255 s)             -m / s
    user-minmax:lo..:hi..  (UserMinMaxNorm)  none                1 / (255 (hi - lo))     -lo / (hi - lo)

for uint8 sources: ``ToTensor``'s ``/ 255`` is folded in (it cancels in every statistic mode; the user values are in
``ToTensor`` units).  fp32 sources drop the 255.  Both coefficients are float64 expressions rounded once to fp32 and
``out = fadd(fmul(float(x), scale), offset)``, the product and the sum rounded separately.  For uint8 the sums are
integers and ``N S2 - S1^2`` is exact; whole-image modes add the channels' records first.  A constant image or plane
(``std == 0``, ``max == min``, ``N == 1``) has ``scale = offset = 0``: it becomes zeros, where the reference yields NaN /
inf - a stated deviation, so that a blank tile does not poison a run.  Non-finite fp32 pixels are outside the definition.

``reference_stats`` / ``reference_coef`` / ``reference_apply`` are this definition in plain torch and Python numbers,
on any device; ``stats`` / ``apply`` are the product: three launches of libmarl_hip.so (include/marl_hip_normalize.h).
"""

from __future__ import annotations

import ctypes as C
import math
from abc import ABCMeta, abstractmethod
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import torch as th

MODES = {"normal": 0, "channel-normal": 1, "minmax": 2, "channel-minmax": 3, "user-normal": 4, "user-minmax": 5}
MAX_USER_CHANNELS = 16  # MARL_NORM_MAX_USER_CHANNELS
RECORD_WIDTH = 4  # (S1, S2, min, max)


# ---- the choice and its command-line spelling ---------------------------------------------------------------------
@dataclass(frozen=True)
class Spec:
    """What ``parse`` returns: the mode and, for the user modes, the two value lists (``first`` = means or lows,
    ``second`` = stds or highs, one per channel).  ``dataset`` is a request, not a transform: ``dataset_spec`` resolves
    it to a ``user-normal`` Spec."""

    mode: str
    first: Tuple[float, ...] = ()
    second: Tuple[float, ...] = ()

    @property
    def is_user(self) -> bool:
        return self.mode in ("user-normal", "user-minmax")

    @property
    def whole_image(self) -> bool:
        return self.mode in ("normal", "minmax")

    @property
    def spelling(self) -> str:
        """The string ``parse`` reads back into an equal Spec (``repr`` of a float round-trips)."""
        if not self.is_user:
            return self.mode
        return ":".join([self.mode, ",".join(repr(v) for v in self.first), ",".join(repr(v) for v in self.second)])

    def user(self, channels: int):
        """``[(m, s)]`` or ``[(lo, hi)]`` per channel of a user mode, checked against the image's channel count"""
        if len(self.first) != channels:
            raise ValueError(f'normalize "{self.spelling}": {len(self.first)} values per list for {channels} channels')
        if channels > MAX_USER_CHANNELS:
            raise ValueError(f"normalize: user modes take at most {MAX_USER_CHANNELS} channels, got {channels}")
        return list(zip(self.first, self.second))


def _values(text: str, spec: str) -> Tuple[float, ...]:
    try:
        values = tuple(float(t) for t in text.split(","))
    except ValueError:
        values = ()
    if not values or not all(math.isfinite(v) for v in values):
        raise ValueError(f'normalize: bad value list "{text}" in "{spec}" (finite numbers, comma-separated)')
    return values


def parse(spec) -> Spec:
    """``normal | channel-normal | minmax | channel-minmax | user-normal:m0,m1,..:s0,s1,.. | user-minmax:lo..:hi.. |
    dataset``.  Anything else: ValueError."""
    if isinstance(spec, Spec):
        return spec
    if not isinstance(spec, str):
        raise ValueError(f"normalize: the spec must be a string, got {spec!r}")
    head, *rest = spec.strip().split(":")
    if head == "dataset" and not rest:
        return Spec("dataset")
    if head in MODES and head not in ("user-normal", "user-minmax"):
        if rest:
            raise ValueError(f'normalize: "{head}" takes no values, got "{spec}"')
        return Spec(head)
    if head in ("user-normal", "user-minmax") and len(rest) == 2:
        first, second = _values(rest[0], spec), _values(rest[1], spec)
        if len(first) != len(second):
            raise ValueError(f'normalize: the two lists of "{spec}" differ in length')
        if len(first) > MAX_USER_CHANNELS:
            raise ValueError(f'normalize: "{spec}" names more than {MAX_USER_CHANNELS} channels')
        for a, b in zip(first, second):
            width = b if head == "user-normal" else b - a
            if width == 0 or not math.isfinite(width):
                raise ValueError(f'normalize: "{spec}" divides by zero (a std of 0, or hi == lo)')
        return Spec(head, first, second)
    raise ValueError(f'normalize: unknown spec "{spec}" (normal, channel-normal, minmax, channel-minmax, '
                     "user-normal:m0,m1,..:s0,s1,.., user-minmax:lo0,..:hi0,.., dataset)")


def resolve(spec) -> Optional[Spec]:
    """``None`` / ``"none"`` -> None, else ``parse``; a loader or model cannot run ``dataset`` itself."""
    if spec is None or spec == "none":
        return None
    s = parse(spec)
    if s.mode == "dataset":
        raise ValueError('normalize: "dataset" must be resolved against the training split first '
                         "(transforms.dataset_spec)")
    return s


# ---- the definition -----------------------------------------------------------------------------------------------
def _check_images(src: th.Tensor, who: str) -> None:
    if src.dtype not in (th.uint8, th.float32):
        raise TypeError(f"{who}: src must be uint8 or float32, got {src.dtype}")
    if src.dim() != 4:
        raise ValueError(f"{who}: src must be [N, C, H, W], got {tuple(src.shape)}")


def _selected(src: th.Tensor, rows: Optional[th.Tensor]) -> th.Tensor:
    if rows is None:
        return src
    return src.index_select(0, rows.to(src.device, th.int64).clamp(0, src.shape[0] - 1))


def reference_stats(src: th.Tensor, rows: Optional[th.Tensor] = None) -> th.Tensor:
    """``[B, C, 4]`` records ``(S1, S2, min, max)`` of ``src[rows]`` (``rows`` None: every image; rows are clamped):
    int64 for uint8 sources - exact integers - and float64 for fp32 sources (sums in float64, min / max exact)."""
    _check_images(src, "transforms.reference_stats")
    x = _selected(src, rows)
    nb, c = x.shape[0], x.shape[1]
    x = x.reshape(nb, c, -1).to(th.int64 if src.dtype == th.uint8 else th.float64)
    return th.stack([x.sum(-1), (x * x).sum(-1), x.min(-1).values, x.max(-1).values], dim=-1)


def _coef_of(mode: str, uint8: bool, n: int, s1, s2, lo, hi) -> Tuple[float, float]:
    """(scale64, offset64) of one statistic, in the order of operations of the module docstring"""
    if mode in ("normal", "channel-normal"):
        num = float(n * s2 - s1 * s1) if uint8 else float(n) * s2 - s1 * s1  # (Python ints: exact, converted once)
        if n < 2 or not num > 0.0:
            return 0.0, 0.0
        std = math.sqrt(num / float(n * (n - 1)))
        mean = float(s1) / float(n)
        return 1.0 / std, -mean / std
    d = float(hi) - float(lo)
    if not d > 0.0:
        return 0.0, 0.0
    return 1.0 / d, -float(lo) / d


def reference_coef(records: th.Tensor, spec, shape: Sequence[int], uint8: bool) -> th.Tensor:
    """``[B, C, 2]`` float64 ``(scale64, offset64)`` from ``records`` (``reference_stats``' or ``stats``'; ignored by
    the user modes, where ``records`` may be an int: the batch size) for images of ``shape = (C, H, W)``.  Python ints
    and floats throughout; ``.float()`` of the result is the pair the kernel multiplies by."""
    spec = parse(spec)
    c, h, w = (int(v) for v in shape)
    nb = int(records) if isinstance(records, int) else int(records.shape[0])
    out = th.zeros(nb, c, 2, dtype=th.float64)
    if spec.is_user:
        k = 255.0 if uint8 else 1.0
        for ch, (a, b) in enumerate(spec.user(c)):
            if spec.mode == "user-normal":
                pair = (1.0 / (k * b), -a / b)
            else:
                pair = (1.0 / (k * (b - a)), -a / (b - a))
            out[:, ch, 0], out[:, ch, 1] = pair
        return out
    if spec.mode not in MODES:
        raise ValueError(f'normalize: "{spec.mode}" names no transform')
    rec = records.cpu().tolist()
    for b in range(nb):
        if spec.whole_image:
            s1, s2 = sum(r[0] for r in rec[b]), sum(r[1] for r in rec[b])  # (ascending channels)
            lo, hi = min(r[2] for r in rec[b]), max(r[3] for r in rec[b])
            pair = _coef_of(spec.mode, uint8, c * h * w, s1, s2, lo, hi)
            for ch in range(c):
                out[b, ch, 0], out[b, ch, 1] = pair
        else:
            for ch in range(c):
                out[b, ch, 0], out[b, ch, 1] = _coef_of(spec.mode, uint8, h * w, *rec[b][ch])
    return out


def reference_apply(src: th.Tensor, rows: Optional[th.Tensor], spec) -> th.Tensor:
    """The definition in plain torch, on any device: ``src`` ``[N, C, H, W]`` uint8 or fp32, ``rows`` ``[B]`` integers
    (None: every image) -> fp32 ``[B, C, H, W]``.  The fp32 multiply and add are two separate torch ops."""
    spec = parse(spec)
    _check_images(src, "transforms.reference_apply")
    x = _selected(src, rows)
    records = x.shape[0] if spec.is_user else reference_stats(x)
    coef = reference_coef(records, spec, x.shape[1:], src.dtype == th.uint8).to(th.float32).to(x.device)
    scale, offset = coef[:, :, 0, None, None], coef[:, :, 1, None, None]
    prod = x.to(th.float32) * scale
    return prod + offset


def dataset_spec(resident_x: th.Tensor, chunk: int = 256) -> Spec:
    """The usual dataset mean / std as a ``user-normal`` Spec: the integer records of the whole set (``[N, C, H, W]``
    uint8 or fp32; on a GPU through ``stats``, ``chunk`` images at a time) summed per channel, then mean and unbiased
    std over all ``N H W`` pixels of a channel, in ``ToTensor`` units for uint8.  The Spec needs no data at test time."""
    _check_images(resident_x, "transforms.dataset_spec")
    return dataset_spec_of(resident_x[at: at + chunk] for at in range(0, resident_x.shape[0], chunk))


def dataset_spec_of(batches) -> Spec:
    """``dataset_spec`` of the concatenation of ``batches`` (an iterable of ``[n, C, H, W]`` tensors of one dtype and
    shape, on one device), for sets that are not resident."""
    total, n = None, 0
    for part in batches:
        _check_images(part, "transforms.dataset_spec")
        part = part.contiguous()
        rec = stats(part) if part.is_cuda else reference_stats(part)
        total = rec[:, :, :2].sum(0) if total is None else total + rec[:, :, :2].sum(0)
        n += part.shape[0]
        (c, h, w), uint8 = part.shape[1:], part.dtype == th.uint8
    if total is None:
        raise ValueError("normalize: the set is empty")
    means, stds = [], []
    pixels = n * h * w
    k = 255.0 if uint8 else 1.0
    for s1, s2 in total.cpu().tolist():
        num = float(pixels * s2 - s1 * s1) if uint8 else float(pixels) * s2 - s1 * s1
        if pixels < 2 or not num > 0.0:
            raise ValueError("normalize: a channel of the set is constant: its dataset std is 0")
        means.append(float(s1) / float(pixels) / k)
        stds.append(math.sqrt(num / float(pixels * (pixels - 1))) / k)
    return Spec("user-normal", tuple(means), tuple(stds))


# ---- the reference's classes ----------------------------------------------------------------------------------------
class ImgTransform(metaclass=ABCMeta):
    """A transform of one image ``[C, H, W]`` fp32 (CPU or GPU), as in the reference."""

    @abstractmethod
    def __call__(self, img_data: th.Tensor) -> th.Tensor:
        raise NotImplementedError(self.__class__.__name__ + ".__call__ method is not implemented, must be overridden !")

    def __repr__(self) -> str:
        return self.__class__.__name__ + "()"


class _SpecTransform(ImgTransform):
    """``reference_apply`` of one fp32 image under a fixed Spec, any number of channels"""

    spec: Spec

    def __call__(self, x: th.Tensor) -> th.Tensor:
        if x.dim() != 3:
            raise ValueError(f"{self.__class__.__name__}: an image [C, H, W] is expected, got {tuple(x.shape)}")
        return reference_apply(x.to(th.float32).unsqueeze(0), None, self.spec)[0]


class UserNormalNorm(_SpecTransform):
    def __init__(self, mean: Sequence[float], std: Sequence[float]) -> None:
        super().__init__()
        self.spec = parse(Spec("user-normal", tuple(float(v) for v in mean), tuple(float(v) for v in std)).spelling)

    def __repr__(self) -> str:
        return self.__class__.__name__ + f"(mean = {list(self.spec.first)}, std = {list(self.spec.second)})"


class ChannelNormalNorm(_SpecTransform):
    spec = Spec("channel-normal")


class NormalNorm(_SpecTransform):
    spec = Spec("normal")


class UserMinMaxNorm(_SpecTransform):
    def __init__(self, min_value: Sequence[float], max_value: Sequence[float]) -> None:
        super().__init__()
        self.spec = parse(Spec("user-minmax", tuple(float(v) for v in min_value),
                               tuple(float(v) for v in max_value)).spelling)

    def __repr__(self) -> str:
        return (self.__class__.__name__ +
                f"(min_value = {list(self.spec.first)}, max_value = {list(self.spec.second)})")


class MinMaxNorm(_SpecTransform):
    spec = Spec("minmax")


class ChannelMinMaxNorm(_SpecTransform):
    spec = Spec("channel-minmax")


# ---- the product: three launches of libmarl_hip.so ------------------------------------------------------------------
class NormalizePlan(C.Structure):
    """Mirror of ``marl_normalize_plan_info`` (include/marl_hip_normalize.h)."""

    _fields_ = [(name, C.c_int32) for name in ("chunk_elems partials_per_plane load_bytes lds_bytes store_bytes "
                                               "apply_chunk_elems apply_blocks_per_plane reserved").split()]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


def _need_source(src: th.Tensor, rows: Optional[th.Tensor], who: str) -> int:
    from .augment import _need_images

    _need_images(src, f"{who}: src")
    nb = int(src.shape[0]) if rows is None else int(rows.shape[0])
    if rows is not None and (rows.device != src.device or rows.dtype != th.int64 or rows.dim() != 1
                             or not rows.is_contiguous()):
        raise ValueError(f"{who}: rows must be a contiguous int64 [B] tensor on {src.device}")
    return nb


def _need_out(out: Optional[th.Tensor], who: str, shape, dtype, dev, called: Optional[str] = None) -> th.Tensor:
    """the tensor a launch writes: a fresh one, or the caller's ``out`` if it is what a fresh one would be (``called``:
    how the message names the dtype, ``dtype`` itself if None)"""
    if out is None:
        return th.empty(shape, dtype=dtype, device=dev)
    if out.device != dev or out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous {called or dtype} {shape} tensor on {dev}")
    return out


def _user_array(spec: Spec, c: int):
    """the pairs of a user Spec, checked against ``c`` channels, as the ``double[2 c]`` the C entries take"""
    return (C.c_double * (2 * c))(*[v for pair in spec.user(c) for v in pair])


def plan(src: th.Tensor, out: Optional[th.Tensor] = None) -> dict:
    """What ``stats`` / ``apply`` launch for images like ``src`` (``marl_batch_normalize_plan``): the chunk a workgroup
    reduces, the partial records per plane, load and store widths, LDS bytes.  ``src`` may live anywhere (only its shape,
    element size and - on a GPU - address are read)."""
    from . import _lib

    info = NormalizePlan()
    _, c, h, w = src.shape
    _lib.check(_lib.load().marl_batch_normalize_plan(c, h, w, src.element_size(), src.data_ptr() if src.is_cuda else None,
                                                     None if out is None else out.data_ptr(), C.byref(info)))
    return info.as_dict()


def stats(src: th.Tensor, rows: Optional[th.Tensor] = None) -> th.Tensor:
    """``reference_stats`` on GPU tensors, two launches on the current stream: ``[B, C, 4]`` int64 (uint8 ``src``) or
    float64 (fp32 ``src``).  uint8 images of more than 2^23 pixels are refused (``marl_batch_stats``)."""
    from . import _lib

    nb = _need_source(src, rows, "transforms.stats")
    _, c, h, w = src.shape
    dev = src.device
    records = th.empty(nb, c, RECORD_WIDTH, dtype=th.int64 if src.dtype == th.uint8 else th.float64, device=dev)
    if nb == 0:
        return records
    lib = _lib.load()
    need = lib.marl_batch_stats_scratch_bytes(nb, c, h, w, src.element_size())
    scratch = th.empty(max(need, 8) // 8, dtype=th.int64, device=dev)  # (the partial records between the launches)
    with th.cuda.device(dev):
        _lib.check(lib.marl_batch_stats(src.data_ptr(), src.shape[0], None if rows is None else rows.data_ptr(), nb, c,
                                        h, w, src.element_size(), scratch.data_ptr(), records.data_ptr(),
                                        th.cuda.current_stream(dev).cuda_stream))
    return records


def apply(src: th.Tensor, rows: Optional[th.Tensor], spec, return_coef: bool = False,
          out: Optional[th.Tensor] = None, records: Optional[th.Tensor] = None):
    """``reference_apply`` on GPU tensors, on the current stream: the two launches of ``stats`` (statistic modes;
    ``records`` given: skipped) and one that writes the fp32 batch.  ``return_coef``: also the fp32 ``[B, C, 2]`` pairs
    the kernel derived.  ``out`` (None: a fresh tensor) must not overlap ``src``."""
    from . import _lib

    spec = resolve(spec)
    if spec is None:
        raise ValueError("transforms.apply: no transform given")
    nb = _need_source(src, rows, "transforms.apply")
    _, c, h, w = src.shape
    dev = src.device
    out = _need_out(out, "transforms.apply", (nb, c, h, w), th.float32, dev, called="float32")
    coef = th.empty(nb, c, 2, dtype=th.float32, device=dev) if return_coef else None
    if nb > 0:
        user = None
        if spec.is_user:
            user = _user_array(spec, c)
            records = None
        elif records is None:
            records = stats(src, rows)
        with th.cuda.device(dev):
            _lib.check(_lib.load().marl_batch_normalize(
                src.data_ptr(), src.shape[0], None if rows is None else rows.data_ptr(),
                None if records is None else records.data_ptr(), MODES[spec.mode], user, nb, c, h, w,
                src.element_size(), out.data_ptr(), None if coef is None else coef.data_ptr(),
                th.cuda.current_stream(dev).cuda_stream))
    return (out, coef) if return_coef else out
