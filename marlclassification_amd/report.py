"""Episode report: what ALL of an episode's ``step_preds [Ns,Na,Nb,nC]`` say about the classifier, reduced on the
device by ``marl_episode_report`` (include/marl_hip_report.h has the definition; csrc/report.hip the two kernels):
vote accuracy, top-k, NLL and agreement per step, every agent's own accuracy, the confusion matrix and the calibration
of the last step's vote, and the steps an episode needs when it stops once the vote is confident enough.

``EpisodeReport.add`` is one library call and never synchronises; reading (``result()``, ``conf_mat()`` ...) is the
only place that does.  ``reference_counts`` is the same definition in float64 torch, on any device, in the library's
layout - for tests and as documentation, like ``augment.reference_apply``.
"""

from __future__ import annotations

import ctypes as C
import json
import math
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch as th

MAX_STEPS, MAX_AGENTS, MAX_CLASSES, MAX_TOPK, MAX_BINS, MAX_EXITS = 1024, 64, 1024, 16, 64, 8

# the fields of the report buffer in the library's order (enum in include/marl_hip_report.h): the integer fields, then
# the two fp64 ones
INT_FIELDS = ("n", "skipped", "vote_hit", "rank_hist", "agent_hit", "agree", "confusion", "cal_count", "cal_hit",
              "exit_hist", "exit_hit")
F64_FIELDS = ("nll_sum", "cal_conf")


def _f32(x: float) -> float:
    return struct.unpack("f", struct.pack("f", x))[0]


@dataclass(frozen=True)
class ReportOptions:
    """``topk``: ranks reported (1 .. 16).  ``bins``: equal-width confidence bins of the calibration (1 .. 64).
    ``exit_thresholds``: up to 8 confidences in [0, 1]; an episode "exits" at the first step whose vote is at least
    that confident.  The thresholds are kept as the fp32 values the kernel compares with."""

    topk: int = 5
    bins: int = 15
    exit_thresholds: Tuple[float, ...] = ()

    def __post_init__(self) -> None:
        for name, hi in (("topk", MAX_TOPK), ("bins", MAX_BINS)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
                raise ValueError(f"{name} must be an integer in [1, {hi}], got {v!r}")
        try:
            taus = tuple(float(t) for t in self.exit_thresholds)
        except TypeError:
            raise ValueError(f"exit_thresholds must be a sequence of numbers, got {self.exit_thresholds!r}") from None
        if len(taus) > MAX_EXITS:
            raise ValueError(f"at most {MAX_EXITS} exit thresholds, got {len(taus)}")
        for t in taus:
            if not (math.isfinite(t) and 0.0 <= t <= 1.0):
                raise ValueError(f"exit thresholds must lie in [0, 1], got {t}")
        object.__setattr__(self, "exit_thresholds", tuple(_f32(t) for t in taus))


def check_sizes(ns: int, na: int, nc: int) -> None:
    for name, v, hi in (("nb_step", ns, MAX_STEPS), ("nb_agent", na, MAX_AGENTS), ("nb_class", nc, MAX_CLASSES)):
        if not 1 <= v <= hi:
            raise ValueError(f"{name} must lie in [1, {hi}], got {v}")


def layout(ns: int, na: int, nc: int, options: ReportOptions) -> Dict[str, object]:
    """Field -> (offset in 8-byte words, shape), the library's ``marl_report_layout``; ``int_words`` and ``words``."""
    check_sizes(ns, na, nc)
    k, nbin, ne = options.topk, options.bins, len(options.exit_thresholds)
    shapes = {"n": (1,), "skipped": (1,), "vote_hit": (ns,), "rank_hist": (ns, k + 1), "agent_hit": (ns, na),
              "agree": (ns,), "confusion": (nc, nc), "cal_count": (nbin,), "cal_hit": (nbin,),
              "exit_hist": (ne, ns), "exit_hit": (ne,), "nll_sum": (ns,), "cal_conf": (nbin,)}
    out: Dict[str, object] = {}
    at = 0
    for name in INT_FIELDS + F64_FIELDS:
        if name == F64_FIELDS[0]:
            out["int_words"] = at
        out[name] = (at, shapes[name])
        at += math.prod(shapes[name])
    out["words"] = at
    return out


def split_fields(int_buf: th.Tensor, f64_buf: th.Tensor, lay: Dict[str, object]) -> Dict[str, th.Tensor]:
    """Views of the two buffers by field name."""
    iw = lay["int_words"]
    out = {}
    for name in INT_FIELDS:
        off, shape = lay[name]
        out[name] = int_buf[off: off + math.prod(shape)].view(shape)
    for name in F64_FIELDS:
        off, shape = lay[name]
        out[name] = f64_buf[off - iw: off - iw + math.prod(shape)].view(shape)
    return out


def _lowest_argmax(x: th.Tensor) -> th.Tensor:
    """Lowest index of the maximum over the last axis (``argmax`` does not promise which of several it returns)."""
    n = x.shape[-1]
    idx = th.arange(n, device=x.device)
    return th.where(x == x.max(dim=-1, keepdim=True).values, idx, n).min(dim=-1).values


def reference_counts(step_preds: th.Tensor, y: th.Tensor, options: ReportOptions) -> Tuple[th.Tensor, th.Tensor]:
    """The definition of include/marl_hip_report.h in float64, on ``step_preds``' device: (int64 buffer, float64
    buffer) in the library's layout (``layout`` / ``split_fields``)."""
    if step_preds.dim() != 4:
        raise ValueError(f"step_preds must be [Ns, Na, Nb, nC], got {tuple(step_preds.shape)}")
    ns, na, nb, nc = step_preds.shape
    lay = layout(ns, na, nc, options)
    dev = step_preds.device
    y = y.to(dev).long()
    if tuple(y.shape) != (nb,):
        raise ValueError(f"y must be [{nb}], got {tuple(y.shape)}")
    ibuf = th.zeros(lay["int_words"], dtype=th.int64, device=dev)
    fbuf = th.zeros(lay["words"] - lay["int_words"], dtype=th.float64, device=dev)
    f = split_fields(ibuf, fbuf, lay)
    p = step_preds.double()
    valid = th.isfinite(p).all(dim=3).all(dim=1).all(dim=0) & (y >= 0) & (y < nc)
    f["skipped"][0] = int((~valid).sum())
    f["n"][0] = nv = int(valid.sum())
    if nv == 0:
        return ibuf, fbuf
    p, y = p[:, :, valid], y[valid]
    z = th.zeros(ns, nv, nc, dtype=th.float64, device=dev)
    for a in range(na):  # (ascending a)
        z = z + p[:, a]
    z = z / na
    cls = th.arange(nc, device=dev)
    pred = _lowest_argmax(z)                                    # [Ns, Nv]
    zy = z.gather(2, y.view(1, nv, 1).expand(ns, nv, 1))        # [Ns, Nv, 1]
    rank = (z > zy).sum(dim=2) + ((z == zy) & (cls < y.view(1, nv, 1))).sum(dim=2)
    mx = z.max(dim=2, keepdim=True).values
    se = th.exp(z - mx).sum(dim=2)
    nll = -(zy[..., 0] - mx[..., 0] - th.log(se))
    conf = 1.0 / se
    hit = pred == y
    pa = _lowest_argmax(p)                                      # [Ns, Na, Nv]
    f["vote_hit"].copy_(hit.sum(dim=1))
    r = rank.clamp(max=options.topk)
    for j in range(options.topk + 1):
        f["rank_hist"][:, j] = (r == j).sum(dim=1)
    f["agent_hit"].copy_((pa == y).sum(dim=2))
    f["agree"].copy_((pa == pred[:, None, :]).sum(dim=(1, 2)))
    f["nll_sum"].copy_(nll.sum(dim=1))
    ones = th.ones(nv, dtype=th.int64, device=dev)
    f["confusion"].view(-1).scatter_add_(0, y * nc + pred[-1], ones)
    bins = (conf[-1] * options.bins).long().clamp(max=options.bins - 1)
    f["cal_count"].scatter_add_(0, bins, ones)
    f["cal_hit"].scatter_add_(0, bins, hit[-1].long())
    f["cal_conf"].scatter_add_(0, bins, conf[-1])
    steps = th.arange(ns, device=dev).view(ns, 1)
    for j, tau in enumerate(options.exit_thresholds):
        e = th.where(conf >= tau, steps, ns - 1).min(dim=0).values
        f["exit_hist"][j].scatter_add_(0, e, ones)
        f["exit_hit"][j] = hit.gather(0, e.view(1, nv)).sum()
    return ibuf, fbuf


class EpisodeReport:
    """Accumulates episode reports on ``device``.

    ``add(step_preds, y)`` is one ``marl_episode_report`` call (two launches on the current stream, no
    synchronisation).  With ``window_size`` it writes a ring of report buffers with ``accumulate=0`` - the report is
    the sum of the last ``window_size`` batches, as the windowed ``ConfusionMeter`` - else one buffer with
    ``accumulate=1``.  ``merge`` adds buffers in the library's layout (``reference_counts``, another report's
    ``buffers()``); ``all_reduce`` sums the report over the ranks.  ``conf_mat()`` / ``precision()`` / ``recall()`` /
    ``save_conf_matrix`` are ``ConfusionMeter``'s, so a report can stand where a meter stands."""

    def __init__(self, nb_step: int, nb_agent: int, nb_class: int, options: Optional[ReportOptions] = None,
                 device="cpu", window_size: Optional[int] = None) -> None:
        self.options = ReportOptions() if options is None else options
        if not isinstance(self.options, ReportOptions):
            raise ValueError(f"options must be a ReportOptions, got {type(options).__name__}")
        if window_size is not None and window_size < 1:
            raise ValueError(f"window_size must be >= 1 or None, got {window_size}")
        self.nb_step, self.nb_agent, self.nb_class = int(nb_step), int(nb_agent), int(nb_class)
        self.layout = layout(self.nb_step, self.nb_agent, self.nb_class, self.options)
        self.device = th.device(device)
        self.window_size = window_size
        self._words, self._int_words = self.layout["words"], self.layout["int_words"]
        self._ring: Optional[th.Tensor] = None  # [window or 1][words] int64, the tail of each row holds fp64 bits
        self._count = 0                          # adds so far
        self._scratch: Optional[th.Tensor] = None
        self._extra: Optional[Tuple[th.Tensor, th.Tensor]] = None  # what merge / all_reduce brought
        ne = len(self.options.exit_thresholds)
        self._taus = (C.c_float * max(ne, 1))(*self.options.exit_thresholds)
        self._lib = None

    # -- writing ------------------------------------------------------------------------------------------------------
    def add(self, step_preds: th.Tensor, y: th.Tensor) -> None:
        want = (self.nb_step, self.nb_agent, self.nb_class)
        if step_preds.dim() != 4 or (step_preds.shape[0], step_preds.shape[1], step_preds.shape[3]) != want:
            raise ValueError(f"step_preds must be [{want[0]}, {want[1]}, Nb, {want[2]}], got {tuple(step_preds.shape)}")
        if not step_preds.is_cuda or step_preds.device != self.device:
            raise RuntimeError(f"step_preds lives on {step_preds.device}, the report on {self.device}: the HIP path "
                               "only reads device memory (there is no CPU implementation in this package)")
        if step_preds.dtype != th.float32:
            raise TypeError(f"step_preds must be float32, got {step_preds.dtype}")
        nb = step_preds.shape[2]
        if tuple(y.shape) != (nb,) or nb < 1:
            raise ValueError(f"y must be [{nb}] with at least one image, got {tuple(y.shape)}")
        if y.dtype != th.int64:
            raise TypeError(f"y must be int64, got {y.dtype}")
        from . import _lib

        if self._lib is None:
            self._lib = _lib.load()
        lib = self._lib
        step_preds = step_preds.detach().contiguous()
        y = y.to(self.device).contiguous()
        if self._ring is None:
            self._ring = th.zeros(self.window_size or 1, self._words, dtype=th.int64, device=self.device)
        need = lib.marl_report_scratch_bytes(self.nb_step, self.nb_agent, nb, self.nb_class, self.options.topk,
                                             self.options.bins, len(self.options.exit_thresholds))
        if self._scratch is None or self._scratch.numel() * 8 < need:
            self._scratch = th.empty((need + 7) // 8, dtype=th.int64, device=self.device)
        slot = self._ring[self._count % self.window_size if self.window_size else 0]
        _lib.check(lib.marl_episode_report(
            step_preds.data_ptr(), y.data_ptr(), self.nb_step, self.nb_agent, nb, self.nb_class, self.options.topk,
            self.options.bins, self._taus, len(self.options.exit_thresholds), 0 if self.window_size else 1,
            slot.data_ptr(), self._words * 8, self._scratch.data_ptr(), self._scratch.numel() * 8,
            th.cuda.current_stream(self.device).cuda_stream))
        self._count += 1

    def merge(self, int_buf: th.Tensor, f64_buf: th.Tensor) -> None:
        """Adds a report in the library's layout (``reference_counts``' or ``buffers()``' pair)."""
        if (int_buf.dtype != th.int64 or f64_buf.dtype != th.float64 or int_buf.numel() != self._int_words or
                f64_buf.numel() != self._words - self._int_words):
            raise ValueError(f"merge: an int64 [{self._int_words}] and a float64 [{self._words - self._int_words}] "
                             "buffer of this report's layout needed")
        i, f = int_buf.to(self.device).reshape(-1), f64_buf.to(self.device).reshape(-1)
        self._extra = (i.clone(), f.clone()) if self._extra is None else (self._extra[0] + i, self._extra[1] + f)

    def all_reduce(self, group=None) -> None:
        """Data-parallel evaluation: every rank saw its shard; sum both buffers over the ranks so that the report
        describes the WHOLE set on every rank (as ``ConfusionMeter.all_reduce``)."""
        from .parallel import _all_reduce_sum

        i, f = self.buffers()
        i, f = i.contiguous(), f.contiguous()
        _all_reduce_sum(i, group)
        _all_reduce_sum(f, group)
        # (the reduced sums replace what this rank held, as ConfusionMeter.all_reduce replaces its window)
        self._count = 0
        if self._ring is not None:
            self._ring.zero_()
        self._extra = (i, f)

    # -- reading (synchronises) ---------------------------------------------------------------------------------------
    def buffers(self) -> Tuple[th.Tensor, th.Tensor]:
        """(int64 buffer, float64 buffer): the sum of what the window holds and of what was merged."""
        iw = self._int_words
        i = th.zeros(iw, dtype=th.int64, device=self.device)
        f = th.zeros(self._words - iw, dtype=th.float64, device=self.device)
        if self._ring is not None and self._count:
            rows = self._ring[: min(self._count, self.window_size) if self.window_size else 1]
            i = i + rows[:, :iw].sum(dim=0)
            f = f + rows[:, iw:].contiguous().view(th.float64).sum(dim=0)
        if self._extra is not None:
            i, f = i + self._extra[0], f + self._extra[1]
        return i, f

    def fields(self) -> Dict[str, th.Tensor]:
        i, f = self.buffers()
        return split_fields(i, f, self.layout)

    def conf_mat(self) -> th.Tensor:
        return self.fields()["confusion"]

    def precision(self) -> th.Tensor:
        cm = self.conf_mat().to(th.float)
        return cm.diagonal() / (cm.sum(dim=0) + 1e-8)

    def recall(self) -> th.Tensor:
        cm = self.conf_mat().to(th.float)
        return cm.diagonal() / (cm.sum(dim=1) + 1e-8)

    def save_conf_matrix(self, epoch: int, output_dir: str, stage: str) -> str:
        from .metrics import ConfusionMeter

        return ConfusionMeter.save_conf_matrix(self, epoch, output_dir, stage)

    def result(self) -> dict:
        """Plain Python numbers and lists.  ``topk[t][j - 1]`` is the top-j accuracy of step t (j = 1 .. topk);
        ``ece`` = sum over the bins of |cal_hit - cal_conf| / n; per threshold ``mean_steps`` = sum_e (e + 1) *
        exit_hist[e] / n.  With n = 0 every ratio is 0."""
        return result_from_fields({k: v.cpu() for k, v in self.fields().items()}, self.options, self.nb_agent)

    def to_json(self, path: str) -> str:
        with open(path, "w") as fh:
            json.dump(self.result(), fh, indent=1)
        return path

    def save_step_curve(self, path: str) -> str:
        """Accuracy per step as a PNG: the vote bold, every agent thin (matplotlib imported on use)."""
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt

        res = self.result()
        steps = list(range(1, self.nb_step + 1))
        fig, ax = plt.subplots()
        for a in range(self.nb_agent):
            ax.plot(steps, [row[a] for row in res["agent_accuracy"]], color="tab:gray", linewidth=0.6, alpha=0.6)
        ax.plot(steps, res["accuracy"], color="tab:blue", linewidth=2.5, label="vote")
        ax.set_xlabel("step")
        ax.set_ylabel("accuracy")
        ax.set_title(f"accuracy per step ({res['n']} images)")
        ax.legend()
        fig.savefig(path)
        plt.close(fig)
        return path


def result_from_fields(f: Dict[str, th.Tensor], options: ReportOptions, nb_agent: int) -> dict:
    """``EpisodeReport.result`` from the fields of a report (``split_fields``; host tensors)."""
    n = int(f["n"][0])
    d = float(max(n, 1))
    ns = f["vote_hit"].shape[0]
    k = options.topk
    cal_hit, cal_conf = f["cal_hit"].double(), f["cal_conf"].double()
    steps = th.arange(1, ns + 1, dtype=th.float64)
    exits: List[dict] = []
    for j, tau in enumerate(options.exit_thresholds):
        hist = f["exit_hist"][j]
        exits.append({"threshold": tau, "mean_steps": float((hist.double() * steps).sum()) / d,
                      "exit_accuracy": int(f["exit_hit"][j]) / d, "exit_hist": hist.tolist()})
    return {
        "n": n,
        "skipped": int(f["skipped"][0]),
        "accuracy": (f["vote_hit"].double() / d).tolist(),
        "topk": (f["rank_hist"][:, :k].cumsum(dim=1).double() / d).tolist(),
        "agent_accuracy": (f["agent_hit"].double() / d).tolist(),
        "agreement": (f["agree"].double() / (d * nb_agent)).tolist(),
        "nll": (f["nll_sum"].double() / d).tolist(),
        "ece": float((cal_hit - cal_conf).abs().sum()) / d,
        "calibration": {"count": f["cal_count"].tolist(), "hit": f["cal_hit"].tolist(),
                        "conf": f["cal_conf"].tolist()},
        "confusion": f["confusion"].tolist(),
        "exits": exits,
    }


def step_table(res: dict, options: ReportOptions) -> List[str]:
    """The lines ``test --report`` prints: one row per step, one line per exit threshold."""
    k = options.topk
    lines = [f"{'step':>4} {'acc':>7} {'top' + str(k):>7} {'nll':>8} {'best':>7} {'worst':>7} {'agree':>7}"]
    for t, acc in enumerate(res["accuracy"]):
        ag = res["agent_accuracy"][t]
        lines.append(f"{t + 1:>4} {acc:>7.4f} {res['topk'][t][k - 1]:>7.4f} {res['nll'][t]:>8.4f} {max(ag):>7.4f} "
                     f"{min(ag):>7.4f} {res['agreement'][t]:>7.4f}")
    for e in res["exits"]:
        lines.append(f"exit at confidence >= {e['threshold']:.4g}: mean steps {e['mean_steps']:.3f}, "
                     f"accuracy {e['exit_accuracy']:.4f}")
    return lines


def summary_metrics(res: dict, options: ReportOptions, prefix: str) -> Dict[str, float]:
    """``{prefix}_acc``, ``{prefix}_top{k}``, ``{prefix}_nll`` (last step) and ``{prefix}_ece``."""
    k = options.topk
    return {f"{prefix}_acc": res["accuracy"][-1], f"{prefix}_top{k}": res["topk"][-1][k - 1],
            f"{prefix}_nll": res["nll"][-1], f"{prefix}_ece": res["ece"]}


def parse_exit_at(spec: Optional[str]) -> Tuple[float, ...]:
    """``--exit-at t1,t2,...`` -> thresholds."""
    if spec is None or spec.strip() == "":
        return ()
    try:
        return tuple(float(s) for s in spec.split(","))
    except ValueError:
        raise ValueError(f'--exit-at takes comma-separated numbers, got "{spec}"') from None
