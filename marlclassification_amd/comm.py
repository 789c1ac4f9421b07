"""Communication graphs of the message exchange.

A communication matrix ``M`` is fp32 ``[Na, Na]``, row = receiver, column = sender; an agent's aggregated
message is ``mbar[a] = sum_a' M[a, a'] * m[a']`` (``marl_comm_matrix`` in include/marl_hip.h).  The reference's
``aggregate_messages`` (networks/message.py:5-17) is ``full(na)``, the complete graph; ``None`` keeps that mean
on its own, unchanged code path.  An entry that is exactly 0 means "no link": that sender is skipped.

The constructors return CPU tensors (``model.set_comm(comm.ring(16).to(device))``); adjacency graphs are
row-normalised by degree (every neighbour weighs 1 / degree, an agent without neighbours receives zeros).
"""

from __future__ import annotations

import re
from typing import NamedTuple, Optional, Sequence, Union

import torch as th
from torch import nn

MAX_AGENTS = 32  # what the mixing kernel serves (mix_msg_kernel holds every agent's input in registers)


def from_adjacency(adj, self_loops: bool = False) -> th.Tensor:
    """Row-normalised mixing matrix of a 0/1 (or weighted) adjacency ``adj[receiver, sender]``; the diagonal is
    dropped unless ``self_loops``; a row of degree 0 stays all zero."""
    a = th.as_tensor(adj, dtype=th.float64).clone()
    if a.dim() != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1:
        raise ValueError(f"adjacency must be a square matrix, got shape {tuple(a.shape)}")
    if not th.isfinite(a).all():
        raise ValueError("adjacency has a non-finite entry")
    if not self_loops:
        a.fill_diagonal_(0.0)
    deg = a.sum(dim=1, keepdim=True)
    out = th.where(deg != 0, a / th.where(deg != 0, deg, th.ones_like(deg)), th.zeros_like(a))
    return out.to(th.float32)


def _check_na(na: int) -> int:
    if not isinstance(na, int) or isinstance(na, bool) or na < 1:
        raise ValueError(f"number of agents must be a positive integer, got {na!r}")
    return na


def full(na: int) -> th.Tensor:
    """The complete graph: (1 - I) / (na - 1), the reference's mean over the other agents (zeros for one agent)."""
    _check_na(na)
    return from_adjacency(th.ones(na, na))


def none(na: int) -> th.Tensor:
    """No communication: every agent receives zeros."""
    return th.zeros(_check_na(na), na, dtype=th.float32)


def ring(na: int, k: int = 1) -> th.Tensor:
    """Agent a hears a +- 1 .. a +- k (indices modulo na)."""
    _check_na(na)
    if not isinstance(k, int) or k < 1:
        raise ValueError(f"ring: k must be a positive integer, got {k!r}")
    a = th.zeros(na, na)
    for i in range(na):
        for d in range(1, k + 1):
            a[i, (i + d) % na] = 1.0
            a[i, (i - d) % na] = 1.0
    return from_adjacency(a)


def star(na: int, hub: int = 0) -> th.Tensor:
    """The hub hears every other agent; every other agent hears the hub only."""
    _check_na(na)
    if not isinstance(hub, int) or not 0 <= hub < na:
        raise ValueError(f"star: hub {hub!r} outside [0, {na})")
    a = th.zeros(na, na)
    a[hub, :] = 1.0
    a[:, hub] = 1.0
    return from_adjacency(a)


def grid(rows: int, cols: int) -> th.Tensor:
    """rows x cols lattice, agent r * cols + c hears its 4-neighbours (no wrap-around)."""
    _check_na(rows)
    _check_na(cols)
    na = rows * cols
    a = th.zeros(na, na)
    for r in range(rows):
        for c in range(cols):
            i = r * cols + c
            for dr, dc in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                rr, cc = r + dr, c + dc
                if 0 <= rr < rows and 0 <= cc < cols:
                    a[i, rr * cols + cc] = 1.0
    return from_adjacency(a)


def teams(sizes: Sequence[int]) -> th.Tensor:
    """Disjoint teams of consecutive agents, a complete graph inside each (block diagonal)."""
    sizes = list(sizes)
    if not sizes:
        raise ValueError("teams: no team sizes")
    for s in sizes:
        _check_na(s)
    na = sum(sizes)
    a = th.zeros(na, na)
    o = 0
    for s in sizes:
        a[o:o + s, o:o + s] = 1.0
        o += s
    return from_adjacency(a)


def validate(matrix, na: Optional[int]) -> th.Tensor:
    """``matrix`` as a contiguous fp32 [na, na] tensor (device kept); ValueError for another shape, more than
    ``MAX_AGENTS`` agents or a non-finite entry.  ``na`` None: any square size."""
    m = matrix if isinstance(matrix, th.Tensor) else th.as_tensor(matrix)
    if m.dim() != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
        raise ValueError(f"communication matrix must be square [Na, Na], got shape {tuple(m.shape)}")
    if na is not None and m.shape[0] != na:
        raise ValueError(f"communication matrix is {tuple(m.shape)} but there are {na} agents")
    if m.shape[0] > MAX_AGENTS:
        raise ValueError(f"communication matrix for {m.shape[0]} agents: at most {MAX_AGENTS} are supported")
    if m.is_complex() or m.dtype == th.bool:
        raise ValueError(f"communication matrix must be real-valued, got {m.dtype}")
    m = m.detach().to(th.float32).contiguous()
    if not bool(th.isfinite(m).all()):
        raise ValueError("communication matrix has a non-finite entry")
    return m


_INT = r"\d+"


def parse(text: str, na: int) -> Optional[th.Tensor]:
    """The command-line spelling: ``full | none | ring[:k] | star[:hub] | grid:RxC | teams:a,b,... | FILE.npy``
    for ``na`` agents.  ValueError for anything else (or a graph of another size)."""
    if not isinstance(text, str) or not text:
        raise ValueError("empty communication graph")
    _check_na(na)
    if text.endswith(".npy"):
        import numpy as np

        return validate(th.from_numpy(np.load(text, allow_pickle=False)), na)
    if text == "full":
        return full(na)
    if text == "none":
        return none(na)
    m = re.fullmatch(rf"ring(?::({_INT}))?", text)
    if m:
        return ring(na, int(m.group(1)) if m.group(1) else 1)
    m = re.fullmatch(rf"star(?::({_INT}))?", text)
    if m:
        return star(na, int(m.group(1)) if m.group(1) else 0)
    m = re.fullmatch(rf"grid:({_INT})x({_INT})", text)
    if m:
        return validate(grid(int(m.group(1)), int(m.group(2))), na)
    m = re.fullmatch(rf"teams:({_INT}(?:,{_INT})*)", text)
    if m:
        return validate(teams([int(v) for v in m.group(1).split(",")]), na)
    raise ValueError(f'unknown communication graph "{text}" (full | none | ring[:k] | star[:hub] | grid:RxC | '
                     "teams:a,b,... | FILE.npy)")


def check_spelling(text: str) -> str:
    """argparse ``type=``: the spelling only (the number of agents is known later)."""
    if text.endswith(".npy") and len(text) > 4:
        return text
    pats = ("full", "none", rf"ring(?::{_INT})?", rf"star(?::{_INT})?", rf"grid:{_INT}x{_INT}",
            rf"teams:{_INT}(?:,{_INT})*")
    if not any(re.fullmatch(p, text) for p in pats):
        raise ValueError(f'unknown communication graph "{text}"')
    return text


Graph = Union[str, th.Tensor, None]


# ---- range-limited communication: the graph follows the agents ------------------------------------------------------
METRICS = ("chebyshev", "euclidean")  # (the library's MARL_COMM_CHEBYSHEV / MARL_COMM_EUCLIDEAN, in this order)


class CommRange(NamedTuple):
    """``set_comm_range``'s setting: agents hear each other within ``radius`` pixels (window corners)."""

    radius: int
    metric: str = "chebyshev"
    normalize: bool = True

    @property
    def metric_id(self) -> int:
        return METRICS.index(self.metric)

    def spelling(self) -> str:
        """The command-line form ``R[:metric][:raw]`` (``parse_range`` reads it back)."""
        return (str(self.radius) + ("" if self.metric == "chebyshev" else ":" + self.metric) +
                ("" if self.normalize else ":raw"))


def check_range(radius, metric: str = "chebyshev", normalize: bool = True) -> CommRange:
    """The setting as a ``CommRange``; ValueError for a radius that is not an integer >= 0 (below 2^31) or an unknown
    metric."""
    if not isinstance(radius, int) or isinstance(radius, bool) or not 0 <= radius < 2 ** 31:
        raise ValueError(f"communication range: the radius must be an integer >= 0 (pixels), got {radius!r}")
    if metric not in METRICS:
        raise ValueError(f'communication range: unknown metric {metric!r} ("chebyshev" or "euclidean")')
    return CommRange(radius, metric, bool(normalize))


def check_range_base(base: th.Tensor, normalize: bool) -> None:
    """``normalize`` rescales a receiver's in-range weights to the row sum of the base: that needs a base >= 0."""
    if normalize and bool((base < 0).any()):
        raise ValueError("communication range with normalize=True needs a base matrix >= 0 (a row's in-range weights "
                         "are rescaled to the row's sum); use normalize=False for signed weights")


def parse_range(text: str) -> CommRange:
    """The command-line spelling ``R[:chebyshev|euclidean][:raw]`` (``raw``: normalize=False)."""
    m = re.fullmatch(rf"({_INT})(?::(chebyshev|euclidean))?(?::(raw))?", text) if isinstance(text, str) else None
    if not m:
        raise ValueError(f'unknown communication range "{text}" (R[:chebyshev|euclidean][:raw], R in pixels)')
    return check_range(int(m.group(1)), m.group(2) or "chebyshev", m.group(3) is None)


def range_matrices(base, pos, radius: int, metric: str = "chebyshev", normalize: bool = True) -> th.Tensor:
    """The mixing matrices of a range-limited exchange, ``[..., Na, Na]`` fp32 (row = receiver), for positions ``pos``
    ``[Na, ..., 2]`` (integers; the layout of ``step_pos[t]``: agents first): ``base[a, a']`` (None: ``full(Na)``)
    where agents a and a' are within ``radius`` pixels of each other - chebyshev: max(|dy|, |dx|) <= radius, euclidean:
    dy^2 + dx^2 <= radius^2 -, 0 elsewhere; an agent is always in range of itself, so the base's diagonal decides
    self-loops.  ``normalize``: every row is rescaled by S_a / s_a (S_a the row sum of the base, s_a of its in-range
    part), a row with s_a <= 0 is all zero - for ``full`` the mean over the in-range other agents.  This is what the
    fused episode builds in its kernels per (step, image) from the positions of the step that emitted the message; here
    in plain torch, for users, documentation and visualisation."""
    r = check_range(radius, metric, normalize)
    pos = th.as_tensor(pos)
    if pos.dim() < 2 or pos.shape[-1] != 2 or pos.is_floating_point() or pos.is_complex() or pos.dtype == th.bool:
        raise ValueError(f"positions must be an integer tensor [Na, ..., 2], got {pos.dtype} {tuple(pos.shape)}")
    na = pos.shape[0]
    b = full(na) if base is None else validate(base, na)
    check_range_base(b, r.normalize)
    p = pos.to(th.int64).movedim(0, -2)                      # [..., Na, 2]
    d = (p.unsqueeze(-2) - p.unsqueeze(-3)).abs()            # [..., Na(receiver), Na(sender), 2]
    if r.metric == "chebyshev":
        gate = d.amax(dim=-1) <= r.radius
    else:
        gate = (d * d).sum(dim=-1) <= r.radius * r.radius
    b = b.to(p.device)
    u = th.where(gate, b, th.zeros_like(b))
    if not r.normalize:
        return u
    big, small = b.sum(dim=-1, keepdim=True), u.sum(dim=-1, keepdim=True)
    ok = small > 0
    return th.where(ok, u * (big / th.where(ok, small, th.ones_like(small))), th.zeros_like(u))


# ---- live sources: a matrix that is learned -------------------------------------------------------------------------
def is_live(source) -> bool:
    """Is ``source`` a LIVE matrix source for ``set_comm`` - a tensor that requires grad, a module or a callable that
    returns the matrix - rather than a constant (which ``set_comm`` clones)?"""
    if isinstance(source, th.Tensor):
        return source.requires_grad
    return callable(source)


def evaluate(source, na: Optional[int], device) -> "tuple[th.Tensor, th.Tensor]":
    """One evaluation of a live source: (the matrix as the source gave it - attached to its autograd graph when grad
    mode is on -, its detached contiguous fp32 value, which is what the library reads).  Checks shape, dtype and
    device only: a finiteness check would synchronise the host with the device on every forward."""
    m = source if isinstance(source, th.Tensor) else source()
    if not isinstance(m, th.Tensor):
        raise TypeError(f"the communication source returned {type(m).__name__}, not a tensor")
    if m.dim() != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
        raise ValueError(f"communication matrix must be square [Na, Na], got shape {tuple(m.shape)}")
    if na is not None and m.shape[0] != na:
        raise ValueError(f"communication matrix is {tuple(m.shape)} but there are {na} agents")
    if m.shape[0] > MAX_AGENTS:
        raise ValueError(f"communication matrix for {m.shape[0]} agents: at most {MAX_AGENTS} are supported")
    if not m.is_floating_point():
        raise ValueError(f"a learnable communication matrix must be floating point, got {m.dtype}")
    if device is not None and m.device != th.device(device):
        raise ValueError(f"communication matrix lives on {m.device}, expected {th.device(device)}")
    return m, m.detach().to(th.float32).contiguous()


def leaves(source) -> "list[th.Tensor]":
    """The tensors an optimiser updates behind a live source: the tensor itself, a module's parameters that require
    grad, or what a callable's ``parameters()`` yields (a plain function has none to offer: [])."""
    if isinstance(source, th.Tensor):
        return [source] if source.requires_grad else []
    params = getattr(source, "parameters", None)
    if callable(params):
        return [p for p in params() if p.requires_grad]
    return []


class LearnableComm(nn.Module):
    """A learnable communication graph on a FIXED support: ``forward()`` is the row softmax of the logits over the
    support, so every row with a neighbour stays a convex combination of its neighbours and entries off the support
    are exact zeros - the mixing kernels keep skipping them and team isolation keeps holding bit for bit.  A row
    without support is all zero.

    ``init`` [Na, Na] (row = receiver): its entries on the support must be positive; the logits start at
    ``log(init)`` there, so ``forward()`` at construction is the row-normalised ``init`` (``comm.ring(16)`` gives
    ``comm.ring(16)``).  ``mask`` (bool [Na, Na], default ``init != 0``) is the support.  The logits' gradient off the
    support is exactly 0.  ``model.set_comm(LearnableComm(comm.ring(16)).to(device))`` makes it the model's live
    source; ``from_matrix`` / ``to_matrix`` are the checkpoint format (the matrix itself: ``--comm FILE.npy``)."""

    def __init__(self, init, mask=None) -> None:
        super().__init__()
        m = validate(init, None).to(th.float64)
        if mask is None:
            support = m != 0
        else:
            support = th.as_tensor(mask)
            if support.dtype != th.bool or tuple(support.shape) != tuple(m.shape):
                raise ValueError(f"mask must be a bool tensor of shape {tuple(m.shape)}, got {support.dtype} "
                                 f"{tuple(support.shape)}")
            support = support.to(m.device)
        if bool((m[support] <= 0).any()):
            raise ValueError("LearnableComm: entries of init on the support must be positive (they are softmax "
                             "weights: logits start at log(init))")
        logits = th.where(support, m.clamp_min(1e-300).log(), th.zeros_like(m)).to(th.float32)
        self.logits = nn.Parameter(logits)
        self.register_buffer("support", support.clone())

    @property
    def nb_agents(self) -> int:
        return self.logits.shape[0]

    def forward(self) -> th.Tensor:
        sup = self.support
        z = self.logits.masked_fill(~sup, float("-inf"))
        # (a row without support: shift by 0, exp(-inf) = 0, and the guarded denominator keeps it at 0 - no NaN in
        # the value or in the gradient; masked_fill / where cut the gradient off the support to exactly 0;
        # the shift is detached: the softmax does not depend on it
        top = z.detach().amax(dim=1, keepdim=True)
        top = th.where(th.isfinite(top), top, th.zeros_like(top))
        e = th.where(sup, (z - top).exp(), th.zeros_like(z))
        den = e.sum(dim=1, keepdim=True)
        return e / th.where(den > 0, den, th.ones_like(den))

    @classmethod
    def from_matrix(cls, matrix, mask=None) -> "LearnableComm":
        """From a stored matrix (``to_matrix`` / ``comm_epoch_{e}.npy``): same ``forward()``.  ``mask``: the stored
        support (``to_mask``).  Without it the support is ``matrix != 0``, which loses a link whose weight underflowed
        to exactly 0 in fp32; with it such a link stays on the support and restarts from the smallest positive
        weight."""
        if mask is None:
            return cls(matrix)
        m = validate(matrix, None)
        support = th.as_tensor(mask).to(m.device)
        if support.dtype != th.bool or tuple(support.shape) != tuple(m.shape):
            raise ValueError(f"mask must be a bool tensor of shape {tuple(m.shape)}")
        tiny = th.finfo(th.float32).tiny
        return cls(th.where(support & (m == 0), th.full_like(m, tiny), m), support)

    @th.no_grad()
    def to_mask(self) -> th.Tensor:
        """The support, on the CPU (bool [Na, Na]) - store it next to ``to_matrix()`` to reload with ``from_matrix``."""
        return self.support.detach().to("cpu").clone()

    @th.no_grad()
    def to_matrix(self) -> th.Tensor:
        """The current matrix, detached, on the CPU (fp32 [Na, Na]) - what ``--comm FILE.npy`` loads."""
        return self.forward().detach().to("cpu", th.float32).contiguous()
