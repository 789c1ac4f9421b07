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
from typing import Optional, Sequence, Union

import torch as th

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
