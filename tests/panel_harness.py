"""Shared by tests/test_gpu_panel_kernels.py (GPU) and tests/test_panel_plan_host.py (CPU): the case grid of the panel
kernels' own entry points (include/marl_hip_panelops.h), each case's witness over marl_panel_plan, the descriptor
builders, and an independent Python restatement of the launchers' host arithmetic (csrc/panel.hip).

A case is a plain description (widths, rows, grouping, options); `fwd_desc` / `bwd_desc` turn it into the C descriptor
over tensors of any device - the plan entry dereferences none of them, so the host tests use CPU tensors."""
import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch as th

SENT = -777.25  # sentinel of every output buffer: exactly representable, far outside every result
PANEL_ROWS, MAX_WAVES, MAX_LDS = 16, 12, 144 * 1024


def r4(v):
    return (v + 3) & ~3


def r16(v):
    return (v + 15) & ~15


def frag_groups(k):
    """16-wide K groups of a fragment-order weight copy (tests/test_gpu_panel_wfrag.py states the layout)"""
    return (k + 15) // 16


def frag_floats(n, k):
    """floats of the fragment-order copy of an [n, k] matrix: 32-row tiles, three groups of slack"""
    return (((n + 31) // 32) * frag_groups(k) + 3) * 512


def gamma_n(n):
    """gamma_n = n u / (1 - n u), u = 2^-24: the bound of any fp32 sum of n rounded terms (Higham, Lemma 3.1)"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


# ---- independent restatement of the launchers' host arithmetic (csrc/panel.hip) -------------------------------
def py_stride(k):
    return r16(k) + 4


def py_waves_for(k, n):
    nt = (n + 31) // 32
    w = max(nt * ((r16(k) + 63) // 64), nt)
    if w <= MAX_WAVES:
        return w
    return -1 if nt > MAX_WAVES else (MAX_WAVES // nt) * nt


def py_ksplit(k, nt, nwaves):
    return max(1, min(nwaves // nt, (r16(k) + 63) // 64))


def py_slices(k, n_out, nwaves):
    nt = (n_out + 31) // 32
    ks = py_ksplit(k, nt, nwaves)
    kper = r16(-(-r16(k) // ks))
    empty = sum(1 << s for s in range(ks) if s * kper >= r16(k))
    return {"nt": nt, "ks": ks, "kper": kper, "empty": empty}


def py_fwd_plan(probs):
    """probs: [(k0, widths, mixed)] -> waves, LDS bytes and the per-layer slices of launch_panel_fwd"""
    waves, x0, x1, prm = 1, 0, 0, 0
    for k0, widths, _ in probs:
        kin, s0, s1 = k0, PANEL_ROWS * py_stride(k0), 0
        for l, n in enumerate(widths):
            waves = max(waves, py_waves_for(kin, n))
            v = PANEL_ROWS * py_stride(n)
            if l & 1:
                s0 = max(s0, v)
            else:
                s1 = max(s1, v)
            kin = n
        x0, x1, prm = max(x0, s0), max(x1, s1), max(prm, 3 * sum(widths))
    waves = max(waves, 4)
    floats = x0 + x1 + (MAX_WAVES + 1) * 32 + (waves - 1) * 512 + prm + 16 + (256 if probs[0][2] else 0)
    layers = []
    for k0, widths, _ in probs:
        kin = k0
        for n in widths:
            layers.append(dict(py_slices(kin, n, waves), layer_waves=py_waves_for(kin, n), ln_slots=2 if n <= 128 else 6))
            kin = n
    return {"waves": waves, "lds_bytes": 4 * floats, "layers": layers}


def py_bwd_plan(layers, lddx, mixed=False, cellb=None):
    """layers: [(n, k_in)] last to first; cellb: None or (n, ldg, ldc, lddc) -> launch_panel_bwd's plan"""
    k_last = layers[-1][1]
    tail = k_last % 4 == 0 and lddx % 4 == 0 and (
        cellb is None or (all(v % 4 == 0 for v in cellb) and cellb[0] == k_last))
    retried = False
    while True:
        waves, pmax, nmax, prm = 8, 0, 0, 0
        for l, (n, k_in) in enumerate(layers):
            w = py_waves_for(n, k_in)
            waves = max(waves, MAX_WAVES if w < 0 else w)
            nmax, pmax = max(nmax, n), max(pmax, py_stride(n))
            if l + 1 < len(layers) or tail:
                pmax = max(pmax, py_stride(k_in))
            prm += 2 * n
        waves = min(waves, MAX_WAVES)
        floats = 2 * PANEL_ROWS * pmax + prm + 16 + waves * 2 * nmax + (waves - 1) * 512 + PANEL_ROWS
        lds = 4 * (floats + (256 if mixed else 0))
        if lds > MAX_LDS and tail:
            tail, retried = False, True
            continue
        break
    return {"waves": waves, "lds_bytes": lds, "tail_lds": int(tail), "retried": int(retried),
            "maxc": 2 if nmax <= 128 else 6, "ok": lds <= MAX_LDS,
            "layers": [dict(py_slices(n, k_in, waves), rounds=int(py_waves_for(n, k_in) < 0)) for n, k_in in layers]}


# ---- cases ------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Fwd:
    """One forward problem: k0 -> widths[0] -> widths[1] ...  form: 'plain' (16 consecutive rows per workgroup),
    'staged' (message mean over the other agents while staging x; m = na * nb) or 'chain' (a workgroup owns all agents
    of by_batch images; agg_at > 0 aggregates layer agg_at's input in the workgroup - mean, or the mixing matrix)."""
    name: str
    k0: int
    widths: Tuple[int, ...]
    m: int
    form: str = "plain"
    na: int = 0
    nb: int = 0
    agg_at: int = 0
    mix: bool = False
    pad: int = 0       # 1: padded leading dimensions (NaN behind the columns the kernel may read)
    save: int = 1      # 0: z and stats are not kept
    image: Optional[Tuple[int, int, int]] = None  # (row0, col0, steps) of the last layer's activation image
    witness: Tuple[str, ...] = ()


@dataclass(frozen=True)
class Cell:
    n: int
    rows: int = 0        # ride-along cell only
    g3: int = 0          # the image of the gate gradients is asked for
    skip: int = 0        # skip_f32
    ld_off: int = 0      # added to the leading dimensions (1: breaks the four-wide form)


@dataclass(frozen=True)
class Bwd:
    """One backward launch; layers (n, k_in) are listed LAST layer first, as the kernel walks them."""
    name: str
    layers: Tuple[Tuple[int, int], ...]
    m: int
    form: str = "plain"
    na: int = 0
    nb: int = 0
    agg_at: int = 0
    mix: bool = False
    pad: int = 0
    da2: int = 0
    accumulate: int = 0
    lddx_off: int = 0   # added to lddx (1: no 16-byte rows, the LDS tail is off)
    cell: Optional[Cell] = None
    cellb: Optional[Cell] = None
    witness: Tuple[str, ...] = ()


ROWS = (1, 15, 16, 17, 259)
AGENTS = (1, 2, 5, 16)
NB_OF = {1: 19, 2: 11, 5: 7, 16: 3}  # images: no multiple of by_batch = 16 // na except where by_batch = 1 (na = 16)

# forward widths (K, n): name -> (K, n, witness over the one-layer plan)
FWD_WIDTHS = {
    "c3_encoder_in": (256, 128, ("ln_slots == [2]", "nt == [4]", "ks == [3]", "waves == 12")),
    "two_slot_edge": (128, 64, ("ln_slots == [2]", "nt == [2]", "ks == [2]", "waves == 4")),
    "first_six_slot": (64, 129, ("ln_slots == [6]", "nt == [5]", "ks == [1]")),
    "k_not_mult_4": (23, 22, ("ks == [1]", "kper == [32]", "nt == [1]")),
    "below_one_group": (7, 13, ("ks == [1]", "kper == [16]", "nt == [1]")),
    "k_tail_40": (40, 100, ("nt == [4]", "ks == [1]", "kper == [48]")),
    "widest_row": (96, 384, ("nt == [12]", "ln_slots == [6]", "waves == 12", "ks == [1]")),
    "k_split_400": (400, 32, ("ks == [7]", "kper == [64]", "empty == [0]")),
    "empty_slices_780": (780, 32, ("waves == 12", "ks == [12]", "kper == [80]", "empty == [0b110000000000]")),
    "twelve_slices_1024": (1024, 32, ("ks == [12]", "kper == [96]", "empty == [0b100000000000]")),
    "one_column": (16, 1, ("nt == [1]", "ks == [1]", "waves == 4")),
}


def _fwd_grid():
    out = []
    for wi, (tag, (k, n, wit)) in enumerate(FWD_WIDTHS.items()):
        for ri, m in enumerate(ROWS):
            out.append(Fwd(f"{tag}-m{m}", k, (n,), m, pad=(wi + ri) % 2, save=(wi + 2 * ri) % 3 != 0,
                           witness=wit + (f"blocks == {-(-m // 16)}",)))
    # layers
    out.append(Fwd("two_layers_c3_encoder-m259", 256, (128, 64), 259, pad=1,
                   witness=("ln_slots == [2, 2]", "ks == [3, 2]", "waves == 12")))
    out.append(Fwd("two_layers_six_then_two_slots-m17", 40, (129, 100), 17,
                   witness=("ln_slots == [6, 2]", "nt == [5, 4]")))
    out.append(Fwd("image_of_last_layer-m37", 64, (96, 64), 37, image=(5, 16, 7),
                   witness=("nlayers == 2", "ln_slots == [2, 2]")))
    # (the six-slot row pass; 384 columns are two passes of the image loop's 256 columns per wave)
    out.append(Fwd("image_six_slots_two_passes-m17", 96, (384,), 17, pad=1, image=(2, 16, 26),
                   witness=("ln_slots == [6]", "384 > 256")))
    for i, na in enumerate(AGENTS):
        nb = NB_OF[na]
        bb = 16 // na
        part = () if na == 16 else (f"{nb} % {bb} != 0",)
        w = (f"by_batch == [{bb}, 0]", f"blocks == {-(-nb // bb)}") + part
        out.append(Fwd(f"staged_mean-na{na}", 32, (64, 48), na * nb, "staged", na, nb, pad=i % 2,
                       witness=(f"blocks == {-(-na * nb // 16)}",)))
        for mix in (False, True):
            out.append(Fwd(f"chain4_{'mix' if mix else 'mean'}-na{na}", 40, (64, 32, 64, 48), na * nb, "chain", na, nb,
                           agg_at=2, mix=mix, pad=(i + mix) % 2, save=not (mix and na == 2),
                           witness=w + ("nlayers == 4",)))
    return out


FWD_CASES = _fwd_grid()
# two problems in one launch: a 4-layer chain beside a 1-layer plain problem of other widths (shared LDS offsets / waves)
FWD_PAIR = (Fwd("pair_chain", 40, (64, 32, 64, 48), 5 * 7, "chain", 5, 7, agg_at=2),
            Fwd("pair_plain", 96, (384,), 100, pad=1))
FWD_PAIR_WITNESS = ("waves == 12", "nlayers == 5", "blocks == 7", "nt == [2, 1, 2, 2, 12]", "by_batch == [3, 0]")

# backward (n, k_in): name -> (n, k_in, witness)
BWD_WIDTHS = {
    "two_slots": (128, 64, ("maxc == 2", "tail_lds == 1", "retried == 0")),
    "first_six_slot": (129, 64, ("maxc == 6", "tail_lds == 1")),
    "widest_row": (384, 96, ("maxc == 6", "tail_lds == 1", "nt == [3]", "ks == [4]", "waves == 12")),
    "tail_off_by_alignment": (22, 23, ("tail_lds == 0", "retried == 0", "maxc == 2")),
    "tile_rounds": (24, 400, ("rounds == [1]", "nt == [13]", "waves == 12", "tail_lds == 1")),
    "retry_without_tail": (32, 1024, ("retried == 1", "tail_lds == 0", "rounds == [1]")),
}


def _bwd_grid():
    out = []
    for wi, (tag, (n, k, wit)) in enumerate(BWD_WIDTHS.items()):
        for ri, m in enumerate(ROWS):
            out.append(Bwd(f"{tag}-m{m}", ((n, k),), m, pad=(wi + ri) % 2, da2=(wi + ri // 2) % 2,
                           accumulate=(wi + ri + 1) % 2, witness=wit + (f"blocks == {-(-m // 16)}",)))
    out.append(Bwd("two_layers-m259", ((64, 128), (128, 256)), 259, da2=1, witness=("maxc == 2", "nlayers == 2")))
    out.append(Bwd("two_layers_accumulate_partial_panel-m17", ((100, 129), (129, 40)), 17, accumulate=1, pad=1,
                   witness=("maxc == 6", "tail_lds == 1", "17 % 16 != 0")))
    for i, na in enumerate(AGENTS):
        nb = NB_OF[na]
        bb = 16 // na
        w = (f"by_batch == [{bb}, 0]", f"blocks == {-(-nb // bb)}")
        out.append(Bwd(f"staged_mean-na{na}", ((48, 64), (64, 32)), na * nb, "staged", na, nb, pad=i % 2,
                       accumulate=i % 2))
        for mix in (False, True):
            out.append(Bwd(f"chain4_{'mix' if mix else 'mean'}-na{na}", ((48, 64), (64, 32), (32, 64), (64, 40)),
                           na * nb, "chain", na, nb, agg_at=2, mix=mix, pad=(i + mix) % 2, da2=(i + mix) % 2,
                           accumulate=(i + 1) % 2, witness=w + ("nlayers == 4", "maxc == 2")))
    # ride-along cell: scalar (n = 23, or rows without 16-byte alignment) and four-wide; rows != m, no multiple of the block
    ride = {"scalar_n23": Cell(23, rows=77), "vec4_n64": Cell(64, rows=77), "vec4_image": Cell(64, rows=77, g3=1),
            "vec4_image_skip_f32": Cell(64, rows=77, g3=1, skip=1),
            "scalar_by_ld_image_asked": Cell(64, rows=77, g3=1, skip=1, ld_off=1)}
    for tag, c in ride.items():
        vec = int(c.n % 4 == 0 and not c.ld_off)
        out.append(Bwd(f"ride_along_cell_{tag}", ((64, 32),), 37, cell=c,
                       witness=(f"cell_vec4 == {vec}", f"cell_img_done == {int(vec and c.g3)}",
                                f"cell_blocks == {-(-(77 * (c.n // 4 if vec else c.n)) // 512)}", "77 % 16 != 0")))
    epi = {"tail": Cell(64), "tail_image": Cell(64, g3=1), "tail_image_skip_f32": Cell(64, g3=1, skip=1)}
    for i, (tag, c) in enumerate(epi.items()):
        out.append(Bwd(f"epilogue_cell_{tag}", ((48, 64),), 37, accumulate=i % 2, cellb=c,
                       witness=("tail_lds == 1", f"cellb_img_done == {c.g3}")))
    out.append(Bwd("epilogue_cell_tail_off_image_fallback", ((48, 64),), 37, accumulate=1, lddx_off=1,
                   cellb=Cell(64, g3=1, skip=1), witness=("tail_lds == 0", "cellb_img_done == 0")))
    out.append(Bwd("epilogue_cell_scalar_n23", ((48, 23),), 37, cellb=Cell(23),
                   witness=("tail_lds == 0", "cellb_img_done == 0")))
    return out


BWD_CASES = _bwd_grid()


# ---- descriptors ------------------------------------------------------------------------------------------------
def _p(t):
    return t.data_ptr() if t is not None else None


def fwd_ld(case, width):
    return r4(width) + 8 * case.pad


class FwdBufs:
    """Inputs (from CPU fp32 tensors) and sentinel-filled outputs of one forward problem on `device`."""

    def __init__(self, case, inp, device):
        self.case, self.inp = case, inp
        m, k0 = case.m, case.k0
        self.ldx = fwd_ld(case, k0)
        nan = float("nan")
        x = th.full((m + 2, self.ldx), nan)
        x[:, : r4(k0)] = 0.0  # the columns up to the next multiple of 4 are read: zero, as the product keeps them
        x[:m, :k0] = inp["x"]
        self.x = x.to(device)
        self.w, self.ldw, self.vec = [], [], []
        kin = k0
        for l, n in enumerate(case.widths):
            ldw = kin + 3 * case.pad
            w = th.full((n, ldw), nan)
            w[:, :kin] = inp["w"][l]
            self.w.append(w.to(device))
            self.ldw.append(ldw)
            self.vec.append([inp[k][l].to(device) for k in ("bias", "gamma", "beta")])
            kin = n
        rows = m + 3
        self.ld = [fwd_ld(case, n) for n in case.widths]
        self.z = [th.full((rows, ld), SENT, device=device) if case.save else None for ld in self.ld]
        self.stats = [th.full((rows, 2), SENT, device=device) if case.save else None for _ in self.ld]
        self.a = [th.full((rows, ld), SENT, device=device) for ld in self.ld]
        self.xbar = None
        if case.form == "staged":
            self.xbar = th.full((rows, self.ldx), SENT, device=device)
            self.ld_xbar = self.ldx
        elif case.agg_at:
            self.ld_xbar = fwd_ld(case, case.widths[case.agg_at - 1])
            self.xbar = th.full((rows, self.ld_xbar), SENT, device=device)
        self.mix = inp["mix"].to(device).contiguous() if case.mix else None
        self.a3 = None

    def desc(self, P):
        c = self.case
        P.x, P.ldx, P.k0, P.m, P.nlayers = _p(self.x), self.ldx, c.k0, c.m, len(c.widths)
        for l, n in enumerate(c.widths):
            L = P.layer[l]
            L.w, L.ldw = _p(self.w[l]), self.ldw[l]
            L.bias, L.gamma, L.beta = (_p(v) for v in self.vec[l])
            L.n, L.z, L.ldz, L.stats, L.a, L.lda = n, _p(self.z[l]), self.ld[l], _p(self.stats[l]), _p(self.a[l]), self.ld[l]
            if c.image and l == len(c.widths) - 1 and self.a3 is not None:
                L.a3, L.a3_row0, L.a3_col0, L.a3_steps = _p(self.a3), c.image[0], c.image[1], c.image[2]
        if c.form == "staged":
            P.agg_na, P.agg_nb = c.na, c.nb
        if c.form == "chain":
            P.by_batch, P.g_na, P.g_nb, P.agg_at = -1, c.na, c.nb, c.agg_at
        if self.xbar is not None:
            P.xbar, P.ld_xbar = _p(self.xbar), self.ld_xbar
        P.mix = _p(self.mix)
        return P


def fwd_inputs(case, seed=0):
    g = th.Generator().manual_seed(seed + 7919 * len(case.name) + case.k0 * 31 + case.m)
    inp = {"x": th.randn(case.m, case.k0, generator=g), "w": [], "bias": [], "gamma": [], "beta": []}
    kin = case.k0
    for n in case.widths:
        inp["w"].append(th.randn(n, kin, generator=g) / kin ** 0.5)
        inp["bias"].append(th.randn(n, generator=g) * 0.5)
        inp["gamma"].append(1.0 + 0.25 * th.randn(n, generator=g))
        inp["beta"].append(0.25 * th.randn(n, generator=g))
        kin = n
    if case.mix:
        inp["mix"] = mixing_matrix(case.na, g)
    return inp


def mixing_matrix(na, g):
    """non-symmetric, with exact zeros (every third entry off the diagonal, and the whole column of the last agent
    except its own row, so that one sender reaches nobody else)"""
    mtx = th.randn(na, na, generator=g) * 0.5
    for a in range(na):
        for b in range(na):
            if a != b and ((a + 2 * b) % 3 == 0 or b == na - 1):
                mtx[a, b] = 0.0
    return mtx


def fwd_descs(bufs):
    from marlclassification_amd import _lib

    arr = (_lib.PanelFwdProb * len(bufs))()
    for i, b in enumerate(bufs):
        b.desc(arr[i])
    return arr


def fwd_scratch_bytes(lib, cases):
    tot = 0
    for c in cases:
        ks = (c.k0,) + tuple(c.widths[:-1])
        n = len(c.widths)
        tot += lib.marl_panel_scratch_bytes(0, n, (C.c_int * n)(*c.widths), (C.c_int * n)(*ks))
    return tot


def fwd_plan(cases, device="cpu"):
    """marl_panel_plan of one launch of these forward problems (no GPU needed)"""
    from marlclassification_amd import _lib

    lib = _lib.load()
    bufs = [FwdBufs(c, fwd_inputs(c), device) for c in cases]
    out = _lib.PanelPlan()
    _lib.check(lib.marl_panel_plan(fwd_descs(bufs), len(bufs), None, C.byref(out)))
    return out.as_dict()


# ---- backward -----------------------------------------------------------------------------------------------------
def cell_inputs(c, rows, g):
    n = c.n
    t = {"gates": th.cat([th.sigmoid(th.randn(rows, n, generator=g)), th.sigmoid(th.randn(rows, n, generator=g)),
                          th.tanh(th.randn(rows, n, generator=g)), th.sigmoid(th.randn(rows, n, generator=g))], dim=1),
         "c_prev": th.randn(rows, n, generator=g), "c_new": th.randn(rows, n, generator=g),
         "dc": th.randn(rows, n, generator=g), "dh": th.randn(rows, n, generator=g)}
    # small |c|: where 1 - tanh(c)^2 and tanh(c) of a fast tanh would show an absolute error first
    t["c_new"][::3] = (th.rand(t["c_new"][::3].shape, generator=g) * 2 - 1) * 1e-3
    return t


def bwd_inputs(case, seed=0):
    g = th.Generator().manual_seed(seed + 104729 * len(case.name) + case.m + 13 * case.layers[0][0])
    m = case.m
    inp = {"da": th.randn(m, case.layers[0][0], generator=g), "da2": th.randn(m, case.layers[0][0], generator=g),
           "z": [], "gamma": [], "beta": [], "w": [], "dx0": th.randn(m, case.layers[-1][1], generator=g)}
    for n, k in case.layers:
        inp["z"].append(th.randn(m, n, generator=g) * 1.5 + 0.3)
        inp["gamma"].append(1.0 + 0.25 * th.randn(n, generator=g))
        inp["beta"].append(0.25 * th.randn(n, generator=g))
        inp["w"].append(th.randn(n, k, generator=g) / n ** 0.5)
    if case.mix:
        inp["mix"] = mixing_matrix(case.na, g)
    if case.cell:
        inp["cell"] = cell_inputs(case.cell, case.cell.rows, g)
    if case.cellb:
        inp["cellb"] = cell_inputs(case.cellb, m, g)
    return inp


def stats_of(z):
    """(mean, rstd) of each row as the forward keeps them: float64 arithmetic, rounded to fp32"""
    z64 = z.double()
    mean = z64.mean(dim=1)
    var = ((z64 - mean[:, None]) ** 2).mean(dim=1)
    return th.stack([mean, 1.0 / th.sqrt(var + 1e-5)], dim=1).float()


class CellBufs:
    def __init__(self, c, t, rows, device, lib):
        n = c.n
        self.c, self.rows = c, rows
        self.ldn = r4(n) + 4 + c.ld_off
        self.ldg = r4(4 * n) + 4 + c.ld_off

        def buf(src, ld):
            b = th.full((rows + 2, ld), SENT)
            b[:rows, : src.shape[1]] = src
            return b.to(device)

        self.gates, self.dc = buf(t["gates"], self.ldg), buf(t["dc"], self.ldn)
        self.c_prev, self.c_new, self.dh = buf(t["c_prev"], self.ldn), buf(t["c_new"], self.ldn), buf(t["dh"], self.ldn)
        self.g3 = None
        self.row0, self.steps = 3, (4 * n + 15) // 16 + 1
        if c.g3 and lib is not None:
            self.g3 = th.full((lib.marl_image_bytes(rows + self.row0 + 2, 16 * self.steps) + 256,), 0x5A,
                              dtype=th.uint8, device=device)

    def desc(self, D, image=True):
        D.dh, D.dc, D.gates, D.c_prev, D.c_new = _p(self.dh), _p(self.dc), _p(self.gates), _p(self.c_prev), _p(self.c_new)
        D.lddh, D.lddc, D.ldg, D.ldc, D.n = self.ldn, self.ldn, self.ldg, self.ldn, self.c.n
        if self.c.g3:
            D.g3 = _p(self.g3) if self.g3 is not None else 16  # (plans: only its presence matters)
            D.g3_row0, D.g3_steps = self.row0, self.steps
        D.skip_f32 = self.c.skip


class BwdBufs:
    def __init__(self, case, inp, device, lib=None, blocks=None):
        self.case, self.inp = case, inp
        m = case.m
        nan = float("nan")
        n0 = case.layers[0][0]
        self.ldda = r4(n0) + 8 * case.pad

        def grad_in(t):
            b = th.full((m + 2, self.ldda), nan)
            b[:, : r4(n0)] = 0.0
            b[:m, :n0] = t
            return b.to(device)

        self.da = grad_in(inp["da"])
        self.da2 = grad_in(inp["da2"]) if case.da2 else None
        self.z, self.stats, self.vec, self.w, self.ldw, self.dz, self.part, self.ld = [], [], [], [], [], [], [], []
        if blocks is None:
            blocks = -(-case.nb // (16 // case.na)) if case.form == "chain" else -(-m // 16)
        self.blocks = blocks
        for l, (n, k) in enumerate(case.layers):
            ld = r4(n) + 8 * case.pad
            z = th.full((m + 2, ld), nan)
            z[:m, :n] = inp["z"][l]
            self.z.append(z.to(device))
            self.stats.append(stats_of(inp["z"][l]).to(device))
            self.vec.append([inp["gamma"][l].to(device), inp["beta"][l].to(device)])
            ldw = k + 3 * case.pad
            w = th.full((n, ldw), nan)
            w[:, :k] = inp["w"][l]
            self.w.append(w.to(device))
            self.ldw.append(ldw)
            self.ld.append(ld)
            self.dz.append(th.full((m + 3, ld), SENT, device=device))
            self.part.append(th.full((blocks + 1, 2 * n), SENT, device=device))
        k_last = case.layers[-1][1]
        self.lddx = r4(k_last) + 8 * case.pad + case.lddx_off
        dx = th.full((m + 3, self.lddx), SENT)
        if case.accumulate:
            dx[:m, :k_last] = inp["dx0"]
        elif not case.cellb:
            dx[:m, :k_last] = nan  # a prefill that must not survive
        self.dx = dx.to(device)
        self.mix = inp["mix"].to(device).contiguous() if case.mix else None
        self.cell = CellBufs(case.cell, inp["cell"], case.cell.rows, device, lib) if case.cell else None
        self.cellb = CellBufs(case.cellb, inp["cellb"], m, device, lib) if case.cellb else None

    def desc(self):
        from marlclassification_amd import _lib

        c, P = self.case, _lib.PanelBwdProb()
        P.da, P.ldda, P.da2, P.ldda2 = _p(self.da), self.ldda, _p(self.da2), self.ldda
        P.m, P.nlayers = c.m, len(c.layers)
        for l, (n, k) in enumerate(c.layers):
            L = P.layer[l]
            L.z, L.ldz, L.stats, L.gamma, L.beta = _p(self.z[l]), self.ld[l], _p(self.stats[l]), _p(self.vec[l][0]), _p(self.vec[l][1])
            L.n, L.k_in, L.w, L.ldw, L.dz, L.lddz, L.part = n, k, _p(self.w[l]), self.ldw[l], _p(self.dz[l]), self.ld[l], _p(self.part[l])
        P.dx, P.lddx, P.accumulate = _p(self.dx), self.lddx, c.accumulate
        if c.form == "staged":
            P.agg_na, P.agg_nb = c.na, c.nb
        if c.form == "chain":
            P.by_batch, P.g_na, P.g_nb, P.agg_at = -1, c.na, c.nb, c.agg_at
        P.mix = _p(self.mix)
        if self.cellb:
            P.has_cellb = 1
            self.cellb.desc(P.cellb)
        if self.cell:
            P.has_cell, P.cell_rows = 1, c.cell.rows
            self.cell.desc(P.cell)
        return P


def bwd_scratch_bytes(lib, case):
    n = len(case.layers)
    return lib.marl_panel_scratch_bytes(1, n, (C.c_int * n)(*[a for a, _ in case.layers]),
                                        (C.c_int * n)(*[b for _, b in case.layers]))


def bwd_plan(case, device="cpu"):
    from marlclassification_amd import _lib

    lib = _lib.load()
    bufs = BwdBufs(case, bwd_inputs(case), device)
    out = _lib.PanelPlan()
    d = bufs.desc()
    _lib.check(lib.marl_panel_plan(None, 0, C.byref(d), C.byref(out)))
    return out.as_dict()


# ---- known-answer operands ------------------------------------------------------------------------------------------
def one_hot_rows(k):
    """[k, k]: row r = 2^(r % 5) e_r"""
    return th.diag(2.0 ** (th.arange(k) % 5).float())


def slice_kat(k, ks, kper, rows=16):
    """x [rows, k] with one 2^-s in each non-empty K slice s of every row (at a column that moves with the row, the
    slice's first and last column included), and the exact sums"""
    x = th.zeros(rows, k)
    want = th.zeros(rows, dtype=th.float64)
    for s in range(ks):
        lo, hi = s * kper, min((s + 1) * kper, k)
        if lo >= hi:
            continue
        for r in range(rows):
            col = lo if r == 0 else hi - 1 if r == 1 else lo + (5 * r + 3 * s) % (hi - lo)
            x[r, col] = 2.0 ** -s
            want[r] += 2.0 ** -s
    return x, want
