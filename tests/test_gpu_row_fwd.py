"""GPU: the small row kernels of the step loop (csrc/rowops.hip) and marl_image_build through their own entry points
(include/marl_hip_rowops.h), against float64 references on the CPU (tests/row_cases.py) and the host model of the k16
image (tests/image_model.py), at the smallest shapes that reach every form of every launcher.

Every output buffer starts as a sentinel pattern between two guard regions: padding columns (ld > n) and the guards must
come back untouched.  Bounds are the project's own - FWD_TOL x max(1, |ref|max) for forward outputs and statistics,
GRAD_TOL x |ref|max for gradients - and the achieved errors go to the record ``row_fwd_errors``
(profiles/row_fwd_errors.json is one run)."""
import ctypes as C

import numpy as np
import pytest
import torch as th
import torch.nn.functional as F

from tests import image_model as im
from tests import row_cases as rc
from tests.buffers import SENTINEL, guarded, guards_intact
from tests.parity import Recorder  # (its fwd / grad hold FWD_TOL and GRAD_TOL)

pytestmark = pytest.mark.gpu

REC = Recorder("row_fwd_errors", "row_fwd")
EINVAL, ELIMIT = -1, -2
SENT32 = int(np.array([SENTINEL] * 4, dtype=np.uint8).view(np.int32)[0])


def _lib():
    from marlclassification_amd import _lib

    return _lib.load(), _lib.check


class Buf:
    """a [rows, ld] fp32 device matrix between two guards; ``data`` (CPU, [rows, n]) fills the first n columns, the rest
    - or everything - is the sentinel"""

    def __init__(self, device, rows, ld, data=None, offset=0, dtype=th.float32):
        self.rows, self.ld, self.offset = rows, ld, offset
        self.whole, self.view = guarded((rows, ld), dtype, device, offset)
        self.n = ld if data is None else data.shape[1]
        if data is not None:
            self.view[:, : self.n] = data.to(device)
        self.before = self.whole.clone()

    @property
    def ptr(self):
        return self.view.data_ptr()

    def cols(self, n):
        return self.view[:, :n].cpu()

    def intact_beyond(self, n, what):
        """columns >= n of every row and both guards hold what they held before the call"""
        assert guards_intact(self.whole, self.offset, self.rows * self.ld * 4), f"{what}: wrote outside the buffer"
        if n < self.ld:
            assert th.equal(self.view[:, n:].contiguous().view(th.int32),
                            th.full((self.rows, self.ld - n), SENT32, dtype=th.int32, device=self.view.device)), \
                f"{what}: wrote into the padding columns"

    def unchanged(self, what):
        assert th.equal(self.whole, self.before), f"{what}: a refused call wrote"


def _vec(device, t):
    return Buf(device, 1, t.numel(), t.reshape(1, -1))


def _bits(t):
    return t.contiguous().view(th.int32)


# ======================================================================================================================
# marl_image_build against the host model
# ======================================================================================================================
def _image_values(rows, k, seed):
    g = th.Generator().manual_seed(seed)
    x = th.randn(rows, k, generator=g) * th.exp2(th.rand(rows, k, generator=g) * 40 - 20)
    p = th.from_numpy(im.planted())
    flat = x.reshape(-1)
    idx = th.randperm(flat.numel(), generator=g)[: p.numel()]
    flat[idx] = p[: idx.numel()]
    return flat.reshape(rows, k)


def _build_image(device, x, ld):
    lib, check = _lib()
    rows, k = x.shape
    src = Buf(device, rows, ld, x)
    nbytes = lib.marl_image_bytes(rows, k)
    assert nbytes == im.image_bytes(rows, k)
    whole, img = guarded((nbytes,), th.uint8, device)
    check(lib.marl_image_build(src.ptr, ld, rows, k, img.data_ptr(), None))
    th.cuda.synchronize()
    assert guards_intact(whole, 0, nbytes), "marl_image_build wrote outside marl_image_bytes"
    return img.cpu().numpy()


@pytest.mark.parametrize("k", [1, 7, 16, 40, 100])
@pytest.mark.parametrize("rows", [1, 33, 95])
def test_image_build_equals_the_host_model(device, rows, k):
    x = _image_values(rows, k, 100 * rows + k)
    assert np.isin(im.planted().view(np.uint32)[: rows * k], x.numpy().view(np.uint32)).all()
    want = im.valid_rows(im.build(x.numpy()), rows, k)
    k4 = (k + 3) // 4 * 4
    for ld in (k4, k4 + 8):
        got = im.valid_rows(_build_image(device, x, ld), rows, k)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"rows={rows} k={k} ld={ld}: first difference at (row, step, plane, k%16) {bad[0]}"
    REC.put(f"image rows={rows} k={k}", {"valid_rows_equal_the_host_model": True, "lds": [k4, k4 + 8]})


def test_image_build_outside_the_exact_range_is_recorded(device):
    """subnormal inputs and finite inputs that round to a bf16 infinity are outside the equality (split.h): what the
    device returns for them is recorded, not asserted"""
    bits = np.array([0x00000001, 0x00400000, 0x807FFFFF, 0x0C000000, 0x7F7F8000, 0xFF7FFFFF, 0x7F7FFFFF, 0x0C7FFFFF],
                    dtype=np.uint32)
    x = th.from_numpy(bits.view(np.float32).copy()).reshape(1, -1)
    got = im.valid_rows(_build_image(device, x, 8), 1, 8)[0, 0]          # [plane, 16]
    with np.errstate(invalid="ignore"):
        want = im.valid_rows(im.build(x.numpy()), 1, 8)[0, 0]
    REC.put("image outside the exact range", {
        "input_bits": [f"{b:08x}" for b in bits],
        "device_planes": [[f"{v:04x}" for v in got[pl, :8]] for pl in range(3)],
        "host_model_planes": [[f"{v:04x}" for v in want[pl, :8]] for pl in range(3)]})
    assert np.all(got[:, 8:] == 0)  # (the K padding is still zero)


# ======================================================================================================================
# GroupNorm + SiLU forward, with the fused next-layer im2col
# ======================================================================================================================
def _gn_operands(device, rows, P, C, G, offset):
    z = rc.norm_input((rows, P, C), seed=1000 * rows + P * C + G, offset=offset)
    gamma, beta = rc.affine(C, C + P)
    act, stats = rc.gn_silu(z.double(), gamma.double(), beta.double(), G)
    return z, act, stats, Buf(device, rows, P * C, z.reshape(rows, -1)), _vec(device, gamma), _vec(device, beta)


def _gn_run(device, tag, rows, P, C, G, offset=False):
    lib, check = _lib()
    z, act, stats, zd, gd, bd = _gn_operands(device, rows, P, C, G, offset)
    ldo = P * C + 12
    for chw in (0, 1):
        out, st = Buf(device, rows, ldo), Buf(device, rows, 2 * G)
        check(lib.marl_gn_silu_fwd(zd.ptr, gd.ptr, bd.ptr, out.ptr, ldo, chw, st.ptr, rows, P, C, G, None, 0, 0, None))
        th.cuda.synchronize()
        ref = act if chw else act.permute(0, 2, 1)
        t = f"{tag} chw={chw}"
        out.intact_beyond(P * C, t)
        st.intact_beyond(2 * G, t)
        REC.fwd(f"{t} out", out.cols(P * C), ref.reshape(rows, -1))
        got = st.cols(2 * G).reshape(rows, G, 2)
        REC.fwd(f"{t} mean", got[..., 0], stats[..., 0])
        REC.fwd(f"{t} rstd", got[..., 1], stats[..., 1])


_GN = [(form, P, C, G) for form, cases in rc.GN_CASES.items() for (P, C, G) in cases]


@pytest.mark.parametrize("rows", rc.GN_ROWS)
@pytest.mark.parametrize("form,P,C,G", _GN)
def test_gn_silu_fwd(device, form, P, C, G, rows):
    assert rc.gn_form(P, C) == form
    _gn_run(device, f"gn {form} P={P} C={C} G={G} rows={rows}", rows, P, C, G)


@pytest.mark.parametrize("form", list(rc.GN_OFFSET))
def test_gn_silu_fwd_offset_inputs(device, form):
    """mean 8, standard deviation 0.5: a one-pass variance would lose these (the two-pass one must not)"""
    P, C, G = rc.GN_OFFSET[form]
    _gn_run(device, f"gn offset {form} P={P} C={C} G={G} rows=67", 67, P, C, G, offset=True)


_GN_SQUARE = [(P, C, G) for form, P, C, G in _GN if form != "general" and int(P ** 0.5) ** 2 == P]


@pytest.mark.parametrize("rows", rc.GN_ROWS)
@pytest.mark.parametrize("P,C,G", _GN_SQUARE)
def test_gn_silu_fwd_im2col(device, P, C, G, rows):
    lib, check = _lib()
    hin = int(P ** 0.5)
    hout = (hin - 1) // 2 + 1
    z, act, stats, zd, gd, bd = _gn_operands(device, rows, P, C, G, False)
    want = rc.im2col(act, hin)
    ldk, ldo = 9 * C + 4, P * C + 12
    tag = f"gn im2col P={P} C={C} G={G} rows={rows}"
    runs = []
    for with_out in (False, True):  # the episode's call (cols only), then both outputs
        cols = Buf(device, rows * hout * hout, ldk)
        cols.view.zero_()
        out, st = Buf(device, rows, ldo), Buf(device, rows, 2 * G)
        check(lib.marl_gn_silu_fwd(zd.ptr, gd.ptr, bd.ptr, out.ptr if with_out else None, ldo, 0, st.ptr, rows, P, C, G,
                                   cols.ptr, ldk, hin, None))
        th.cuda.synchronize()
        t = f"{tag} out={int(with_out)}"
        assert guards_intact(cols.whole, 0, cols.rows * ldk * 4), f"{t}: wrote outside cols"
        got = cols.cols(9 * C)
        assert th.equal(cols.view[:, 9 * C:].cpu(), th.zeros(cols.rows, 4)), f"{t}: the spare columns are not zero"
        assert bool((got[want == 0] == 0).all()), f"{t}: a padding tap was written"
        REC.fwd(f"{t} cols", got, want)
        REC.fwd(f"{t} rstd", st.cols(2 * G).reshape(rows, G, 2)[..., 1], stats[..., 1])
        if with_out:
            out.intact_beyond(P * C, t)
            REC.fwd(f"{t} out", out.cols(P * C), act.permute(0, 2, 1).reshape(rows, -1))
        else:
            out.unchanged(t)
        runs.append(got)
    assert th.equal(_bits(runs[0]), _bits(runs[1])), f"{tag}: cols differ between the two calls"


# ======================================================================================================================
# LayerNorm + SiLU forward with the fused one-output dot
# ======================================================================================================================
def _ln_run(device, tag, m, n, dot, offset=False):
    lib, check = _lib()
    z = rc.norm_input((m, n), seed=1000 * m + n, offset=offset)
    gamma, beta = rc.affine(n, n)
    g = th.Generator().manual_seed(n + m)
    w, b = th.randn(n, generator=g), th.randn(1, generator=g)
    act, stats = rc.ln_silu(z.double(), gamma.double(), beta.double())
    ldz, ldo = n + 4, n + 8
    zd, gd, bd, wd, b1 = Buf(device, m, ldz, z), _vec(device, gamma), _vec(device, beta), _vec(device, w), _vec(device, b)
    out, st, dd = Buf(device, m, ldo), Buf(device, m, 2), Buf(device, 1, m)
    check(lib.marl_ln_silu_dot_fwd(zd.ptr, ldz, gd.ptr, bd.ptr, out.ptr, ldo, st.ptr, m, n, wd.ptr if dot else None,
                                   b1.ptr if dot else None, dd.ptr if dot else None, None))
    th.cuda.synchronize()
    out.intact_beyond(n, tag)
    st.intact_beyond(2, tag)
    REC.fwd(f"{tag} out", out.cols(n), act)
    REC.fwd(f"{tag} mean", st.cols(2)[:, 0], stats[:, 0])
    REC.fwd(f"{tag} rstd", st.cols(2)[:, 1], stats[:, 1])
    if dot:
        dd.intact_beyond(m, tag)
        REC.fwd(f"{tag} dot", dd.cols(m)[0], act @ w.double() + b.double())
    else:
        dd.unchanged(tag)


@pytest.mark.parametrize("n", rc.LN_N_REG + rc.LN_N_GENERAL)
def test_ln_silu_dot_fwd(device, n):
    for m in rc.LN_M:  # (a wave owns rows r and r + ceil(m / 2): odd m leaves the last wave one row)
        _ln_run(device, f"ln n={n} m={m}", m, n, dot=n <= 384)
    if n <= 384:       # the same kernels without the dot
        _ln_run(device, f"ln n={n} m=9 nodot", 9, n, dot=False)


@pytest.mark.parametrize("n", rc.LN_OFFSET_N)
def test_ln_silu_dot_fwd_offset_inputs(device, n):
    _ln_run(device, f"ln offset n={n} m=67", 67, n, dot=n <= 384, offset=True)


# ======================================================================================================================
# position embedding
# ======================================================================================================================
@pytest.mark.parametrize("rows", rc.POS_ROWS)
@pytest.mark.parametrize("nd", rc.POS_ND)
def test_pos_embed_fwd(device, nd, rows):
    lib, check = _lib()
    H, W = rc.POS_HW
    g = th.Generator().manual_seed(100 * nd + rows)
    pos = th.stack([th.randint(0, H, (rows,), generator=g), th.randint(0, W, (rows,), generator=g)], 1).int()
    wt, b = th.randn(nd, 2, generator=g), th.randn(nd, generator=g) * 0.5
    gamma, beta = rc.affine(nd, nd)
    w4 = th.full((nd, 4), float("nan"))
    w4[:, :2] = wt
    wd, bd, gd, btd = Buf(device, nd, 4, w4), _vec(device, b), _vec(device, gamma), _vec(device, beta)
    ldz, ldo = nd + 3, nd + 5
    for given in (False, True):
        npos = th.rand(rows, 2, generator=g) if given else None
        p64 = npos.double() if given else pos.double() / th.tensor([H, W], dtype=th.float64)
        z64 = p64 @ wt.double().t() + b.double()
        act, stats = rc.ln_silu(z64, gamma.double(), beta.double())
        pd = Buf(device, rows, 2, pos, dtype=th.int32)
        nd_in = Buf(device, rows, 2, npos) if given else None
        for extras in (True, False):
            tag = f"pos nd={nd} rows={rows} given={int(given)} extras={int(extras)}"
            n4, st = Buf(device, rows, 4), Buf(device, rows, 2)
            z, out = Buf(device, rows, ldz), Buf(device, rows, ldo)
            check(lib.marl_pos_embed_fwd(None if given else pd.ptr, nd_in.ptr if given else None, H, W, wd.ptr, bd.ptr,
                                         gd.ptr, btd.ptr, n4.ptr if extras else None, z.ptr, ldz,
                                         st.ptr if extras else None, out.ptr, ldo, rows, nd, None))
            th.cuda.synchronize()
            z.intact_beyond(nd, tag)
            out.intact_beyond(nd, tag)
            REC.fwd(f"{tag} z", z.cols(nd), z64)
            REC.fwd(f"{tag} out", out.cols(nd), act)
            assert th.isfinite(out.cols(nd)).all(), f"{tag}: the NaN columns of the packed weight were read"
            if nd == 1:
                REC.fwd(f"{tag} silu(beta)", out.cols(1), F.silu(beta.double()).expand(rows, 1))
            if extras:
                n4.intact_beyond(2, tag)
                st.intact_beyond(2, tag)
                REC.fwd(f"{tag} npos", n4.cols(2), p64)
                REC.fwd(f"{tag} mean", st.cols(2)[:, 0], stats[:, 0])
                REC.fwd(f"{tag} rstd", st.cols(2)[:, 1], stats[:, 1])
            else:
                n4.unchanged(tag)
                st.unchanged(tag)


# ======================================================================================================================
# LSTM cell backward
# ======================================================================================================================
class Cell:
    """one cell's device operands; ldg_pad: extra floats of the gates' leading dimension"""

    def __init__(self, device, x, ldg_pad=4, ld_pad=4, image_row0=None):
        n, rows = x.n, x.rows
        self.x, self.n = x, n
        self.dh, self.dc = Buf(device, rows, n + ld_pad, x.dh), Buf(device, rows, n + ld_pad, x.dc)
        self.gates = Buf(device, rows, 4 * n + ldg_pad, x.gates)
        self.cp, self.cn = Buf(device, rows, n + ld_pad, x.c_prev), Buf(device, rows, n + ld_pad, x.c_new)
        self.row0, self.steps, self.img = image_row0, rc_steps(n), None
        if image_row0 is not None:
            self.img_bytes = im.image_bytes(rows + image_row0, 16 * self.steps)
            self.img_whole, self.img = guarded((self.img_bytes,), th.uint8, device)

    def check(self, tag, skipped=False):
        n = self.n
        ref_g, ref_dc = rc.cell_bwd_formulas(self.x.gates, self.x.c_prev, self.x.c_new, self.x.dh, self.x.dc)
        self.gates.intact_beyond(4 * n, tag)
        self.dc.intact_beyond(n, tag)
        for b in (self.dh, self.cp, self.cn):
            b.unchanged(tag)
        if skipped:
            assert th.equal(_bits(self.gates.cols(4 * n)), _bits(self.x.gates)), f"{tag}: skip_f32 wrote the gates"
        else:
            got = self.gates.cols(4 * n)
            for k, name in enumerate("ifgo"):
                REC.grad(f"{tag} d{name}", got[:, k * n:(k + 1) * n], ref_g[:, k * n:(k + 1) * n])
        REC.grad(f"{tag} dc", self.dc.cols(n), ref_dc)


def rc_steps(n):
    return -(-4 * n // 16)


def _cell_launch(cells, rows, skip=False):
    lib, _ = _lib()
    cnt = len(cells)
    vp, ia = (C.c_void_p * cnt), (C.c_int * cnt)
    imgs = any(c.img is not None for c in cells)
    return lib.marl_lstm_cell_bwd(
        cnt, vp(*[c.dh.ptr for c in cells]), vp(*[c.dc.ptr for c in cells]), vp(*[c.gates.ptr for c in cells]),
        vp(*[c.cp.ptr for c in cells]), vp(*[c.cn.ptr for c in cells]), ia(*[c.dh.ld for c in cells]),
        ia(*[c.dc.ld for c in cells]), ia(*[c.gates.ld for c in cells]), ia(*[c.cp.ld for c in cells]),
        ia(*[c.n for c in cells]),
        vp(*[None if c.img is None else c.img.data_ptr() for c in cells]) if imgs else None,
        ia(*[c.row0 or 0 for c in cells]) if imgs else None, ia(*[c.steps for c in cells]) if imgs else None,
        ia(*[int(skip)] * cnt) if imgs else None, rows, None)


@pytest.mark.parametrize("rows", rc.CELL_ROWS)
@pytest.mark.parametrize("n", rc.CELL_N_VEC4 + [rc.CELL_N_SCALAR])
def test_lstm_cell_bwd(device, n, rows):
    _, check = _lib()
    cell = Cell(device, rc.CellInputs(rows, n, seed=10 * n + rows), ldg_pad=4 if n % 4 == 0 else 3,
                ld_pad=4 if n % 4 == 0 else 1)
    check(_cell_launch([cell], rows))
    th.cuda.synchronize()
    cell.check(f"cell n={n} rows={rows}")


@pytest.mark.parametrize("rows", rc.CELL_ROWS)
def test_lstm_cell_bwd_scalar_form_has_the_four_wide_bits(device, rows):
    """n = 20 with ldg = 4 n + 1 takes the scalar form: same arithmetic, same bits"""
    _, check = _lib()
    x = rc.CellInputs(rows, 20, seed=rows)
    wide, scalar = Cell(device, x), Cell(device, x, ldg_pad=1)
    check(_cell_launch([wide], rows))
    check(_cell_launch([scalar], rows))
    th.cuda.synchronize()
    scalar.check(f"cell n=20 ldg=81 rows={rows}")
    assert th.equal(_bits(wide.gates.cols(80)), _bits(scalar.gates.cols(80))), "the gate gradients differ in bits"
    assert th.equal(_bits(wide.dc.cols(20)), _bits(scalar.dc.cols(20))), "dc differs in bits"


@pytest.mark.parametrize("rows", rc.CELL_ROWS)
@pytest.mark.parametrize("pair", rc.CELL_PAIRS)
def test_lstm_cell_bwd_two_cells(device, pair, rows):
    """(64, 20): the grid is sized by the wider cell, whichever comes first; (20, 23): both go scalar"""
    _, check = _lib()
    for order in (pair, pair[::-1]):
        cells = [Cell(device, rc.CellInputs(rows, n, seed=7 * n + rows), ldg_pad=4 if n % 4 == 0 else 3,
                      ld_pad=4 if n % 4 == 0 else 1) for n in order]
        check(_cell_launch(cells, rows))
        th.cuda.synchronize()
        for c in cells:
            c.check(f"cells {order} n={c.n} rows={rows}")


def test_lstm_cell_bwd_saturated(device):
    _, check = _lib()
    for n in (20, 23):
        x = rc.CellInputs(65, n, seed=n, saturated=True)
        cell = Cell(device, x, ldg_pad=4 if n % 4 == 0 else 3)
        check(_cell_launch([cell], 65))
        th.cuda.synchronize()
        got, dc = cell.gates.cols(4 * n), cell.dc.cols(n)
        assert th.isfinite(got).all() and th.isfinite(dc).all(), f"n={n}: NaN / Inf from saturated gates"
        worst = got.abs().max().item()
        REC.put(f"cell saturated n={n}", {"max_abs_gate_gradient": worst, "bound": rc.saturated_bound(x)})
        assert worst <= rc.saturated_bound(x), (n, worst)
        cell.check(f"cell saturated n={n}")


@pytest.mark.parametrize("row0", [0, 37])
@pytest.mark.parametrize("n", rc.CELL_N_VEC4)
def test_lstm_cell_bwd_gate_gradient_image(device, n, row0):
    _, check = _lib()
    for rows in rc.CELL_ROWS:
        x = rc.CellInputs(rows, n, seed=10 * n + rows)
        tag = f"cell image n={n} rows={rows} row0={row0}"
        cell = Cell(device, x, image_row0=row0)
        check(_cell_launch([cell], rows))
        th.cuda.synchronize()
        cell.check(tag)
        assert guards_intact(cell.img_whole, 0, cell.img_bytes), f"{tag}: wrote outside the image"
        want = np.full(cell.img_bytes, SENTINEL, dtype=np.uint8)
        im.place(want, cell.gates.cols(4 * n).numpy(), row0=row0, steps=cell.steps)
        got = cell.img.cpu().numpy()
        assert np.array_equal(got, want), f"{tag}: the image differs from the host model of the fp32 gradients"
        # skip_f32: the gates keep the activations; dc and the image are the same bits
        skip = Cell(device, x, image_row0=row0)
        check(_cell_launch([skip], rows, skip=True))
        th.cuda.synchronize()
        skip.check(f"{tag} skip_f32", skipped=True)
        assert np.array_equal(skip.img.cpu().numpy(), got), f"{tag}: skip_f32 changed the image"
        assert th.equal(_bits(skip.dc.cols(n)), _bits(cell.dc.cols(n))), f"{tag}: skip_f32 changed dc"
        assert guards_intact(skip.img_whole, 0, skip.img_bytes)
    REC.put(f"cell image n={n} row0={row0}", {"image_equals_the_host_model": True})


def test_lstm_cell_bwd_two_cells_with_images(device):
    _, check = _lib()
    rows = 65
    cells = [Cell(device, rc.CellInputs(rows, n, seed=n), image_row0=r0) for n, r0 in ((64, 37), (20, 0))]
    check(_cell_launch(cells, rows))
    th.cuda.synchronize()
    for c in cells:
        c.check(f"cells image n={c.n}")
        want = np.full(c.img_bytes, SENTINEL, dtype=np.uint8)
        im.place(want, c.gates.cols(4 * c.n).numpy(), row0=c.row0, steps=c.steps)
        assert np.array_equal(c.img.cpu().numpy(), want), f"n={c.n}: image"


# ======================================================================================================================
# policy logit gradients
# ======================================================================================================================
def _dlogits(device, form, x, dlogp, dprobs, layout, inv_tau=1.0, keep=1.0, floor=0.0, probs=None):
    """one call; layout "aligned" | "ld" (ld = nA + 1) | "offset" (probs one float off a 16-byte boundary)"""
    lib, check = _lib()
    rows, nA = x.rows, x.n_actions
    ld = nA + 1 if layout == "ld" else (nA + 3) // 4 * 4 + 4
    p = (x.probs if probs is None else probs).reshape(1, -1)
    pd = Buf(device, 1, rows * nA, p, offset=4 if layout == "offset" else 0)
    assert pd.ptr % 16 == (4 if layout == "offset" else 0)
    gd = _vec(device, dprobs) if dprobs is not None else None
    ld_ = _vec(device, dlogp) if dlogp is not None else None
    ad = Buf(device, 1, rows, x.actions.reshape(1, -1), dtype=th.int32)
    out = Buf(device, rows, ld)
    check(lib.marl_policy_dlogits(form, ld_.ptr if ld_ else None, gd.ptr if gd else None, pd.ptr, ad.ptr, out.ptr, ld,
                                  rows, nA, inv_tau, keep, floor, None))
    th.cuda.synchronize()
    out.intact_beyond(nA, f"dlogits form={form} nA={nA} rows={rows} {layout}")
    for b in (pd, ad):
        b.unchanged("dlogits inputs")
    return out.cols(nA)


def _layouts(nA):
    return ("aligned", "ld", "offset") if nA % 4 == 0 else ("aligned",)


def _same_bits(tag, runs):
    for name, got in runs.items():
        assert th.equal(_bits(got), _bits(runs["aligned"])), f"{tag}: the {name} run differs from the aligned one in bits"


@pytest.mark.parametrize("rows", rc.POLICY_ROWS)
@pytest.mark.parametrize("nA", rc.POLICY_NA)
def test_policy_dlogits_plain_and_probs(device, nA, rows):
    x = rc.PolicyInputs(rows, nA, seed=100 * nA + rows)
    for dlogp in (x.dlogp, None):
        tag = f"dlogits form=0 nA={nA} rows={rows} dlogp={int(dlogp is not None)}"
        runs = {lay: _dlogits(device, 0, x, dlogp, None, lay) for lay in _layouts(nA)}
        REC.grad(tag, runs["aligned"], rc.dlogits_plain(x.probs, x.actions, dlogp))
        _same_bits(tag, runs)
        tag = f"dlogits form=1 nA={nA} rows={rows} dlogp={int(dlogp is not None)}"
        runs = {lay: _dlogits(device, 1, x, dlogp, x.dprobs, lay) for lay in _layouts(nA)}
        REC.grad(tag, runs["aligned"], rc.dlogits_probs(x.probs, x.actions, dlogp, x.dprobs))
        _same_bits(tag, runs)


@pytest.mark.parametrize("tau", rc.EXPLORE_TAU)
@pytest.mark.parametrize("nA", rc.POLICY_NA)
def test_policy_dlogits_explore(device, nA, tau):
    for rows in rc.POLICY_ROWS:
        x = rc.PolicyInputs(rows, nA, seed=100 * nA + rows, tau=tau, eps=rc.EXPLORE_EPS)
        for dlogp, dprobs in ((x.dlogp, x.dprobs), (x.dlogp, None), (None, x.dprobs), (None, None)):
            tag = (f"dlogits form=2 nA={nA} rows={rows} tau={tau} dlogp={int(dlogp is not None)} "
                   f"dprobs={int(dprobs is not None)}")
            runs = {lay: _dlogits(device, 2, x, dlogp, dprobs, lay, 1.0 / tau, x.keep, x.floor) for lay in _layouts(nA)}
            REC.grad(tag, runs["aligned"],
                     rc.dlogits_explore_autograd(x.logits, x.actions, dlogp, dprobs, tau, x.keep, x.floor))
            _same_bits(tag, runs)


@pytest.mark.parametrize("nA", [5, 8])
def test_policy_dlogits_explore_drops_the_log_prob_of_an_impossible_action(device, nA):
    """keep = 1, floor = 0 and a forced action of probability exactly 0: its log-prob term is dropped (no 0 / 0)"""
    rows = 257
    x = rc.PolicyInputs(rows, nA, seed=nA)
    logits = x.logits.clone()
    logits[th.arange(rows), x.actions.long()] = -float("inf")
    probs = th.softmax(logits, -1).float()
    assert bool((probs[th.arange(rows), x.actions.long()] == 0).all())
    for lay in _layouts(nA):
        got = _dlogits(device, 2, x, x.dlogp, x.dprobs, lay, probs=probs)
        assert th.isfinite(got).all(), "NaN / Inf from an action of probability 0"
        assert bool((got[th.arange(rows), x.actions.long()] == 0).all())
        REC.grad(f"dlogits form=2 nA={nA} impossible action {lay}", got,
                 rc.dlogits_explore_formula(probs, x.actions, None, x.dprobs, 1.0, 1.0, 0.0))


# ======================================================================================================================
# row dot and message mean
# ======================================================================================================================
@pytest.mark.parametrize("n", rc.ROWDOT_N)
def test_rowdot(device, n):
    lib, check = _lib()
    for rows in rc.ROWDOT_ROWS:
        g = th.Generator().manual_seed(10 * n + rows)
        a, w, b = th.randn(rows, n, generator=g), th.randn(n, generator=g), th.randn(1, generator=g)
        ad, wd, bd, out = Buf(device, rows, n + 3, a), _vec(device, w), _vec(device, b), Buf(device, 1, rows)
        check(lib.marl_rowdot(ad.ptr, n + 3, wd.ptr, bd.ptr, out.ptr, rows, n, None))
        th.cuda.synchronize()
        out.intact_beyond(rows, f"rowdot n={n} rows={rows}")
        REC.fwd(f"rowdot n={n} rows={rows}", out.cols(rows)[0], a.double() @ w.double() + b.double())


@pytest.mark.parametrize("n", rc.AGG_N)
@pytest.mark.parametrize("na", rc.AGG_NA)
def test_agg_msg(device, na, n):
    lib, check = _lib()
    for nb in rc.AGG_NB:
        tag = f"agg na={na} nb={nb} n={n}"
        m = th.randn(na * nb, n, generator=th.Generator().manual_seed(100 * na + 10 * nb + n))
        ld = n + 3
        src, out, inplace = Buf(device, na * nb, ld, m), Buf(device, na * nb, ld), Buf(device, na * nb, ld, m)
        check(lib.marl_agg_msg(src.ptr, out.ptr, ld, na, nb, n, None))
        check(lib.marl_agg_msg(inplace.ptr, inplace.ptr, ld, na, nb, n, None))  # the backward driver's call
        th.cuda.synchronize()
        out.intact_beyond(n, tag)
        inplace.intact_beyond(n, tag)
        src.unchanged(tag)
        REC.fwd(tag, out.cols(n), rc.agg_msg(m, na, nb))
        assert th.equal(_bits(out.cols(n)), _bits(inplace.cols(n))), f"{tag}: in place differs"
        if na == 1:
            assert th.equal(out.cols(n), th.zeros(nb, n)), f"{tag}: one agent must give zeros"


# ======================================================================================================================
# refusals: the documented code, and nothing written
# ======================================================================================================================
def _refused(call, code, bufs, what):
    lib, _ = _lib()
    assert call() == code, what
    assert lib.marl_last_error(), what
    th.cuda.synchronize()
    for b in bufs:
        b.unchanged(what)


def test_gn_silu_fwd_refusals(device):
    lib, _ = _lib()
    rows, P, C, G = 5, 9, 16, 4
    z, g, b = Buf(device, rows, P * C), Buf(device, 1, C), Buf(device, 1, C)
    out, st, cols = Buf(device, rows, P * C), Buf(device, rows, 2 * G), Buf(device, rows * 4, 9 * C + 4)
    bufs = [out, st, cols]

    def call(z=z.ptr, g=g.ptr, b=b.ptr, out=out.ptr, ldo=P * C, rows=rows, P=P, C=C, G=G, cols=None, ldk=0, hin=0):
        return lambda: lib.marl_gn_silu_fwd(z, g, b, out, ldo, 0, st.ptr, rows, P, C, G, cols, ldk, hin, None)

    for kw in (dict(z=None), dict(g=None), dict(b=None), dict(out=None), dict(rows=-1), dict(P=0), dict(C=0), dict(G=0),
               dict(G=3), dict(ldo=P * C - 1), dict(cols=cols.ptr, ldk=9 * C - 1, hin=3),
               dict(cols=cols.ptr, ldk=9 * C + 4, hin=2), dict(cols=cols.ptr, ldk=9 * C + 4, hin=0)):
        _refused(call(**kw), EINVAL, bufs, f"gn {kw}")
    # a cols request on a general-form shape: a channel count that is no power of two, a row longer than 1024
    big = Buf(device, 4, 9 * 32 + 4)
    _refused(call(C=24, G=3, cols=cols.ptr, ldk=9 * 24 + 4, hin=3, ldo=9 * 24), ELIMIT, bufs, "gn cols C=24")
    _refused(call(P=36, C=32, G=4, cols=big.ptr, ldk=9 * 32 + 4, hin=6, ldo=36 * 32), ELIMIT, bufs + [big], "gn cols 1152")
    _refused(call(C=24, G=3, out=None, ldo=9 * 24), EINVAL, bufs, "gn no output")
    assert call(rows=0)() == 0
    th.cuda.synchronize()
    for bf in bufs:
        bf.unchanged("gn rows = 0")


def test_ln_silu_dot_fwd_refusals(device):
    lib, _ = _lib()
    m, n = 5, 400
    z, g, b, w = Buf(device, m, n), Buf(device, 1, n), Buf(device, 1, n), Buf(device, 1, n)
    out, st, dot = Buf(device, m, n), Buf(device, m, 2), Buf(device, 1, m)
    bufs = [out, st, dot]

    def call(z=z.ptr, g=g.ptr, b=b.ptr, out=out.ptr, ldz=n, ldo=n, m=m, n=64, w=w.ptr, bd=b.ptr, dot=dot.ptr):
        return lambda: lib.marl_ln_silu_dot_fwd(z, ldz, g, b, out, ldo, st.ptr, m, n, w, bd, dot, None)

    for kw in (dict(z=None), dict(g=None), dict(b=None), dict(out=None), dict(m=-1), dict(n=0), dict(ldz=63),
               dict(ldo=63), dict(bd=None), dict(dot=None)):
        _refused(call(**kw), EINVAL, bufs, f"ln {kw}")
    for wide in (385, 400, 1000):  # the general kernel has no dot
        _refused(call(n=wide, ldz=1000, ldo=1000), ELIMIT, bufs, f"ln dot n={wide}")
    assert call(m=0)() == 0
    th.cuda.synchronize()
    for bf in bufs:
        bf.unchanged("ln m = 0")


def test_pos_embed_fwd_refusals(device):
    lib, _ = _lib()
    rows, nd = 5, 8
    pos, npos = Buf(device, rows, 2, th.zeros(rows, 2).int(), dtype=th.int32), Buf(device, rows, 2, th.zeros(rows, 2))
    w, v = Buf(device, nd, 4), Buf(device, 1, nd)
    n4, z, st, out = Buf(device, rows, 4), Buf(device, rows, nd), Buf(device, rows, 2), Buf(device, rows, nd)
    bufs = [n4, z, st, out]

    def call(pos=pos.ptr, npos=None, h=28, wd=36, w=w.ptr, b=v.ptr, g=v.ptr, bt=v.ptr, z=z.ptr, ldz=nd, out=out.ptr,
             ldo=nd, rows=rows, nd=nd):
        return lambda: lib.marl_pos_embed_fwd(pos, npos, h, wd, w, b, g, bt, n4.ptr, z, ldz, st.ptr, out, ldo, rows, nd,
                                              None)

    for kw in (dict(pos=None), dict(h=0), dict(wd=-3), dict(w=None), dict(b=None), dict(g=None), dict(bt=None),
               dict(z=None), dict(out=None), dict(rows=-1), dict(nd=0), dict(ldz=nd - 1), dict(ldo=nd - 1)):
        _refused(call(**kw), EINVAL, bufs, f"pos {kw}")
    assert call(rows=0)() == 0 and call(pos=None, npos=npos.ptr, h=0, wd=0, rows=0)() == 0
    th.cuda.synchronize()
    for bf in bufs:
        bf.unchanged("pos rows = 0")


def test_lstm_cell_bwd_refusals(device):
    lib, _ = _lib()
    rows = 3
    x20, x23 = rc.CellInputs(rows, 20, seed=1), rc.CellInputs(rows, 23, seed=2)

    def untouched(cells, what):
        th.cuda.synchronize()
        for c in cells:
            for b in (c.dh, c.dc, c.gates, c.cp, c.cn):
                b.unchanged(what)
            if c.img is not None:
                assert bool((c.img_whole == SENTINEL).all()), f"{what}: the image was written"

    # an image request that falls to the scalar form: an odd width, an odd leading dimension, a scalar partner
    for cells in ([Cell(device, x23, ldg_pad=4, image_row0=0)], [Cell(device, x20, ldg_pad=1, image_row0=0)],
                  [Cell(device, x20, image_row0=0), Cell(device, x23, ldg_pad=3)]):
        assert _cell_launch(cells, rows) == EINVAL and lib.marl_last_error()
        untouched(cells, "cell image on the scalar form")
    cell = Cell(device, x20, image_row0=0)
    vp, ia = C.c_void_p * 1, C.c_int * 1

    def call(count=1, dh=cell.dh.ptr, dc=cell.dc.ptr, gates=cell.gates.ptr, cp=cell.cp.ptr, cn=cell.cn.ptr, lddh=24,
             lddc=24, ldg=84, ldc=24, n=20, img=cell.img.data_ptr(), row0=0, steps=5, skip=0, rows=rows):
        return lib.marl_lstm_cell_bwd(count, vp(dh), vp(dc), vp(gates), vp(cp), vp(cn), ia(lddh), ia(lddc), ia(ldg),
                                      ia(ldc), ia(n), vp(img), ia(row0), ia(steps), ia(skip), rows, None)

    for kw in (dict(count=0), dict(count=3), dict(dh=None), dict(dc=None), dict(gates=None), dict(cp=None), dict(cn=None),
               dict(lddh=19), dict(lddc=19), dict(ldc=19), dict(ldg=79), dict(n=0), dict(n=-4), dict(rows=-1),
               dict(steps=4), dict(row0=-1), dict(img=cell.img.data_ptr() + 8), dict(img=None, skip=1),
               dict(dh=cell.dh.ptr + 4), dict(gates=cell.gates.ptr + 8)):
        assert call(**kw) == EINVAL and lib.marl_last_error(), kw
        untouched([cell], f"cell {kw}")
    assert lib.marl_lstm_cell_bwd(1, None, None, None, None, None, None, None, None, None, None, None, None, None, None,
                                  rows, None) == EINVAL
    assert call(rows=0) == 0
    untouched([cell], "cell rows = 0")


def test_policy_dlogits_refusals(device):
    lib, _ = _lib()
    rows, nA = 5, 4
    f, a, out = Buf(device, rows, 20), Buf(device, 1, rows, th.zeros(1, rows).int(), dtype=th.int32), Buf(device, rows, 20)

    def call(form=1, dlogp=f.ptr, dprobs=f.ptr, probs=f.ptr, actions=a.ptr, out=out.ptr, ld=nA, rows=rows, nA=nA,
             inv_tau=1.0, keep=0.75, floor=0.0625):
        return lambda: lib.marl_policy_dlogits(form, dlogp, dprobs, probs, actions, out, ld, rows, nA, inv_tau, keep, floor,
                                               None)

    for kw in (dict(form=-1), dict(form=3), dict(probs=None), dict(out=None), dict(rows=-1), dict(nA=0), dict(ld=nA - 1),
               dict(form=1, dprobs=None), dict(form=0, actions=None), dict(form=1, actions=None),
               dict(form=2, actions=None), dict(form=2, keep=0.0), dict(form=2, inv_tau=0.0), dict(form=2, floor=-0.1),
               dict(form=2, keep=float("nan"))):
        _refused(call(**kw), EINVAL, [out], f"dlogits {kw}")
    for form in (0, 1, 2):  # more actions than the library's maximum
        _refused(call(form=form, nA=17, ld=20), ELIMIT, [out], f"dlogits form={form} nA=17")
    assert call(rows=0)() == 0
    th.cuda.synchronize()
    out.unchanged("dlogits rows = 0")


def test_rowdot_and_agg_msg_refusals(device):
    lib, _ = _lib()
    a, w, out = Buf(device, 4, 16), Buf(device, 1, 16), Buf(device, 4, 16)
    for args in ((None, 16, w.ptr, w.ptr, out.ptr, 4, 16), (a.ptr, 16, None, w.ptr, out.ptr, 4, 16),
                 (a.ptr, 16, w.ptr, None, out.ptr, 4, 16), (a.ptr, 16, w.ptr, w.ptr, None, 4, 16),
                 (a.ptr, 16, w.ptr, w.ptr, out.ptr, -1, 16), (a.ptr, 16, w.ptr, w.ptr, out.ptr, 4, 0),
                 (a.ptr, 15, w.ptr, w.ptr, out.ptr, 4, 16)):
        _refused(lambda: lib.marl_rowdot(*args, None), EINVAL, [out], f"rowdot {args[1:]}")
    for args in ((None, out.ptr, 16, 2, 2, 16), (a.ptr, None, 16, 2, 2, 16), (a.ptr, out.ptr, 15, 2, 2, 16),
                 (a.ptr, out.ptr, 16, 0, 2, 16), (a.ptr, out.ptr, 16, 2, -1, 16), (a.ptr, out.ptr, 16, 2, 2, 0)):
        _refused(lambda: lib.marl_agg_msg(*args, None), EINVAL, [out], f"agg {args[2:]}")
    assert lib.marl_rowdot(a.ptr, 16, w.ptr, w.ptr, out.ptr, 0, 16, None) == 0
    assert lib.marl_agg_msg(a.ptr, out.ptr, 16, 2, 0, 16, None) == 0
    th.cuda.synchronize()
    out.unchanged("rows = 0")
