"""CPU: the definition of the resampling batch gather (``warp.reference_apply``), the matrices of the ``augment`` views
(``warp.from_ops``, ``warp.compose_ops``), the new tokens of the spec grammar and ``Policy.draw_warp`` /
``Policy.warp_views``.  The GPU kernel is held to this definition bit for bit in test_gpu_warp.py."""
import math
import re

import pytest
import torch as th
import torch.nn.functional as F

from marlclassification_amd import augment, warp
from tests.buffers import same_bits as _same_bits

ONE = warp.ONE
VIEW_SHAPES = [(1, 5, 7), (3, 16, 16), (3, 33, 33), (1, 1, 1), (2, 9, 4)]
FILL = {th.uint8: 200, th.float32: -1.5}


def _images(n, shape, dtype, seed=0):
    g = th.Generator().manual_seed(seed + 7 * shape[1] + shape[2])
    if dtype == th.uint8:
        return th.randint(0, 256, (n,) + tuple(shape), dtype=th.uint8, generator=g)
    return th.randn((n,) + tuple(shape), generator=g)


def _view_ops(h, w):
    codes = range(8) if h == w else (0, 2, 4, 6)
    shifts = ((0, 0), (1, -2), (h - 1, w - 1), (-(h - 1), -(w - 1)), (-(h - 1), 1), (h + 5, -(w + 5)))
    return th.tensor([[d, dy, dx, 0, 0, 0, 0, 0] for d in codes for dy, dx in shifts], dtype=th.int32)


# ---- three consequences of the definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", VIEW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_identity_matrix_is_a_plain_gather(shape, dtype):
    src = _images(6, shape, dtype)
    rows = th.tensor([5, 0, 3, 3])
    for mode in ("reflect", "zero"):
        assert _same_bits(warp.reference_apply(src, rows, warp.identity(4), None, mode, FILL[dtype]), src[rows])
    assert _same_bits(warp.reference_apply(src, None, warp.identity(6)), src)


@pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", VIEW_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_augment_view_is_a_matrix_of_signed_units(shape, dtype):
    c, h, w = shape
    src = _images(6, shape, dtype)
    ops = _view_ops(h, w)
    rows = th.randint(0, 6, (ops.shape[0],), generator=th.Generator().manual_seed(1))
    mats = warp.from_ops(ops, h, w)
    assert mats.dtype == th.int32 and set(mats[:, :4].abs().flatten().tolist()) <= {0, ONE}
    assert bool((mats[:, 4:6] % (2 * ONE) == 0).all()) and not mats[:, 6:].any()
    for mode in ("reflect", "zero"):
        want = augment.reference_apply(src, rows, ops, mode, FILL[dtype])
        assert _same_bits(warp.reference_apply(src, rows, mats, None, mode, FILL[dtype]), want), mode
        # ... and handed over as ops they are folded into the matrices
        assert _same_bits(warp.reference_apply(src, rows, warp.identity(ops.shape[0]), ops, mode, FILL[dtype]), want)


def test_from_ops_refuses_a_transposing_code_on_non_square_images():
    with pytest.raises(ValueError, match="square"):
        warp.from_ops(th.tensor([[3, 0, 0, 0, 0, 0, 0, 0]], dtype=th.int32), 5, 7)
    warp.from_ops(th.tensor([[3, 0, 0, 0, 0, 0, 0, 0]], dtype=th.int32), 7, 7)
    with pytest.raises(ValueError):
        warp.from_ops(th.zeros(2, 7, dtype=th.int32), 7, 7)


def test_against_grid_sample_within_the_weight_quantisation():
    """17 degrees, zoom 1.2, 3 x 32 x 32, data in [0, 1), zero padding.  A weight is off by at most 1/512 per axis, so
    the bound is 2/512 (max - min) = 3.9e-3 plus the rounding of the Q16 matrix, of order 2^-17 (H + W) / max(H, W);
    4.5e-3 holds both (2.2e-3 to 2.4e-3 is what comes out)."""
    g = th.Generator().manual_seed(0)
    src = th.rand(4, 3, 32, 32, generator=g)
    mats = warp.matrices(th.full((4,), 17.0), th.full((4,), 1.2), th.ones(4))
    got = warp.reference_apply(src, None, mats, None, "zero", 0.0)
    a = mats[:, :4].double() / ONE
    theta = th.zeros(4, 2, 3, dtype=th.float64)  # affine_grid works in (x, y): the matrix with both axes swapped
    theta[:, 0, 0], theta[:, 0, 1], theta[:, 1, 0], theta[:, 1, 1] = a[:, 3], a[:, 2], a[:, 1], a[:, 0]
    grid = F.affine_grid(theta.float(), (4, 3, 32, 32), align_corners=False)
    ref = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    err = (got - ref).abs().max().item()
    print(f"max |warp - grid_sample| = {err:.3e}")
    assert err <= 4.5e-3
    assert (got - src).abs().max().item() > 0.1  # (it did rotate)


# ---- known answers --------------------------------------------------------------------------------------------------
def test_a_half_pixel_shift_of_uint8_averages_neighbours_rounding_up():
    for a, b in ((10, 21), (0, 255), (254, 255), (7, 7), (1, 0)):
        src = th.tensor([[[[a, b]]]], dtype=th.uint8)
        m = warp.identity(1)
        m[0, 5] = ONE  # tx = one half pixel
        out = warp.reference_apply(src, None, m, None, "zero", 0)
        assert int(out[0, 0, 0, 0]) == (a + b + 1) >> 1
        assert int(out[0, 0, 0, 1]) == (b + 0 + 1) >> 1  # the tap past the edge is the fill
        assert int(warp.reference_apply(src, None, m, None, "reflect")[0, 0, 0, 1]) == (b + a + 1) >> 1
    src = th.tensor([[[[100, 200], [50, 150]]]], dtype=th.uint8)  # a quarter pixel in both axes: weights 192 / 64
    m = warp.identity(1)
    m[0, 4] = m[0, 5] = ONE // 2
    top, bot = 100 * 192 + 200 * 64, 50 * 192 + 150 * 64
    assert int(warp.reference_apply(src, None, m)[0, 0, 0, 0]) == (top * 192 + bot * 64 + 32768) >> 16


def test_a_zero_weight_is_skipped_not_multiplied():
    nan, inf = float("nan"), float("inf")
    src = th.tensor([[[[1.5, nan, 2.5], [inf, 4.0, nan]]]])
    out = warp.reference_apply(src, None, warp.identity(1), None, "zero", 0.0)  # fx == fy == 0: v00 alone
    assert th.equal(out.isnan(), src.isnan()) and out[0, 0, 0, 0] == 1.5 and out[0, 0, 1, 1] == 4.0
    m = warp.identity(1)
    m[0, 4] = ONE  # half a pixel down: fx == 0, the columns stay apart
    out = warp.reference_apply(src, None, m, None, "reflect")
    assert bool(out[0, 0, 0, 1].isnan()) and bool(out[0, 0, 0, 2].isnan()) and bool(out[0, 0, 0, 0].isinf())
    src = th.tensor([[[[1.5, nan], [3.0, nan]]]])
    assert warp.reference_apply(src, None, m, None, "reflect")[0, 0, 0, 0] == 2.25  # v01, v11 = NaN behind fx == 0
    # the blend is made of separately rounded products and sums
    g = th.Generator().manual_seed(2)
    src = th.randn(1, 1, 8, 8, generator=g)
    m = warp.identity(1)
    m[0, 4], m[0, 5] = 3 * ONE // 8, 5 * ONE // 8   # fy = 48, fx = 80
    out = warp.reference_apply(src, None, m, None, "reflect")
    wx, wy = th.tensor(80 / 256), th.tensor(48 / 256)
    v = src[0, 0]
    top = v[2, 3] * (1 - wx) + v[2, 4] * wx
    bot = v[3, 3] * (1 - wx) + v[3, 4] * wx
    assert out[0, 0, 2, 3] == top * (1 - wy) + bot * wy


# ---- compose_ops ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 16, 16), (2, 9, 4)], ids=["3x16x16", "2x9x4"])
def test_compose_ops_is_warp_then_view_exactly(shape):
    c, h, w = shape
    g = th.Generator().manual_seed(5)
    codes = list(range(8)) if h == w else [0, 2, 4, 6]
    ops = th.tensor([[d, dy, dx, 0, 0, 0, 0, 0] for d in codes for dy, dx in ((0, 0), (2, -1), (-3, 3))], dtype=th.int32)
    nb = ops.shape[0]
    u = th.rand(3, nb, generator=g)
    mats = warp.matrices(360 * u[0] - 180, 0.5 + u[1], 0.8 + 0.4 * u[2])
    mats[:, 4:6] = th.randint(-3 * ONE, 3 * ONE, (nb, 2), generator=g, dtype=th.int32)
    got = warp.compose_ops(mats, ops, h, w).to(th.int64)
    # in exact rational arithmetic: A = A_m A_v / 65536, t = A_m t_v / 65536 + t_m
    v, m = warp.from_ops(ops, h, w).to(th.int64), mats.to(th.int64)
    for b in range(nb):
        am, av = m[b, :4].view(2, 2), v[b, :4].view(2, 2)
        a = am @ av
        t = am @ v[b, 4:6]
        assert bool((a % ONE == 0).all()) and bool((t % ONE == 0).all())
        assert got[b, :4].tolist() == (a // ONE).flatten().tolist()
        assert got[b, 4:6].tolist() == (t // ONE + m[b, 4:6]).tolist() and not got[b, 6:].any()
    # the view of the warped image, pixel for pixel where the view reads inside the image (shifts 0: everywhere)
    src = _images(4, shape, th.uint8)
    flips = ops[::3]
    warped = warp.reference_apply(src, None, mats[:4])
    for k in range(flips.shape[0]):
        want = augment.reference_apply(warped, None, flips[k: k + 1].expand(4, -1))
        assert th.equal(warp.reference_apply(src, None, mats[:4], flips[k: k + 1].expand(4, -1)), want)
    assert th.equal(warp.compose_ops(mats, th.zeros(nb, 8, dtype=th.int32), h, w), mats)


# ---- sanitising -----------------------------------------------------------------------------------------------------
def test_hostile_matrices_and_rows_are_clamped():
    big = 2**31 - 1
    src = _images(5, (2, 9, 12), th.uint8)
    mats = th.tensor([[big, -big - 1, big, -big - 1, big, -big - 1, 3, 4],
                      [-big - 1, big, 0, big, -big - 1, big, 0, 0]], dtype=th.int32)
    clamped = th.tensor([[1 << 20, -(1 << 20), 1 << 20, -(1 << 20), 1 << 30, -(1 << 30), 0, 0],
                         [-(1 << 20), 1 << 20, 0, 1 << 20, -(1 << 30), 1 << 30, 0, 0]], dtype=th.int32)
    for mode in ("reflect", "zero"):
        got = warp.reference_apply(src, th.tensor([-7, 99]), mats, None, mode, 9)
        assert th.equal(got, warp.reference_apply(src, th.tensor([0, 4]), clamped, None, mode, 9))
    assert bool((warp.reference_apply(src, None, clamped, None, "zero", 9) == 9).all())  # 8192 pixels away
    ops = th.tensor([[0, 0, 0, -big - 1, -big - 1, big, big, 0], [0, 0, 0, 4, 5, -big - 1, 3, 0]], dtype=th.int32)
    got = warp.reference_apply(src, None, warp.identity(2), ops, "reflect", 9)
    assert not bool((got[0] == 9).all()) and th.equal(got[1], src[1])  # sums in 64 bits: two empty rectangles
    with pytest.raises(ValueError):
        warp.reference_apply(src, None, th.zeros(2, 6, dtype=th.int32))
    with pytest.raises(ValueError):
        warp.reference_apply(src, th.tensor([0]), warp.identity(2))
    with pytest.raises(ValueError, match="pad mode"):
        warp.reference_apply(src, None, warp.identity(2), None, "wrap")


def test_matrices_round_to_q16():
    m = warp.matrices(th.tensor([0.0, 90.0, 17.0]), th.tensor([1.0, 2.0, 1.2]), th.tensor([1.0, 1.0, 1.5]))
    assert m.dtype == th.int32 and m[0].tolist() == [ONE, 0, 0, ONE, 0, 0, 0, 0]
    assert m[1].tolist() == [0, -ONE // 2, ONE // 2, 0, 0, 0, 0, 0]
    t, s = math.radians(17.0), math.sqrt(1.5)
    want = [math.cos(t) * s / 1.2, -math.sin(t) / s / 1.2, math.sin(t) * s / 1.2, math.cos(t) / s / 1.2]
    assert all(abs(int(m[2, k]) - want[k] * ONE) <= 1.0 for k in range(4))


# ---- the grammar ----------------------------------------------------------------------------------------------------
def test_parse_the_new_tokens_and_their_defaults():
    p = augment.parse("d4,shift:2")
    assert (p.rotate, p.scale, p.stretch, p.zooms, p.has_warp) == (0.0, (1.0, 1.0), 1.0, (), False)
    p = augment.parse("rotate:15")
    assert p.rotate == 15.0 and p.has_warp and p.group() == (0,)
    p = augment.parse("hflip, rotate:180,scale:0.8:1.25 ,stretch:1.5,erase:4")
    assert (p.rotate, p.scale, p.stretch, p.hflip, p.erase) == (180.0, (0.8, 1.25), 1.5, True, 4) and p.has_warp
    assert augment.parse("scale:0.0625:16").scale == (1 / 16, 16.0) and augment.parse("stretch:4").stretch == 4.0
    assert not augment.parse("scale:1:1,stretch:1").has_warp and augment.parse("scale:2:2").has_warp
    p = augment.parse_tta("d4,zoom:0.8/1/1.25")
    assert p.zooms == (0.8, 1.0, 1.25) and p.has_warp and p.views().shape == (8, 8)
    assert augment.parse_tta("zoom:2").zooms == (2.0,) and not augment.parse_tta("hflip").has_warp


@pytest.mark.parametrize("bad", ["rotate", "rotate:0", "rotate:181", "rotate:-5", "rotate:x", "rotate:nan", "rotate:5:5",
                                 "scale:1", "scale:2:1", "scale:0.01:1", "scale:1:17", "scale:a:b", "scale:1:2:3",
                                 "scale:nan:1", "stretch", "stretch:0.5", "stretch:4.5", "stretch:r", "stretch:2:2",
                                 "zoom:1", "zoom:0.8/1.25", "zoom"])
def test_parse_names_the_bad_token(bad):
    with pytest.raises(ValueError, match=re.escape(f'"{bad}"')):
        augment.parse("hflip," + bad)


@pytest.mark.parametrize("bad", ["zoom:", "zoom:0", "zoom:1/", "zoom:1/x", "zoom:17", "zoom:1:2", "zoom:nan",
                                 "rotate:10", "scale:0.8:1.2", "stretch:2"])
def test_parse_tta_names_bad_zooms_and_refuses_the_random_tokens(bad):
    with pytest.raises(ValueError, match=re.escape(bad)):
        augment.parse_tta("d4," + bad)


def test_warp_views_are_the_codes_times_the_zooms():
    ops, mats = augment.parse_tta("rot90,zoom:0.5/1/4").warp_views()
    assert ops.dtype == mats.dtype == th.int32 and ops.shape == mats.shape == (12, 8)
    assert ops[:, 0].tolist() == [0, 3, 6, 5] * 3 and not ops[:, 1:].any()
    assert mats[:, 0].tolist() == [2 * ONE] * 4 + [ONE] * 4 + [ONE // 4] * 4
    assert th.equal(mats[:, 0], mats[:, 3]) and not mats[:, [1, 2, 4, 5, 6, 7]].any()
    ops, mats = augment.parse_tta("hflip").warp_views()  # no zoom: the views, under identity matrices
    assert th.equal(ops, augment.parse("hflip").views()) and th.equal(mats, warp.identity(2))


# ---- draw_warp ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", ["d4,shift:3,erase:4", "hflip", "shift:2", "erase:5:0.3"])
def test_draw_warp_leaves_the_sequence_of_draw_untouched(spec):
    warped = augment.parse(spec + ",rotate:20,scale:0.5:2,stretch:1.5")
    plain = augment.parse(spec)
    ga, gb = th.Generator().manual_seed(9), th.Generator().manual_seed(9)
    ops, mats = warped.draw_warp(64, ga, size=(32, 32))
    assert th.equal(ops, plain.draw(64, gb, size=(32, 32)))
    # without warp tokens draw_warp consumes what draw consumes, and its matrices are the identity
    ops2, mats2 = plain.draw_warp(64, gb, size=(32, 32))
    assert th.equal(mats2, warp.identity(64))
    gc = th.Generator().manual_seed(9)
    plain.draw(64, gc, size=(32, 32))
    assert th.equal(ops2, plain.draw(64, gc, size=(32, 32)))
    assert mats.dtype == th.int32 and mats.shape == (64, 8) and not mats[:, 4:].any()


def test_draw_warp_draws_inside_the_ranges():
    n = 4096
    _, m = augment.parse("rotate:30").draw_warp(n, th.Generator().manual_seed(1))
    a = m[:, :4].double() / ONE
    ang = th.rad2deg(th.atan2(a[:, 2], a[:, 0]))
    assert -30.01 <= ang.min() < -25 and 25 < ang.max() <= 30.01 and abs(float(ang.mean())) < 2
    assert bool(((a[:, 0] ** 2 + a[:, 2] ** 2 - 1).abs() < 1e-4).all())
    _, m = augment.parse("scale:0.5:2").draw_warp(n, th.Generator().manual_seed(2))
    z = ONE / m[:, 0].double()
    assert 0.4999 <= z.min() < 0.55 and 1.8 < z.max() <= 2.0001 and abs(float(z.log().mean())) < 0.05
    assert th.equal(m[:, 0], m[:, 3]) and not m[:, 1:3].any()
    _, m = augment.parse("stretch:2").draw_warp(n, th.Generator().manual_seed(3))
    r = m[:, 0].double() / m[:, 3].double()
    assert 0.4999 <= r.min() < 0.55 and 1.8 < r.max() <= 2.0001 and not m[:, 1:3].any()
    assert bool(((m[:, 0].double() * m[:, 3].double() / ONE**2 - 1).abs() < 1e-4).all())


# ---- wiring ---------------------------------------------------------------------------------------------------------
def test_apply_needs_a_gpu_and_the_binding_lists_the_entries():
    from marlclassification_amd import _lib

    assert _lib.WARP_ENTRIES == ("marl_batch_warp", "marl_batch_warp_plan")
    assert all(name in _lib._HOOKS for name in _lib.WARP_ENTRIES) and _lib.MARL_ABI_VERSION == 5
    with pytest.raises(RuntimeError, match="GPU"):
        warp.apply(th.zeros(1, 1, 4, 4), None, warp.identity(1))


def test_a_mix_policy_with_a_warping_augment_policy_is_refused_at_construction():
    from marlclassification_amd import mix
    from marlclassification_amd.data import DevicePrefetcher, ResidentLoader, SyntheticImages

    ds = SyntheticImages(8, 1, 8, 3)
    cpu = th.device("cpu")
    for spec in ("rotate:10", "d4,scale:0.9:1.1", "stretch:1.2"):
        with pytest.raises(ValueError, match="mixing warped views is not built"):
            ResidentLoader(ds, range(8), [[0, 1]], cpu, augment=augment.parse(spec), mix=mix.parse("cutmix"), nb_class=3,
                           generator=th.Generator())
        with pytest.raises(ValueError, match="mixing warped views is not built"):
            DevicePrefetcher([], cpu, augment=augment.parse(spec), mix=mix.parse("mixup"), nb_class=3,
                             generator=th.Generator())
    ResidentLoader(ds, range(8), [[0, 1]], cpu, augment=augment.parse("d4"), mix=mix.parse("cutmix"), nb_class=3,
                   generator=th.Generator())
    ResidentLoader(ds, range(8), [[0, 1]], cpu, augment=augment.parse("rotate:10"), generator=th.Generator())


def test_help_texts_name_the_new_tokens(capsys):
    from marlclassification_amd.__main__ import main

    for mode, words in (("train", ("rotate:DEG", "scale:LO:HI", "stretch:R")), ("test", ("zoom:Z1/Z2",))):
        with pytest.raises(SystemExit):
            main(["-a", "3", "--step", "3", "--run-id", "x", mode, "--help"])
        text = " ".join(capsys.readouterr().out.split())
        assert all(w in text for w in words), (mode, words)
