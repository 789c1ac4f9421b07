"""CPU: the definition of the colour jitter (``color.reference_matrix`` / ``reference_apply``), its command-line
spelling, the plan and every guard of the C entries (made-up pointers).  The yardstick of the numeric checks is a direct
float64 evaluation of the four stages with torch matrices (``_direct``): real factors ``p / 4096``, ``p / 16384``, the
plane means ``S1 / N`` unquantised, matrix products by ``@``."""
import ctypes as C
import math

import pytest
import torch as th

from marlclassification_amd import color, transforms
from marlclassification_amd.__main__ import build_parser
from tests.buffers import same_bits

Q12, Q14 = color.Q12, color.Q14


def _images(dtype, shape, n=4, seed=0):
    g = th.Generator().manual_seed(seed + 13 * shape[0] + shape[1])
    if dtype == th.uint8:
        return th.randint(0, 256, (n,) + tuple(shape), dtype=th.uint8, generator=g)
    return th.randn((n,) + tuple(shape), generator=g) * 0.75 + 1.5


def _params(n, seed, c=3, full=True):
    """n random parameter rows over the full range (factors in [0, 4], any hue angle)"""
    g = th.Generator().manual_seed(seed)
    p = th.zeros(n, 8, dtype=th.int32)
    p[:, :3] = th.randint(0, 4 * Q12 + 1, (n, 3), generator=g).to(th.int32)
    ang = (th.rand(n, generator=g, dtype=th.float64) * 2 - 1) * math.pi
    p[:, 3] = th.round(th.cos(ang) * Q14).to(th.int32)
    p[:, 4] = th.round(th.sin(ang) * Q14).to(th.int32)
    return p


def _row(beta=Q12, kappa=Q12, sigma=Q12, hcos=Q14, hsin=0):
    return [beta, kappa, sigma, hcos, hsin, 0, 0, 0]


def _direct(p, x):
    """(M [B, C, C], o [B, C]) float64 of the four stages for the images x [B, C, H, W] (o in the pixel's units)"""
    nb, c = x.shape[:2]
    pd = p.double()
    beta, kappa, sigma = (pd[:, k].clamp(0, 4 * Q12) / Q12 for k in range(3))
    hc, hs = (pd[:, k].clamp(-Q14, Q14) / Q14 for k in (3, 4))
    mean = x.double().reshape(nb, c, -1).mean(-1)
    eye = th.eye(c, dtype=th.float64)
    g = th.tensor(color.GREY, dtype=th.float64) / 256 if c == 3 else th.ones(1, dtype=th.float64)
    big_g = th.ones(c, 1, dtype=th.float64) @ g.view(1, c)
    ms, os_ = [], []
    for b in range(nb):
        m, o = beta[b] * eye, th.zeros(c, dtype=th.float64)
        mu = g @ (m @ mean[b] + o)
        m, o = kappa[b] * m, kappa[b] * o + (1 - kappa[b]) * mu
        if c == 3:
            s = sigma[b] * eye + (1 - sigma[b]) * big_g
            m, o = s @ m, s @ o
            hmat = big_g + hc[b] * (eye - big_g) + hs[b] * th.tensor(color.K, dtype=th.float64)
            m, o = hmat @ m, hmat @ o
        ms.append(m), os_.append(o)
    return th.stack(ms), th.stack(os_)


# ---- the spelling ---------------------------------------------------------------------------------------------------
def test_parse_reads_every_token():
    p = color.parse("brightness:0.4, contrast:0.3,saturation:2.5,hue:0.05,gray:0.1")
    assert (p.brightness, p.contrast, p.saturation, p.hue, p.gray) == (0.4, 0.3, 2.5, 0.05, 0.1)
    assert p.needs_stats and color.parse(p) is p
    q = color.parse("hue:0.5")
    assert not q.needs_stats and q.hue == 0.5 and q.brightness == 0 and q.spec == "hue:0.5"
    assert color.parse("contrast:3").needs_stats and not color.parse("brightness:3,saturation:1,gray:1").needs_stats


@pytest.mark.parametrize("bad", ["", "bright:0.1", "brightness", "brightness:0", "brightness:-0.1", "brightness:3.5",
                                 "contrast:x", "contrast:nan", "saturation:inf", "hue:0.6", "hue:0", "gray:1.5",
                                 "gray:0", "brightness:0.1:0.2", "brightness:0.1,brightness:0.2", "hue:0.1,",
                                 "brightness:0.1;hue:0.1", "cutmix:1"])
def test_parse_names_the_bad_token(bad):
    with pytest.raises(ValueError, match="color") as e:
        color.parse(bad)
    token = bad.split(",")[-1].strip() if "brightness:0.1,brightness" not in bad else "brightness"
    assert f'"{token}"' in str(e.value), str(e.value)


def test_parse_rejects_what_is_no_string_and_the_policy_checks_its_ranges():
    with pytest.raises(ValueError):
        color.parse(3)
    with pytest.raises(ValueError):
        color.Policy(brightness=4.0)
    with pytest.raises(ValueError):
        color.Policy(hue=0.7)


def test_draws_stay_in_their_ranges_and_come_from_the_generator_only():
    pol = color.parse("brightness:0.4,contrast:2,saturation:0.3,hue:0.1,gray:0.25")
    a = pol.draw(4096, th.Generator().manual_seed(5))
    b = pol.draw(4096, th.Generator().manual_seed(5))
    assert a.dtype == th.int32 and a.shape == (4096, 8) and th.equal(a, b) and not a[:, 5:].any()
    assert int(a[:, 0].min()) >= round(0.6 * Q12) and int(a[:, 0].max()) <= round(1.4 * Q12)
    assert int(a[:, 1].min()) >= 0 and int(a[:, 1].max()) <= 3 * Q12 and int(a[:, 1].max()) > 2 * Q12
    grey = a[:, 2] == 0
    assert 0.2 < grey.double().mean().item() < 0.3
    assert int(a[~grey, 2].min()) >= round(0.7 * Q12) and int(a[:, 2].max()) <= round(1.3 * Q12)
    ang = th.atan2(a[:, 4].double(), a[:, 3].double())
    assert ang.abs().max().item() <= 2 * math.pi * 0.1 + 1e-3 and ang.min().item() < -0.5 and ang.max().item() > 0.5
    assert ((a[:, 3].double() ** 2 + a[:, 4].double() ** 2).sqrt() - Q14).abs().max().item() <= 1.0
    # a stage that is off gets its identity, whatever the others draw
    off = color.parse("hue:0.2").draw(64, th.Generator().manual_seed(1))
    assert bool((off[:, :3] == Q12).all()) and bool((off[:, 4] != 0).any())
    assert th.equal(color.parse("gray:1").draw(8, th.Generator().manual_seed(1))[:, :5],
                    th.tensor([[Q12, Q12, 0, Q14, 0]] * 8, dtype=th.int32))
    assert color.parse("brightness:1").draw(0, th.Generator().manual_seed(1)).shape == (0, 8)


def test_the_flag_reaches_the_training_configuration(tmp_path, monkeypatch):
    from marlclassification_amd import __main__ as cli
    from marlclassification_amd import train as train_mod

    parse = lambda *a: build_parser().parse_args(["--run-id", "x", "train", "-o", "out", *a])  # noqa: E731
    assert parse().color is None
    assert parse("--color", "brightness:0.2,hue:0.05").color == "brightness:0.2,hue:0.05"
    for bad in ("none", "hue:0.9", "brightness", ""):
        with pytest.raises(SystemExit):
            parse("--color", bad)
    seen = {}
    monkeypatch.setattr(train_mod, "train_main", lambda m, mc, tc, **kw: seen.update(model=mc, train=tc))
    cli.main(["--run-id", "x", "train", "-o", str(tmp_path), "--color", "contrast:0.5"])
    assert seen["train"].color == "contrast:0.5" and not hasattr(seen["model"], "color")  # (not a key of marl.json)
    cli.main(["--run-id", "x", "train", "-o", str(tmp_path)])
    assert seen["train"].color is None


# ---- the definition against the float64 yardstick -------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_reference_matrix_against_a_direct_float64_evaluation(c):
    """uint8: |A_q / 4096 - M| <= 0.5 / 4096 (the rounding; 1e-9 for the two float64 evaluation orders).  S and H keep
    the vector 1 (their rows sum to 1), so o = (1 - kappa) beta (g . m) 1: the quantised mean (< 1 / 256 grey level,
    g sums to 1) moves it by at most |1 - kappa| beta / 256 <= 3 * 4 / 256.  fp32: one float32 rounding of the same
    float64 chain, |M| <= 70 and |o| <= 12 max|mean|: 2^-24 of those."""
    x = _images(th.uint8, (c, 9, 11), n=64, seed=c)
    p = _params(64, 7 + c)
    rec = transforms.reference_stats(x)
    a = color.reference_matrix(p, rec, (c, 9, 11), True)
    m, o = _direct(p, x)
    assert a.dtype == th.int32 and a.shape == (64, c, c + 1)
    assert (a[:, :, :c].double() / 4096 - m).abs().max().item() <= 0.5 / 4096 + 1e-9
    assert (a[:, :, c].double() / 4096 - o).abs().max().item() <= 0.5 / 4096 + 12 / 256 + 1e-9
    assert int(a[:, :, :c].abs().max()) <= 70 * 4096 < 2 ** 19 and int(a[:, :, c].abs().max()) < 2 ** 30
    # without records contrast is off: the matrix of kappa = 1
    p1 = p.clone()
    p1[:, 1] = Q12
    assert th.equal(color.reference_matrix(p, None, (c, 9, 11), True)[:, :, :c],
                    color.reference_matrix(p1, rec, (c, 9, 11), True)[:, :, :c])
    assert not color.reference_matrix(p, None, (c, 9, 11), True)[:, :, c].any()
    xf = _images(th.float32, (c, 9, 11), n=64, seed=c)
    recf = transforms.reference_stats(xf)
    af = color.reference_matrix(p, recf, (c, 9, 11), False)
    m, o = _direct(p, xf)
    assert af.dtype == th.float32
    assert (af[:, :, :c].double() - m).abs().max().item() <= 70 * 2.0 ** -24 + 1e-9
    top = xf.double().reshape(64, c, -1).mean(-1).abs().max().item()
    assert (af[:, :, c].double() - o).abs().max().item() <= 12 * top * 2.0 ** -24 + 1e-9


def test_reference_apply_uint8_within_one_grey_level_of_the_float64_formula():
    """4000 random draws over the full parameter range against clamp(floor(M x + o + 0.5)) in float64 with the
    quantised mean the definition uses: 0.5 for the rounding + 3 * 255 / 8192 + 1 / 8192 for the quantisation < 1."""
    n = 4000
    x = _images(th.uint8, (3, 2, 3), n=n, seed=3)
    p = _params(n, 11)
    rec = transforms.reference_stats(x)
    got = color.reference_apply(x, None, p, rec)
    assert got.dtype == th.uint8 and got.shape == x.shape
    # the yardstick takes the same quantised plane means (m_q8 / 256): feed it images whose planes ARE that mean
    mq = ((256 * rec[:, :, 0]) // 6).double() / 256
    m, o = _direct(p, mq.view(n, 3, 1, 1).expand(n, 3, 2, 3))
    y = th.einsum("bij,bjhw->bihw", m, x.double()) + o.view(n, 3, 1, 1)
    want = th.floor(y + 0.5).clamp(0, 255)
    assert ((got.double() - want).abs() <= 1).all()
    a = color.reference_matrix(p, rec, (3, 2, 3), True).to(th.int64)
    acc = (a[:, :, :3].abs().sum(-1) * 255 + a[:, :, 3].abs()).max().item()
    assert acc + 2048 < 2 ** 31  # (the int32 accumulator cannot overflow: 3 * 2^19 * 255 + 2^30 + 2048 < 2^31)


def test_reference_apply_fp32_rounds_every_product_and_sum():
    x = _images(th.float32, (3, 5, 7))
    p = _params(4, 2)
    rec = transforms.reference_stats(x)
    a = color.reference_matrix(p, rec, (3, 5, 7), False)
    got = color.reference_apply(x, None, p, rec)
    for i in range(3):
        want = ((x[:, 0] * a[:, i, 0, None, None] + x[:, 1] * a[:, i, 1, None, None]) + x[:, 2] * a[:, i, 2, None, None]
                ) + a[:, i, 3, None, None]
        assert th.equal(got[:, i], want), i
    m, o = _direct(p, x)
    y = th.einsum("bij,bjhw->bihw", m, x.double()) + o.view(4, 3, 1, 1)
    scale = th.einsum("bij,bjhw->bihw", m.abs(), x.double().abs()) + o.abs().view(4, 3, 1, 1)
    # (4 rounded coefficients, 3 products, 3 sums: 10 relative errors of 2^-24, first order; 11 covers the second)
    assert ((got.double() - y).abs() <= 11 * 2.0 ** -24 * scale).all()


# ---- identities -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("c", [1, 3])
def test_identities(dtype, c):
    x = _images(dtype, (c, 6, 5), n=5, seed=9)
    rows = th.tensor([3, 0, 0, 4, -7, 99])  # repeated, and clamped to [0, 5)
    picked = x[rows.clamp(0, 4)]
    rec = transforms.reference_stats(picked)
    ident = th.tensor([_row()] * 6, dtype=th.int32)
    same = color.reference_apply(x, rows, ident, rec)
    assert same.dtype == dtype and same_bits(same, picked), "the identity returns the source bytes"
    assert th.equal(color.reference_apply(x, None, ident[:5]), x)
    black = color.reference_apply(x, rows, th.tensor([_row(beta=0)] * 6, dtype=th.int32), rec)
    assert not black.any()
    flat = color.reference_apply(x, rows, th.tensor([_row(kappa=0)] * 6, dtype=th.int32), rec)
    assert bool((flat == flat[:, :, :1, :1]).all()), "kappa = 0: one value per plane"
    if c == 3:
        assert bool((flat == flat[:, :1]).all()), "... the grey mean, the same on every plane"
        mean = picked.double().reshape(6, 3, -1).mean(-1)
        grey = (mean * th.tensor(color.GREY, dtype=th.float64) / 256).sum(-1)
        assert (flat[:, 0, 0, 0].double() - grey).abs().max().item() <= (1.0 if dtype == th.uint8 else 1e-5)
        mono = color.reference_apply(x, rows, th.tensor([_row(sigma=0)] * 6, dtype=th.int32), rec)
        assert th.equal(mono[:, 0], mono[:, 1]) and th.equal(mono[:, 1], mono[:, 2]), "sigma = 0: three equal planes"
        assert bool(mono.any())


def test_grey_pixels_are_fixed_under_saturation_and_hue():
    v = th.arange(256, dtype=th.uint8).view(1, 1, 16, 16).expand(1, 3, 16, 16).contiguous()
    p = _params(200, 4)
    p[:, 0] = p[:, 1] = Q12  # (brightness and contrast off)
    out = color.reference_apply(v, th.zeros(200, dtype=th.int64), p)
    assert th.equal(out, v.expand(200, 3, 16, 16))
    a = color.reference_matrix(p, None, (3, 16, 16), True)
    assert int((a[:, :, :3].sum(-1) - 4096).abs().max()) <= 2  # (rows of A_q sum to 4096 up to their three roundings)
    assert all(sum(r) == 0.0 for r in color.K), "K's rows sum to exactly 0"
    vf = (v.float() / 255).contiguous()
    outf = color.reference_apply(vf, th.zeros(200, dtype=th.int64), p)
    assert (outf - vf).abs().max().item() <= 4 * 70 * 2.0 ** -24


def test_hostile_params_are_clamped():
    x = _images(th.uint8, (3, 4, 4), n=3, seed=2)
    rec = transforms.reference_stats(x)
    big, small = 2 ** 31 - 1, -2 ** 31
    hostile = th.tensor([[big, big, big, big, big, 7, 7, 7], [small, small, small, small, small, -1, -1, -1],
                         [5 * Q12, -3, 4 * Q12 + 1, Q14 + 1, -Q14 - 1, 0, 0, 0]], dtype=th.int64)
    tame = th.tensor([[4 * Q12, 4 * Q12, 4 * Q12, Q14, Q14, 0, 0, 0], [0, 0, 0, -Q14, -Q14, 0, 0, 0],
                      [4 * Q12, 0, 4 * Q12, Q14, -Q14, 0, 0, 0]], dtype=th.int64)
    assert th.equal(color.reference_matrix(hostile, rec, (3, 4, 4), True), color.reference_matrix(tame, rec, (3, 4, 4), True))
    assert th.equal(color.reference_apply(x, None, hostile, rec), color.reference_apply(x, None, tame, rec))
    with pytest.raises(ValueError, match="channels"):
        color.reference_matrix(tame, None, (2, 4, 4), True)
    with pytest.raises(ValueError, match="params"):
        color.reference_matrix(tame[:, :5], None, (3, 4, 4), True)
    with pytest.raises(ValueError, match="records"):
        color.reference_matrix(tame, rec[:2], (3, 4, 4), True)


def test_the_fused_form_is_the_two_steps_by_definition():
    x = _images(th.uint8, (3, 5, 7))
    p = _params(4, 6)
    rec = transforms.reference_stats(x)
    for spec in ("user-normal:0.485,0.456,0.406:0.229,0.224,0.225", "user-minmax:0.0,0.1,-0.5:1.0,0.8,2.0"):
        fused = color.reference_apply(x, None, p, rec, normalize=spec)
        assert fused.dtype == th.float32
        assert th.equal(fused, transforms.reference_apply(color.reference_apply(x, None, p, rec), None, spec))
    with pytest.raises(ValueError, match="two steps"):
        color.reference_apply(x, None, p, rec, normalize="channel-normal")
    with pytest.raises(ValueError, match="uint8"):
        color.reference_apply(x.float(), None, p, None, normalize="user-normal:0.5,0.5,0.5:0.2,0.2,0.2")


# ---- the C entries: bound beside the ABI, plan and guards are host arithmetic ----------------------------------------
def test_the_entries_are_bound_beside_the_versioned_abi():
    from marlclassification_amd import _lib

    assert _lib.COLOR_ENTRIES == ("marl_batch_color", "marl_batch_color_plan")
    assert all(name in _lib._HOOKS for name in _lib.COLOR_ENTRIES)
    assert not any(name in _lib.EXPORTS for name in _lib.COLOR_ENTRIES)
    assert _lib.MARL_ABI_VERSION == 5 and len(_lib.EXPORTS) == 57


SRC, DST, REC, PAR, COEF = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000


def test_the_plan_is_host_arithmetic():
    from marlclassification_amd import _lib

    lib = _lib.load()
    info = color.ColorPlan()

    def plan(c, h, w, elt, form, src=SRC, dst=DST):
        rc = lib.marl_batch_color_plan(c, h, w, elt, form, src, dst, C.byref(info))
        return rc, info.as_dict()

    rc, p = plan(3, 256, 256, 1, 0)
    assert rc == 0 and p == dict(load_bytes=16, store_bytes=16, pixels_per_vector=16, vectors_per_thread=4, blocks_per_image=4, lds_bytes=0)
    rc, p = plan(3, 256, 256, 1, 1)
    assert rc == 0 and p == dict(load_bytes=4, store_bytes=16, pixels_per_vector=4, vectors_per_thread=4, blocks_per_image=16, lds_bytes=0)
    rc, p = plan(3, 256, 256, 4, 0)
    assert rc == 0 and p == dict(load_bytes=16, store_bytes=16, pixels_per_vector=4, vectors_per_thread=4, blocks_per_image=16, lds_bytes=0)
    # the widest width that divides a plane's bytes and both addresses
    for (h, w, elt, soff, doff), (load, px) in ((((5, 7, 1, 0, 0), (1, 1)), ((6, 6, 1, 0, 0), (4, 4)),
                                                ((6, 4, 1, 0, 0), (8, 8)), ((8, 8, 1, 0, 0), (16, 16)),
                                                ((8, 8, 1, 8, 0), (8, 8)), ((8, 8, 1, 0, 4), (4, 4)),
                                                ((8, 8, 1, 2, 0), (1, 1)), ((8, 8, 1, 0, 1), (1, 1)),
                                                ((5, 7, 4, 0, 0), (4, 1)), ((5, 6, 4, 0, 0), (8, 2)),
                                                ((8, 8, 4, 0, 0), (16, 4)), ((8, 8, 4, 4, 0), (4, 1)),
                                                ((8, 8, 4, 0, 8), (8, 2)), ((1, 1, 1, 0, 0), (1, 1)))):
        rc, p = plan(3, h, w, elt, 0, SRC + soff, DST + doff)
        assert rc == 0 and (p["load_bytes"], p["pixels_per_vector"]) == (load, px), (h, w, elt, soff, doff, p)
        assert p["store_bytes"] == load and p["blocks_per_image"] == -(-(h * w // px) // (256 * p["vectors_per_thread"]))
    for (h, w, soff, doff), px in (((8, 8, 0, 0), 4), ((5, 7, 0, 0), 1), ((8, 8, 2, 0), 1), ((8, 8, 0, 8), 1),
                                   ((8, 8, 4, 16), 4)):
        rc, p = plan(1, h, w, 1, 1, SRC + soff, DST + doff)
        assert rc == 0 and (p["load_bytes"], p["store_bytes"], p["pixels_per_vector"]) == (px, 4 * px, px)
    rc, p = plan(3, 8, 8, 1, 0, None, None)  # (no addresses: by the plane's size alone)
    assert rc == 0 and p["load_bytes"] == 16
    assert lib.marl_batch_color_plan(3, 8, 8, 1, 0, SRC, DST, None) == -1
    for args, word in (((2, 8, 8, 1, 0), "neither 1 nor 3"), ((0, 8, 8, 1, 0), "neither 1 nor 3"),
                       ((3, 8, 8, 2, 0), "elt_bytes"), ((3, 0, 8, 1, 0), "positive"), ((3, 8, -1, 4, 0), "positive"),
                       ((3, 8, 8, 1, 2), "out_form"), ((3, 8, 8, 4, 1), "uint8"), ((3, 8, 8, 1, 1, SRC, DST + 2), "aligned"),
                       ((3, 8, 8, 4, 0, SRC + 2, DST), "aligned")):
        rc, _ = plan(*args)
        msg = lib.marl_last_error().decode()
        assert rc == -1 and msg.startswith("marl_batch_color_plan:") and word in msg, (args, rc, msg)
    for args in ((3, 32768, 32768, 1, 0), (1, 16384, 32768, 4, 0), (3, 16384, 16384, 1, 1)):
        rc, _ = plan(*args)
        assert rc == -2 and "2^31" in lib.marl_last_error().decode(), args


def test_every_guard_answers_before_anything_is_enqueued():
    """No GPU: made-up pointers, never dereferenced - every refusal comes from host arithmetic."""
    from marlclassification_amd import _lib

    lib = _lib.load()
    user = (C.c_double * 6)(0.5, 0.25, 0.5, 0.25, 0.5, 0.25)

    def call(src=SRC, n_src=4, rows=None, rec=REC, par=PAR, form=0, mode=0, usr=None, batch=4, c=3, h=8, w=8, elt=1,
             dst=DST, coef=COEF):
        rc = lib.marl_batch_color(src, n_src, rows, rec, par, form, mode, usr, batch, c, h, w, elt, dst, coef, None)
        return rc, lib.marl_last_error().decode()

    zero_s = (C.c_double * 6)(0.5, 0.25, 0.5, 0.0, 0.5, 0.25)
    same = (C.c_double * 6)(0.5, 0.9, 0.3, 0.3, 0.5, 0.9)
    nan = (C.c_double * 6)(float("nan"), 0.9, 0.3, 0.4, 0.5, 0.9)
    for kw, word in ((dict(src=None), "null"), (dict(dst=None), "null"), (dict(par=None), "null"),
                     (dict(c=2), "neither 1 nor 3"), (dict(c=4), "neither 1 nor 3"), (dict(c=0), "neither 1 nor 3"),
                     (dict(elt=2), "elt_bytes"), (dict(elt=0), "elt_bytes"), (dict(form=2), "out_form"),
                     (dict(form=-1), "out_form"), (dict(form=1, mode=4, usr=user, elt=4), "uint8"),
                     (dict(form=1, mode=1, usr=user), "statistic"), (dict(form=1, mode=0, usr=user), "statistic"),
                     (dict(form=1, mode=6, usr=user), "user norm_mode"), (dict(form=1, mode=4, usr=None), "needs user"),
                     (dict(form=1, mode=4, usr=zero_s), "s must"), (dict(form=1, mode=5, usr=same), "hi - lo"),
                     (dict(form=1, mode=4, usr=nan), "finite"),
                     (dict(batch=0), "positive"), (dict(batch=-3), "positive"), (dict(n_src=0), "positive"),
                     (dict(h=0), "positive"), (dict(w=-1), "positive"), (dict(n_src=3), "n_src"),
                     (dict(src=SRC + 2, elt=4), "aligned"), (dict(dst=DST + 2, elt=4), "aligned"),
                     (dict(form=1, mode=4, usr=user, dst=DST + 2), "aligned"),
                     (dict(rec=REC + 4), "records"), (dict(rows=REC + 4), "rows"), (dict(coef=COEF + 2), "coef"),
                     (dict(par=PAR + 2), "params"),
                     (dict(dst=SRC), "overlaps"), (dict(dst=SRC + 4 * 3 * 64 - 1), "overlaps"),
                     (dict(dst=SRC - 4 * 3 * 64 + 1), "overlaps"),
                     (dict(form=1, mode=4, usr=user, dst=SRC - 4 * 4 * 3 * 64 + 4), "overlaps")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("marl_batch_color:") and word in msg, (kw, rc, msg)
    for kw, word in ((dict(c=3, h=32768, w=32768), "2^31"), (dict(c=1, h=16384, w=32768, elt=4), "2^31"),
                     (dict(form=1, mode=4, usr=user, c=3, h=16384, w=16384), "2^31"),
                     (dict(n_src=2 ** 62), "overflow"),
                     (dict(batch=2 ** 31 - 1, n_src=1, rows=REC, c=1, h=128, w=256, dst=0x7000000000), "workgroups")):
        rc, msg = call(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)
    # adjacent buffers are no overlap: the refusal above turns into a launch attempt only on a GPU, so ask the guards
    # for the NEXT refusal instead - a misaligned coef behind an adjacent, legal dst
    for dst in (SRC + 4 * 3 * 64, SRC - 4 * 3 * 64):
        rc, msg = call(dst=dst, coef=COEF + 1)
        assert rc == -1 and "coef" in msg, (dst, msg)
