"""GPU: the colour jitter ``marl_batch_color`` (``color.apply``) against its definition on the CPU
(``color.reference_matrix`` / ``reference_apply``).

* uint8: ``coef`` equals ``reference_matrix`` integer for integer and the pixels equal ``reference_apply`` byte for
  byte - everything up to the ``rint`` is IEEE ``+ - *`` on exactly representable inputs.
* fp32: the pixels are bit-equal to the pixel rule (``color.apply_matrix``) under the ``coef`` the device returned, and
  ``coef`` is within 1 fp32 ulp of ``reference_matrix`` of the device's own records (the mean is one fp64 division; both
  sides round the same fp64 chain once).  Equality is expected; with MARL_COLOR_ERRORS=<file> the achieved differences
  are written there as JSON (profiles/color_errors.json is one such run).
* ``out_form="norm"`` is bit-equal to ``color.apply`` followed by ``transforms.apply`` in both user modes.
Shapes are the smallest that reach every path (every vector width, planes that are no multiple of 4, more than one
workgroup an image - taken from the plan).  Every destination sits inside a larger buffer whose guard bytes must
survive."""
import ctypes as C
import json
import math
import os

import pytest
import torch as th

from marlclassification_amd import augment, color, transforms
from tests.buffers import N_SRC, source
from tests.buffers import bits as _bits
from tests.buffers import guarded as _guarded
from tests.buffers import guards_intact as _guards_intact
from tests.buffers import same_bits as _same
from tests.buffers import ulps as _ulps

pytestmark = pytest.mark.gpu

Q12, Q14 = color.Q12, color.Q14
DTYPES = pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
ACHIEVED = {}


@pytest.fixture(scope="module", autouse=True)
def _record_achieved():
    yield
    path = os.environ.get("MARL_COLOR_ERRORS")
    if path:
        with open(path, "w") as fh:
            json.dump(ACHIEVED, fh, indent=1, sort_keys=True)
            fh.write("\n")


def _row(beta=Q12, kappa=Q12, sigma=Q12, turns=0.0):
    a = 2.0 * math.pi * turns
    return [beta, kappa, sigma, round(Q14 * math.cos(a)), round(Q14 * math.sin(a)), 0, 0, 0]


def _stage_params(seed=0):
    """every stage alone at a few strengths (its two ends included), then all stages together at random"""
    rows = [_row()]
    rows += [_row(beta=v) for v in (0, 1500, 6000, 4 * Q12)]
    rows += [_row(kappa=v) for v in (0, 2000, 7000, 4 * Q12)]
    rows += [_row(sigma=v) for v in (0, 3000, 9000, 4 * Q12)]  # (4.0: both clamp ends of a uint8 output are reached)
    rows += [_row(turns=t) for t in (-0.5, -0.07, 0.25, 0.4)]
    g = th.Generator().manual_seed(seed)
    for _ in range(7):
        b, k, s = th.randint(0, 4 * Q12 + 1, (3,), generator=g).tolist()
        rows.append(_row(b, k, s, float(th.rand(1, generator=g)) - 0.5))
    return th.tensor(rows, dtype=th.int32)


def _check_case(device, src, rows, params, with_records=True, src_d=None, offset=0, key=None, want_px=None):
    """color.apply of src[rows] on the device against the definition, every property of the docstring"""
    nb = params.shape[0]
    c = src.shape[1]
    shape = (nb,) + tuple(src.shape[1:])
    u8 = src.dtype == th.uint8
    src_d = src.to(device) if src_d is None else src_d
    rows_d, params_d = None if rows is None else rows.to(device), params.to(device)
    rec_d = transforms.stats(src_d, rows_d) if with_records else None
    buf, out = _guarded(shape, src.dtype, device, offset)
    cbuf, _ = _guarded((nb, c, c + 1), th.int32, device)
    if want_px is not None:
        assert color.plan(src_d, out)["pixels_per_vector"] == want_px
    got, coef = color.apply(src_d, rows_d, params_d, rec_d, return_coef=True, out=out)
    assert got.data_ptr() == out.data_ptr()
    th.cuda.synchronize(device)
    assert _guards_intact(buf, offset, out.numel() * out.element_size())
    got, coef = got.cpu(), coef.cpu()
    rec = None if rec_d is None else rec_d.cpu()
    if u8 and rec is not None:
        assert th.equal(rec, transforms.reference_stats(src, rows))
    want_coef = color.reference_matrix(params, rec, src.shape[1:], u8)
    picked = transforms._selected(src, rows)
    if u8:
        assert coef.dtype == th.int32 and th.equal(coef, want_coef)
        assert th.equal(got, color.reference_apply(src, rows, params, rec))
        worst = 0
    else:
        assert coef.dtype == th.float32
        worst = int(_ulps(coef, want_coef).max())
        assert worst <= 1, (coef, want_coef)
        assert th.equal(_bits(got), _bits(color.apply_matrix(picked, coef)))
        exact = (_ulps(coef, want_coef) == 0).all(dim=2).all(dim=1)
        assert th.equal(_bits(got[exact]), _bits(color.reference_apply(src, rows, params, rec)[exact]))
    if key is not None:
        ACHIEVED[key] = {"coef_max_ulps": worst, "pixels_bit_equal": True}
    return got, coef


def _rows_for(nb):
    return th.tensor([(7 * i + 10) % N_SRC for i in range(nb)])


# ---- shapes -----------------------------------------------------------------------------------------------------------
# pixels per vector: uint8 / fp32
SHAPES = [((1, 1, 1), 1, 1), ((3, 1, 1), 1, 1), ((3, 5, 7), 1, 1), ((3, 8, 8), 16, 4), ((1, 28, 28), 16, 4),
          ((3, 33, 31), 1, 1), ((3, 6, 6), 4, 4), ((3, 5, 6), 1, 2), ((1, 6, 4), 8, 4)]


@DTYPES
@pytest.mark.parametrize("shape,px8,px32", SHAPES, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else None)
def test_small_shapes_every_stage_alone_and_all_together(device, shape, px8, px32, dtype):
    src = source(shape, dtype, affine=(0.75, 1.5))
    params = _stage_params(shape[1])
    rows = _rows_for(params.shape[0])
    name = "x".join(map(str, shape)) + ("/u8" if dtype == th.uint8 else "/f32")
    got, _ = _check_case(device, src, rows, params, key=name, want_px=px8 if dtype == th.uint8 else px32)
    _check_case(device, src, rows, params, with_records=False)  # (no records: contrast is off)
    if dtype == th.uint8 and shape[0] == 3 and shape[1] * shape[2] >= 35:
        strong = got[12]  # sigma = 4.0
        assert bool((strong == 0).any()) and bool((strong == 255).any()), "both clamp ends"
    assert _same(got[0], src[rows[0]]), "the identity is a bit copy"


@DTYPES
@pytest.mark.parametrize("c", [1, 3])
def test_a_shape_from_the_plan_with_two_workgroups_an_image(device, dtype, c):
    probe = th.empty(1, c, 16, 16, dtype=dtype)
    px, vpt = (color.plan(probe)[k] for k in ("pixels_per_vector", "vectors_per_thread"))
    h, w = px, 256 * vpt + 1  # one vector a plane more than a workgroup's 256 * vectors_per_thread
    src = source((c, h, w), dtype, n=3, seed=5, affine=(0.75, 1.5))
    assert color.plan(src)["blocks_per_image"] == 2 and color.plan(src)["pixels_per_vector"] == px
    params = _stage_params(3)[[0, 3, 6, 11, 17, 20]]
    _check_case(device, src, th.tensor([2, 0, 2, 1, 1, 0]), params, key=f"{c}x{h}x{w}/" + ("u8" if dtype == th.uint8 else "f32"))


# ---- the fused output form --------------------------------------------------------------------------------------------
def _user(c):
    m, s = [0.485, 0.456, 0.406][:c], [0.229, 0.224, 0.225][:c]
    lo, hi = [0.0, 0.1, -0.5][:c], [1.0, 0.8, 2.0][:c]
    return (transforms.Spec("user-normal", tuple(m), tuple(s)).spelling,
            transforms.Spec("user-minmax", tuple(lo), tuple(hi)).spelling)


@pytest.mark.parametrize("shape,px,offset", [((3, 8, 8), 4, 0), ((3, 5, 7), 1, 0), ((1, 28, 28), 4, 0),
                                             ((3, 8, 8), 1, 8), ((3, 16, 257), 4, 0), ((1, 33, 31), 1, 0)],
                         ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else None)
def test_out_norm_is_out_same_followed_by_the_user_normalisation(device, shape, px, offset):
    src = source(shape, th.uint8)
    params = _stage_params(1)
    nb = params.shape[0]
    rows = _rows_for(nb)
    src_d, rows_d, params_d = src.to(device), rows.to(device), params.to(device)
    rec_d = transforms.stats(src_d, rows_d)
    same, coef = color.apply(src_d, rows_d, params_d, rec_d, return_coef=True)
    for spec in _user(shape[0]):
        buf, out = _guarded((nb,) + shape, th.float32, device, offset)
        assert color.plan(src_d, out, "norm")["pixels_per_vector"] == px
        fused, coef_n = color.apply(src_d, rows_d, params_d, rec_d, out_form="norm", normalize=spec, return_coef=True,
                                    out=out)
        two = transforms.apply(same, None, spec)
        th.cuda.synchronize(device)
        assert _guards_intact(buf, offset, out.numel() * 4)
        assert fused.dtype == th.float32 and th.equal(_bits(fused), _bits(two)), spec
        assert th.equal(coef_n, coef)
        want = color.reference_apply(src, rows, params, rec_d.cpu(), normalize=spec)
        assert th.equal(_bits(fused.cpu()), _bits(want)), spec
    with pytest.raises(ValueError, match="two steps"):
        color.apply(src_d, rows_d, params_d, rec_d, out_form="norm", normalize="channel-normal")
    with pytest.raises(ValueError, match="uint8"):
        color.apply(src_d.float(), rows_d, params_d, None, out_form="norm", normalize=_user(shape[0])[0])


# ---- robustness -------------------------------------------------------------------------------------------------------
@DTYPES
def test_hostile_rows_and_params_are_clamped(device, dtype):
    src = source((3, 8, 10), dtype, affine=(0.75, 1.5))
    rows = th.tensor([-1, -2 ** 62, N_SRC, 2 ** 62, 5, 2 ** 31])
    big, small = 2 ** 31 - 1, -2 ** 31
    hostile = th.tensor([[big] * 8, [small] * 8, [5 * Q12, -3, 4 * Q12 + 1, Q14 + 1, -Q14 - 1, 9, 9, 9],
                         [big, small, big, small, big, 0, 0, 0], _row(), [-1, -1, -1, 0, 0, -1, -1, -1]], dtype=th.int32)
    got, coef = _check_case(device, src, rows, hostile)
    tame = th.tensor([[4 * Q12, 4 * Q12, 4 * Q12, Q14, Q14, 0, 0, 0], [0, 0, 0, -Q14, -Q14, 0, 0, 0],
                      [4 * Q12, 0, 4 * Q12, Q14, -Q14, 0, 0, 0], [4 * Q12, 0, 4 * Q12, -Q14, Q14, 0, 0, 0], _row(),
                      [0, 0, 0, 0, 0, 0, 0, 0]], dtype=th.int32)
    clamped = th.tensor([0, 0, N_SRC - 1, N_SRC - 1, 5, N_SRC - 1])
    got2, coef2 = _check_case(device, src, clamped, tame)
    assert _same(got, got2) and th.equal(_bits(coef), _bits(coef2))


def test_a_nan_behind_a_zero_coefficient_stays_where_it_is(device):
    src = source((3, 6, 6), th.float32, n=3)
    src[0, 1, 2, 3] = float("nan")
    src[1, 0, 0, 0] = float("inf")
    src[2, 2, 5, 5] = float("nan")
    ident = th.tensor([_row()] * 3, dtype=th.int32)
    got, coef = _check_case(device, src, None, ident, with_records=False)
    assert th.equal(_bits(got), _bits(src)), "the identity is a bit copy, NaN and inf included"
    assert th.equal(coef[:, :, :3], th.eye(3).expand(3, 3, 3)) and not coef[:, :, 3].any()
    # brightness only: the matrix stays diagonal, so the NaN stays in its own plane
    got, _ = _check_case(device, src, None, th.tensor([_row(beta=6000)] * 3, dtype=th.int32), with_records=False)
    assert bool(th.isnan(got[0, 1, 2, 3])) and int(th.isnan(got).sum()) == 2 and bool(th.isinf(got[1, 0, 0, 0]))
    # beta = 0: every coefficient is 0, every term is skipped
    got, _ = _check_case(device, src, None, th.tensor([_row(beta=0)] * 3, dtype=th.int32), with_records=False)
    assert not got.any() and not th.isnan(got).any()


@DTYPES
def test_guard_bytes_around_exactly_sized_dst_and_coef_of_the_c_entry(device, dtype):
    from marlclassification_amd import _lib

    lib = _lib.load()
    shape = (3, 33, 31)
    src = source(shape, dtype, affine=(0.75, 1.5))
    params = _stage_params(2)
    nb = params.shape[0]
    rows = _rows_for(nb)
    src_d, rows_d, params_d = src.to(device), rows.to(device), params.to(device)
    rec_d = transforms.stats(src_d, rows_d)
    dbuf, dst = _guarded((nb,) + shape, dtype, device)
    cbuf, coef = _guarded((nb, 3, 4), th.int32 if dtype == th.uint8 else th.float32, device)
    stream = th.cuda.current_stream(device).cuda_stream

    def call(coef_p):
        _lib.check(lib.marl_batch_color(src_d.data_ptr(), N_SRC, rows_d.data_ptr(), rec_d.data_ptr(),
                                        params_d.data_ptr(), 0, 0, None, nb, 3, 33, 31, src.element_size(),
                                        dst.data_ptr(), coef_p, stream))
        th.cuda.synchronize(device)

    call(coef.data_ptr())
    assert _guards_intact(dbuf, 0, dst.numel() * dst.element_size()) and _guards_intact(cbuf, 0, coef.numel() * 4)
    got, pairs = color.apply(src_d, rows_d, params_d, rec_d, return_coef=True)
    assert _same(dst, got)
    assert th.equal(_bits(coef), _bits(pairs))
    first = dst.clone()
    dst.zero_()
    call(None)  # coef == NULL: the same pixels
    assert _same(dst, first)


@DTYPES
def test_a_framed_source_and_destination_take_the_width_their_addresses_allow(device, dtype):
    shape = (3, 8, 8)
    src = source(shape, dtype, affine=(0.75, 1.5))
    params = _stage_params(4)[:8]
    rows = _rows_for(8)
    elt = 1 if dtype == th.uint8 else 4
    for s_off, d_off, px in ((0, 0, 16 // elt), (8, 0, 8 // elt), (0, 4, 4 // elt), (4, 8, 4 // elt)) + \
            (((1, 0, 1), (0, 2, 1)) if elt == 1 else ()):
        sbuf, framed = _guarded((N_SRC,) + shape, dtype, device, s_off)
        framed.copy_(src)
        _check_case(device, src, rows, params, src_d=framed, offset=d_off, want_px=px)
        assert _guards_intact(sbuf, s_off, framed.numel() * elt)


def test_source_offsets_are_64_bit(device):
    """A uint8 set of more than 2^32 bytes (nothing filled but the rows used): the last row and row 0."""
    n, shape = 21846, (3, 256, 256)
    assert n * 3 * 256 * 256 > 2 ** 32
    big = th.empty((n,) + shape, dtype=th.uint8, device=device)
    two = source(shape, th.uint8, n=2, seed=9)
    big[n - 1].copy_(two[0])
    big[0].copy_(two[1])
    rows = th.tensor([n - 1, 0, n - 1], device=device)
    params = _stage_params(6)[[17, 18, 19]]
    rec = transforms.stats(big, rows)
    small_rows = th.tensor([0, 1, 0])
    assert th.equal(rec.cpu(), transforms.reference_stats(two, small_rows))
    got, coef = color.apply(big, rows, params.to(device), rec, return_coef=True)
    assert th.equal(coef.cpu(), color.reference_matrix(params, rec.cpu(), shape, True))
    assert th.equal(got.cpu(), color.reference_apply(two, small_rows, params, rec.cpu()))
    spec = _user(3)[0]
    fused = color.apply(big, rows, params.to(device), rec, out_form="norm", normalize=spec)
    assert th.equal(_bits(fused.cpu()), _bits(color.reference_apply(two, small_rows, params, rec.cpu(), normalize=spec)))
    del big
    th.cuda.empty_cache()


def test_two_calls_give_the_same_bytes_and_a_side_stream_is_respected(device):
    src = source((3, 16, 257), th.float32, n=4, seed=3)
    rows = th.tensor([3, 1, 1, 0])
    params = _stage_params(8)[[17, 18, 19, 20]]
    src_d, rows_d, params_d = src.to(device), rows.to(device), params.to(device)
    rec = transforms.stats(src_d, rows_d)
    (xa, ca), (xb, cb) = (color.apply(src_d, rows_d, params_d, rec, return_coef=True) for _ in range(2))
    assert th.equal(_bits(xa), _bits(xb)) and th.equal(_bits(ca), _bits(cb))
    # the source is produced on a side stream behind some work; the launch must queue behind it on that stream
    side = th.cuda.Stream(device=device)
    late = th.zeros_like(src_d)
    m = th.randn(2048, 2048, device=device)
    th.cuda.synchronize(device)
    with th.cuda.stream(side):
        for _ in range(8):
            m = (m @ m).clamp_(-1.0, 1.0)
        late.copy_(src_d)
        got = color.apply(late, rows_d, params_d, rec)
    side.synchronize()
    assert th.equal(_bits(got), _bits(xa))


def test_every_guard_of_the_c_entry(device):
    """real device buffers (the host-only list of tests/test_color_host.py, with pointers that could be used): a refusal
    enqueues nothing, adjacent buffers are no overlap, and a good call after the refusals runs"""
    from marlclassification_amd import _lib

    lib = _lib.load()
    src = th.zeros(4, 3, 8, 8, dtype=th.uint8, device=device)
    arena = th.zeros(2 * 4 * 3 * 64, dtype=th.uint8, device=device)
    dst = arena[: 4 * 3 * 64]
    dstf = th.zeros(4 * 3 * 64, dtype=th.float32, device=device)
    rec = th.zeros(4, 3, 4, dtype=th.int64, device=device)
    par = th.tensor([_row(beta=6000)] * 4, dtype=th.int32, device=device)
    coef = th.zeros(4, 3, 4, dtype=th.int32, device=device)
    s, d, f, r, p, q = (t.data_ptr() for t in (src, dst, dstf, rec, par, coef))
    user = (C.c_double * 6)(0.5, 0.25, 0.5, 0.25, 0.5, 0.25)
    zero_s = (C.c_double * 6)(0.5, 0.25, 0.5, 0.0, 0.5, 0.25)

    def call(src_p=s, n_src=4, rows=None, rec_p=r, par_p=p, form=0, mode=0, usr=None, batch=4, c=3, h=8, w=8, elt=1,
             dst_p=d, coef_p=q):
        rc = lib.marl_batch_color(src_p, n_src, rows, rec_p, par_p, form, mode, usr, batch, c, h, w, elt, dst_p, coef_p,
                                  None)
        return rc, lib.marl_last_error().decode()

    for kw, word in ((dict(src_p=None), "null"), (dict(dst_p=None), "null"), (dict(par_p=None), "null"),
                     (dict(c=2), "neither 1 nor 3"), (dict(elt=2), "elt_bytes"), (dict(form=3), "out_form"),
                     (dict(form=1, mode=4, usr=user, elt=4, dst_p=f), "uint8"),
                     (dict(form=1, mode=1, usr=user, dst_p=f), "statistic"),
                     (dict(form=1, mode=4, usr=None, dst_p=f), "needs user"),
                     (dict(form=1, mode=4, usr=zero_s, dst_p=f), "s must"),
                     (dict(batch=0), "positive"), (dict(n_src=0), "positive"), (dict(h=-1), "positive"),
                     (dict(w=0), "positive"), (dict(n_src=3), "n_src"), (dict(src_p=s + 2, elt=4, w=2), "aligned"),
                     (dict(form=1, mode=4, usr=user, dst_p=f + 2), "aligned"), (dict(rec_p=r + 4), "records"),
                     (dict(coef_p=q + 2), "coef"), (dict(par_p=p + 2), "params"), (dict(dst_p=s), "overlaps"),
                     (dict(src_p=d + 4 * 3 * 64 - 1), "overlaps")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("marl_batch_color:") and word in msg, (kw, rc, msg)
    for kw in (dict(c=3, h=32768, w=32768), dict(form=1, mode=4, usr=user, dst_p=f, c=3, h=16384, w=16384)):
        rc, msg = call(**kw)
        assert rc == -2 and "2^31" in msg, (kw, rc, msg)
    th.cuda.synchronize(device)
    assert not dst.any() and not dstf.any() and not coef.any(), "a refused call wrote"
    # the source directly behind the destination is no overlap; after all those refusals the entry still runs
    src.copy_(source((3, 8, 8), th.uint8, n=4))
    tail = arena[4 * 3 * 64:].view(src.shape)
    tail.copy_(src)
    assert call(src_p=tail.data_ptr(), rec_p=None)[0] == 0
    th.cuda.synchronize(device)
    want = color.reference_apply(src.cpu(), None, par.cpu())
    assert th.equal(dst.view(4, 3, 8, 8).cpu(), want)
    with pytest.raises(RuntimeError, match="GPU"):
        color.apply(src.cpu(), None, par.cpu())
    with pytest.raises(ValueError, match="params"):
        color.apply(src, None, par[:3])
    with pytest.raises(ValueError, match="records"):
        color.apply(src, None, par, rec.double())
    with pytest.raises(ValueError, match="out"):
        color.apply(src, None, par, out=th.empty(4, 3, 8, 8, dtype=th.float32, device=device))
    with pytest.raises(RuntimeError, match="neither 1 nor 3"):
        color.apply(th.zeros(2, 2, 4, 4, dtype=th.uint8, device=device), None, par[:2].contiguous())


def test_draws_need_no_host_synchronisation(device):
    pol = color.parse("brightness:0.4,contrast:0.4,saturation:0.4,hue:0.1,gray:0.2")
    gen = th.Generator(device=device).manual_seed(3)
    pol.draw(8, gen)  # (warm-up: lazy initialisation may synchronise)
    th.cuda.synchronize(device)
    th.cuda.set_sync_debug_mode("error")
    try:
        params = pol.draw(64, gen)
    finally:
        th.cuda.set_sync_debug_mode("default")
    assert params.device.type == "cuda" and params.dtype == th.int32 and params.shape == (64, 8)
    twin = th.Generator(device=device).manual_seed(3)
    pol.draw(8, twin)
    assert th.equal(params, pol.draw(64, twin))
    p = params.cpu()
    assert int(p[:, :3].min()) >= 0 and int(p[:, :3].max()) <= round(1.4 * Q12) and not p[:, 5:].any()


# ---- the loaders ------------------------------------------------------------------------------------------------------
AUG = "d4,shift:2:zero,erase:5:0.7"
JITTER = "brightness:0.4,contrast:0.5,saturation:0.6,hue:0.08,gray:0.2"


def _expected(policy, spec, x, params):
    """the definition of what a loader makes of the uint8 batch x (CPU) under params"""
    rec = transforms.reference_stats(x) if policy.needs_stats else None
    if spec is not None and transforms.parse(spec).is_user:
        return color.reference_apply(x, None, params, rec, normalize=spec)
    y = color.reference_apply(x, None, params, rec)
    return y if spec is None else transforms.reference_apply(y, None, spec)


def test_resident_loader_jitters_plain_and_augmented_batches(device):
    from marlclassification_amd import data
    from marlclassification_amd.data import ResidentLoader, SyntheticImages
    from marlclassification_amd.train import ShardedBatchSampler

    ds = SyntheticImages(37, 3, 16, 5, seed=3)
    part = th.randperm(37, generator=th.Generator().manual_seed(1))[:31].tolist()
    bs = ShardedBatchSampler(part, 8, 0, 1, shuffle=True, seed=2)
    aug, jitter = augment.parse(AUG), color.parse(JITTER)

    def loader(seed=77, **kw):
        if kw:
            kw["generator"] = th.Generator(device=device).manual_seed(seed)
        return ResidentLoader(ds, part, bs, device, **kw)

    plain = list(loader())
    for (x, y), idx in zip(plain, list(bs)):
        assert th.equal(x.cpu(), ds.x[idx]) and th.equal(y.cpu(), ds.y[idx])
    for spec in (None, "channel-normal", _user(3)[0]):
        ld = loader(color=jitter, normalize=spec)
        twin = th.Generator(device=device).manual_seed(77)
        for (x, y), (x0, y0) in zip(list(ld), plain):
            params = jitter.draw(x0.shape[0], twin).cpu()
            assert th.equal(y, y0) and x.dtype == (th.uint8 if spec is None else th.float32)
            assert _same(x.cpu(), _expected(jitter, spec, x0.cpu(), params)), spec
    # behind an augment policy: ops first, colour last, from one generator
    before = list(loader(augment=aug))
    for spec in (None, "channel-normal", _user(3)[1]):
        ld = loader(augment=aug, color=jitter, normalize=spec)
        got = list(ld)
        twin = th.Generator(device=device).manual_seed(77)
        for k, ((x, y), idx) in enumerate(zip(got, list(bs))):
            rows = ld._row_of[th.tensor(idx, device=device)]
            view = data._augmented(aug, twin, ld._x, rows)
            params = jitter.draw(len(idx), twin).cpu()
            assert _same(x.cpu(), _expected(jitter, spec, view.cpu(), params)), spec
            if k == 0:  # (the first batch's ops are drawn before any colour draw: the batch the loader made before)
                assert th.equal(view, before[0][0])
    # a loader without color= draws exactly as before
    twin = th.Generator(device=device).manual_seed(77)
    for (x, y), idx in zip(before, list(bs)):
        assert th.equal(x, data._augmented(aug, twin, ld._x, ld._row_of[th.tensor(idx, device=device)]))
    # a loader with only color= gets a device generator like the others
    alone = ResidentLoader(ds, part, bs, device, color=jitter)
    assert alone.generator is not None and alone.generator.device.type == "cuda"
    first = next(iter(alone))[0]
    params = jitter.draw(plain[0][0].shape[0], th.Generator(device=device).manual_seed(0)).cpu()
    assert th.equal(first.cpu(), _expected(jitter, None, plain[0][0].cpu(), params))


def test_device_prefetcher_jitters_plain_and_augmented_batches(device):
    from torch.utils.data import DataLoader

    from marlclassification_amd import data, mix
    from marlclassification_amd.data import DevicePrefetcher, SyntheticImages

    ds = SyntheticImages(20, 1, 28, 10, seed=4)
    dl = DataLoader(ds, batch_size=8, shuffle=False)
    aug, jitter = augment.parse(AUG), color.parse("brightness:0.5,contrast:0.5")

    def loader(**kw):
        if kw:
            kw["generator"] = th.Generator(device=device).manual_seed(5)
        return DevicePrefetcher(dl, device, **kw)

    plain = list(loader())
    for k, (x, y) in enumerate(plain):
        assert th.equal(x.cpu(), ds.x[8 * k: 8 * k + 8])
    for spec in (None, "minmax", "user-normal:0.4:0.25"):
        twin = th.Generator(device=device).manual_seed(5)
        for (x, y), (x0, y0) in zip(list(loader(color=jitter, normalize=spec)), plain):
            params = jitter.draw(x0.shape[0], twin).cpu()
            assert th.equal(y, y0) and _same(x.cpu(), _expected(jitter, spec, x0.cpu(), params)), spec
    twin = th.Generator(device=device).manual_seed(5)
    for (x, y), (x0, y0) in zip(list(loader(augment=aug, color=jitter, normalize="channel-normal")), plain):
        view = data._augmented(aug, twin, x0, None)
        params = jitter.draw(x0.shape[0], twin).cpu()
        assert _same(x.cpu(), _expected(jitter, "channel-normal", view.cpu(), params))
    # behind a mix policy the labels and targets are those of the loader without colour
    mp = mix.parse("cutmix:1.0")
    for (x, y, q), (x0, y0, q0) in zip(list(loader(mix=mp, nb_class=10, color=jitter))[:1],
                                       list(loader(mix=mp, nb_class=10))[:1]):
        assert th.equal(y, y0) and th.equal(q, q0) and x.shape == x0.shape and x.dtype == th.uint8
    assert th.equal(list(loader(augment=aug))[0][0],
                    data._augmented(aug, th.Generator(device=device).manual_seed(5), plain[0][0], None))


# ---- through the trainer and the command line -------------------------------------------------------------------------
ACTIONS = [[1, 0], [-1, 0], [0, 1], [0, -1]]


def test_a_train_step_on_a_jittered_batch_equals_the_step_on_the_definitions_tensor(device):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import MnistCnn
    from marlclassification_amd.training import Trainer

    resident = source((1, 28, 28), th.uint8, seed=21)
    rows = th.tensor([10, 0, 3, 3, 7, 1, 9, 2])
    params = color.parse("brightness:0.4,contrast:0.6").draw(8, th.Generator().manual_seed(2))
    y = th.randint(0, 10, (8,), generator=th.Generator().manual_seed(4)).to(device)
    spec = "user-normal:0.4:0.25"
    rec = transforms.reference_stats(resident, rows)
    want = color.reference_apply(resident, rows, params, rec, normalize=spec)
    fused_x = color.apply(resident.to(device), rows.to(device), params.to(device), rec.to(device), out_form="norm",
                          normalize=spec)
    assert th.equal(_bits(fused_x.cpu()), _bits(want)), "the two steps would not see the same bytes"
    weights = []
    for x in (fused_x, want.to(device)):
        th.manual_seed(99)
        model = ModelsWrapper(MnistCnn(6), 32, 32, 8, 12, 8, 2, 4, 10, 48, 48).to(device)
        sampler = EpisodeSampler(MultiAgent(3, model), Environment(ACTIONS, 6), 4)
        Trainer(model, 10, 1e-3, 0.99).train_step(x, y, sampler)
        th.cuda.synchronize(device)
        weights.append({n: p.detach().clone() for n, p in model.named_parameters()})
    assert weights[0].keys() == weights[1].keys()
    for n in weights[0]:
        assert th.equal(weights[0][n], weights[1][n]), n


def test_train_color_from_the_command_line(device, tmp_path, capsys, monkeypatch):
    from marlclassification_amd import color as color_mod
    from marlclassification_amd.__main__ import main

    calls = []
    real_apply = color_mod.apply
    monkeypatch.setattr(color_mod, "apply", lambda src, rows, params, *a, **kw: (
        calls.append((rows is not None, a[0] is not None if a else kw.get("records") is not None)),
        real_apply(src, rows, params, *a, **kw))[1])
    out = str(tmp_path / "run")
    main(["--run-id", "r", "-a", "3", "--step", "3", "--cuda", "train", "--res-folder", "synthetic", "--nb-epoch", "1",
          "--batch-size", "8", "--nb-class", "3", "--color", "brightness:0.3,contrast:0.3", "-o", out])
    text = capsys.readouterr().out
    assert "color brightness:0.3,contrast:0.3" in text
    assert "color" not in json.load(open(os.path.join(out, "marl.json")))
    assert os.path.exists(os.path.join(out, "models", "nn_models_epoch_0.pt"))
    # the training split only (54 of 64 synthetic images in batches of 8: seven batches; the synthetic set is streamed,
    # so the uploaded batch is jittered as it is), with the records contrast needs
    assert len(calls) == 7 and all(c == (False, True) for c in calls)
