"""GPU: the resampling batch gather ``marl_batch_warp`` (``warp.apply``) against its definition
``warp.reference_apply`` on the CPU.  The map, the fold and the uint8 blend are integers and the fp32 blend is made of
separately rounded products and sums, so every comparison is ``torch.equal`` - uint8 and fp32 (compared as bit
patterns) alike.  Shapes are the smallest that reach every store width and more than one workgroup per image, plus the
benchmark shape; each case asserts the store width ``marl_batch_warp_plan`` reports.  Every destination sits inside a
larger buffer whose guard bytes must survive, and every source inside a frame of rows holding a value that no blend of
image pixels and the fill can produce."""
import ctypes as C
import json
import math

import pytest
import torch as th

from marlclassification_amd import augment, warp
from tests.buffers import SENTINEL
from tests.buffers import guarded as _guarded
from tests.buffers import guards_intact as _guards_intact
from tests.buffers import same_bits as _same_bits

pytestmark = pytest.mark.gpu

N_SRC = 7
FRAME = 2  # rows in front of and behind the source rows
FILL = {th.uint8: 250, th.float32: -1.5}
ONE = warp.ONE
EINVAL, ELIMIT = -1, -2  # MARL_EINVAL, MARL_ELIMIT of include/marl_hip.h

# shape -> (batch, store bytes uint8, store bytes fp32) with a 16-byte aligned destination
SHAPES = {
    (1, 5, 7): (9, 1, 4),        # byte stores; 4-byte fp32 rows
    (1, 1, 1): (4, 1, 4),        # the n == 1 fold
    (2, 9, 4): (16, 4, 16),      # 4-byte uint8 rows, one 16-byte fp32 store per row
    (3, 16, 16): (8, 16, 16),    # 16-byte stores
    (3, 33, 33): (6, 1, 4),      # ragged: byte / 4-byte stores, a last workgroup that is not full
    (3, 64, 64): (4, 16, 16),    # more than one workgroup per image (fp32: 4)
    (3, 256, 256): (2, 16, 16),  # the benchmark shape (uint8: 16 workgroups per image, fp32: 64)
}
IDS = ["x".join(map(str, s)) for s in SHAPES]
DTYPES = pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])


def _framed(shape, dtype, device, n=N_SRC, seed=0):
    """(source rows on the CPU, the same rows on the device as a view into a buffer with FRAME marked rows around them).
    uint8 images hold [16, 240), the frame 0: no convex blend of image pixels and FILL gives less than 16.  fp32 images
    are normal draws, the frame 1e30."""
    g = th.Generator().manual_seed(seed + 131 * shape[1] + shape[2])
    if dtype == th.uint8:
        src = th.randint(16, 240, (n,) + tuple(shape), dtype=th.uint8, generator=g)
        whole = th.zeros((n + 2 * FRAME,) + tuple(shape), dtype=th.uint8)
    else:
        src = th.randn((n,) + tuple(shape), generator=g)
        whole = th.full((n + 2 * FRAME,) + tuple(shape), 1e30)
    whole[FRAME: FRAME + n] = src
    whole_d = whole.to(device)
    return src, whole_d[FRAME: FRAME + n]


def _nothing_from_the_frame(got):
    if got.dtype == th.uint8:
        return bool((got >= 16).all())
    return bool((got.abs() < 1e6).all())


def _random_mats(nb, h, w, seed):
    """rotation over the whole circle x zoom in [1/2, 2] x stretch in [2/3, 3/2], translations of up to half the image
    drawn as integers in Q16 half pixels, so every weight 0 .. 255 occurs"""
    g = th.Generator().manual_seed(seed)
    u = th.rand(3, nb, generator=g)
    mats = warp.matrices(360.0 * u[0] - 180.0, th.exp((2 * u[1] - 1) * math.log(2.0)),
                         th.exp((2 * u[2] - 1) * math.log(1.5)))
    mats[:, 4] = th.randint(-h * ONE, h * ONE + 1, (nb,), generator=g, dtype=th.int32)
    mats[:, 5] = th.randint(-w * ONE, w * ONE + 1, (nb,), generator=g, dtype=th.int32)
    return mats


def _rows(nb, seed):
    return th.randint(0, N_SRC, (nb,), generator=th.Generator().manual_seed(seed))


def _check(device, shape, dtype, mats, ops=None, rows="random", offset=0, want_store=None, modes=("reflect", "zero"),
           framed=None):
    """``warp.apply`` into a guarded destination against ``warp.reference_apply``, both pad modes"""
    src, src_d = framed if framed is not None else _framed(shape, dtype, device)
    nb = mats.shape[0]
    if isinstance(rows, str):
        rows = _rows(nb, 17 + nb)
    out_shape = (nb,) + tuple(shape)
    nbytes = th.Size(out_shape).numel() * src.element_size()
    buf, dst = _guarded(out_shape, dtype, device, offset)
    if want_store is not None:
        info = warp.plan(src_d, dst)
        assert info["store_bytes"] == want_store and info["lds_bytes"] == 0, info
        assert info["pixels_per_thread"] * src.element_size() == want_store, info
    for mode in modes:
        buf.fill_(SENTINEL)
        got = warp.apply(src_d, None if rows is None else rows.to(device), mats.to(device),
                         None if ops is None else ops.to(device), pad_mode=mode, fill=FILL[dtype], out=dst)
        assert got is dst
        want = warp.reference_apply(src, rows, mats, ops, mode, FILL[dtype])
        got_h = dst.cpu()
        if not _same_bits(got_h, want):
            bad = [(b, mats[b].tolist()) for b in range(nb) if not _same_bits(got_h[b], want[b])]
            pytest.fail(f"{shape} {dtype} {mode}: images differ under mats {bad}")
        assert _guards_intact(buf, offset, nbytes), f"{shape} {dtype} {mode}: guard bytes overwritten"
        assert _nothing_from_the_frame(got_h), f"{shape} {dtype} {mode}: a pixel from outside the source rows"
    return dst


# ---- the kernel against the definition ------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("shape", list(SHAPES), ids=IDS)
def test_random_rotation_zoom_stretch_and_fractional_translation(device, shape, dtype):
    nb, *stores = SHAPES[shape]
    mats = _random_mats(nb, shape[1], shape[2], seed=5 + shape[1])
    _check(device, shape, dtype, mats, want_store=stores[dtype == th.float32])
    # the fractional cases must be fractional: weights other than 0 in both axes
    m = mats.to(th.int64)
    assert bool(((m[:, 4] % (2 * ONE)) != 0).any()) and bool(((m[:, 0].abs() != ONE) | (m[:, 1] != 0)).any())


@DTYPES
@pytest.mark.parametrize("shape", list(SHAPES), ids=IDS)
def test_identity_is_index_select(device, shape, dtype):
    nb = SHAPES[shape][0]
    src, src_d = _framed(shape, dtype, device)
    rows = _rows(nb, 3)
    for mode in ("reflect", "zero"):
        got = warp.apply(src_d, rows.to(device), warp.identity(nb, device), pad_mode=mode, fill=FILL[dtype])
        assert _same_bits(got, src_d.index_select(0, rows.to(device))), mode


@DTYPES
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 9, 4), (3, 16, 16), (3, 33, 33), (1, 1, 1)],
                         ids=["1x5x7", "2x9x4", "3x16x16", "3x33x33", "1x1x1"])
def test_every_d4_code_under_extreme_shifts_equals_augment_apply(device, shape, dtype):
    """the eight codes (four on non-square images) x shifts up to +-(H-1), +-(W-1): the matrices of ``from_ops`` give
    the bits of ``marl_batch_augment`` and of ``augment.reference_apply``; handed over as ``ops`` they are folded into
    the matrices by ``apply``"""
    c, h, w = shape
    codes = range(8) if h == w else (0, 2, 4, 6)
    shifts = ((0, 0), (h - 1, w - 1), (-(h - 1), -(w - 1)), (-(h - 1), min(2, w - 1)), (h // 2, -(w // 3)))
    ops = th.tensor([[d, dy, dx, 0, 0, 0, 0, 0] for d in codes for dy, dx in shifts], dtype=th.int32)
    nb = ops.shape[0]
    rows = _rows(nb, 9)
    src, src_d = _framed(shape, dtype, device)
    mats = warp.from_ops(ops, h, w)
    assert set(mats[:, :4].abs().flatten().tolist()) <= {0, ONE}
    for mode in ("reflect", "zero"):
        want = augment.reference_apply(src, rows, ops, mode, FILL[dtype])
        plain = augment.apply(src_d, rows.to(device), ops.to(device), pad_mode=mode, fill=FILL[dtype])
        got = warp.apply(src_d, rows.to(device), mats.to(device), pad_mode=mode, fill=FILL[dtype])
        folded = warp.apply(src_d, rows.to(device), warp.identity(nb, device), ops.to(device), pad_mode=mode,
                            fill=FILL[dtype])
        assert _same_bits(plain.cpu(), want) and _same_bits(got, plain) and _same_bits(folded, plain), mode


@DTYPES
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 33, 33), (3, 64, 64)], ids=["1x5x7", "3x33x33", "3x64x64"])
def test_zoom_limits_and_translations_far_outside(device, shape, dtype):
    """zoom 1/16 (the fold runs over many periods of the image: the dividing path) and 16, alone and rotated; the
    translation limits +-2^30, where every tap lies 8192 pixels outside"""
    c, h, w = shape
    z = th.tensor([1 / 16, 16.0, 1 / 16, 16.0, 1.0, 1.0, 1.0, 1.0])
    a = th.tensor([0.0, 0.0, 31.0, -74.0, 0.0, 0.0, 45.0, 0.0])
    mats = warp.matrices(a, z, th.ones(8))
    far = 1 << 30
    mats[4, 4], mats[5, 5], mats[6, 4], mats[6, 5], mats[7, 4], mats[7, 5] = far, -far, -far, far, far - 12345, -far + 777
    assert mats[0, 0] == 16 * ONE and mats[1, 0] == ONE // 16
    _check(device, shape, dtype, mats)


@DTYPES
@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 33, 33), (3, 64, 64)], ids=["3x16x16", "3x33x33", "3x64x64"])
def test_rectangle_over_workgroup_and_vector_edges_full_and_empty(device, shape, dtype):
    c, h, w = shape
    rects = [(0, 0, h, w), (2, 3, 0, 5), (2, 3, 5, 0), (h - 3, w - 5, 9, 9), (-4, -4, 7, 9), (1, 13, 3, 6),
             (h // 2 - 3, 3, 7, 2), (0, w - 1, h, 1)]
    if h == 64:
        rects += [(14, 10, 4, 40), (15, 63, 2, 1), (31, 0, 2, 64), (47, 15, 3, 2)]  # fp32 workgroups end at rows 16 k
    ops = th.tensor([[0, 0, 0, ey, ex, eh, ew, 0] for ey, ex, eh, ew in rects], dtype=th.int32)
    mats = _random_mats(ops.shape[0], h, w, seed=23)
    dst = _check(device, shape, dtype, mats, ops)
    assert bool((dst[0] == FILL[dtype]).all())  # the full rectangle
    # under a dihedral code and a shift in the same op rows: "warp, then view", the rectangle stays in output space
    ops[:, 0] = th.arange(ops.shape[0]) % 8
    ops[:, 1], ops[:, 2] = 2, -3
    _check(device, shape, dtype, mats, ops)


def test_nan_and_inf_behind_zero_weights_stay_out(device):
    """fp32: a tap of weight 0 is skipped, not multiplied.  Whole-pixel maps (flips, shifts, a quarter turn) of an image
    with NaN and Inf pixels move them and spread nothing; a half-pixel shift along x alone keeps rows apart."""
    shape = (2, 9, 12)
    g = th.Generator().manual_seed(4)
    src = th.randn((3,) + shape, generator=g)
    src[:, :, 2, 5], src[:, :, 7, 0], src[:, :, 4, 11] = float("nan"), float("inf"), float("-inf")
    src_d = src.to(device)
    ops = th.tensor([[0, 0, 0], [2, 1, -2], [4, -3, 4], [6, 8, 11]], dtype=th.int32)
    ops = th.cat([ops, th.zeros(4, 5, dtype=th.int32)], dim=1)
    mats = warp.from_ops(ops, 9, 12)
    half = warp.identity(1)
    half[0, 5] = ONE  # x + 1/2: fy == 0 everywhere
    mats = th.cat([mats, half])
    rows = th.tensor([0, 1, 2, 0, 1])
    for mode in ("reflect", "zero"):
        got = warp.apply(src_d, rows.to(device), mats.to(device), pad_mode=mode, fill=0.25).cpu()
        want = warp.reference_apply(src, rows, mats, None, mode, 0.25)
        assert th.equal(got.isnan(), want.isnan())
        assert th.equal(got.nan_to_num(nan=7.0).view(th.int32), want.nan_to_num(nan=7.0).view(th.int32))
        assert int(got[0].isnan().sum()) == 2 and int(got[0].isinf().sum()) == 4  # moved, not spread
        rows_hit = got[4].isnan().any(dim=2) | got[4].isinf().any(dim=2)  # [C, H]: the rows 2, 4, 7 only
        assert rows_hit.nonzero()[:, 1].unique().tolist() == [2, 4, 7]


@DTYPES
@pytest.mark.parametrize("shape", [(3, 64, 64), (2, 9, 4)], ids=["3x64x64", "2x9x4"])
def test_hostile_device_values_are_sanitised(device, shape, dtype):
    big = 2**31 - 1
    mats = th.tensor([[big, big, big, big, big, big, 9, 9],
                      [-big - 1, -big - 1, -big - 1, -big - 1, -big - 1, -big - 1, -1, -1],
                      [big, -big, 0, 0, -big, big, 0, 0],
                      [0, 0, 0, 0, 0, 0, 0, 0],
                      [ONE, 0, 0, ONE, big, -big - 1, 0, 0],
                      [(1 << 20) + 1, 1, -1, -(1 << 20) - 1, (1 << 30) + 1, -(1 << 30) - 1, 0, 0],
                      [ONE, 0, 0, ONE, 0, 0, big, big],
                      [-3, 7, 11, -5, 1, -1, 0, 0]], dtype=th.int32)
    rows = th.tensor([-1, N_SRC + 1, N_SRC, 3, -2**40, 2**40, N_SRC - 1, 0])
    c, h, w = shape
    ops = th.tensor([[0, 0, 0, big, big, big, big, 0], [0, 0, 0, -big - 1, -big - 1, big, big, 0],
                     [0, 0, 0, 1, 1, -big - 1, 5, 0], [0, 0, 0, h - 2, w - 3, 9, 9, 0],
                     [0, 0, 0, -4, -4, 7, 7, 0], [0, 0, 0, 2, 2, -3, 4, 0], [0, 0, 0, 0, 0, 0, 0, 5],
                     [0, 0, 0, h + 2, w + 2, 3, 3, 0]], dtype=th.int32)
    _check(device, shape, dtype, mats, None, rows)
    _check(device, shape, dtype, mats, ops, rows)


@DTYPES
@pytest.mark.parametrize("shape,store", [((3, 64, 64), 4), ((3, 16, 16), 4), ((1, 5, 7), None)],
                         ids=["3x64x64", "3x16x16", "1x5x7"])
def test_destination_offset_by_four_bytes_takes_narrow_stores(device, shape, dtype, store):
    if store is None:
        store = 1 if dtype == th.uint8 else 4
    _check(device, shape, dtype, _random_mats(5, shape[1], shape[2], seed=31), offset=4, want_store=store)
    if shape == (3, 64, 64):
        _check(device, shape, dtype, _random_mats(5, 64, 64, seed=32), offset=8, want_store=8)


@DTYPES
def test_null_rows_null_ops_and_argument_checks(device, dtype):
    shape = (3, 16, 16)
    src, src_d = _framed(shape, dtype, device)
    mats = _random_mats(N_SRC, 16, 16, seed=41)
    _check(device, shape, dtype, mats, rows=None)  # rows == NULL: row b for image b (an uploaded batch)
    mats_d = mats.to(device)
    with pytest.raises(RuntimeError, match="overlaps"):
        warp.apply(src_d, None, mats_d, out=src_d)
    with pytest.raises(RuntimeError, match="n_src"):
        warp.apply(src_d[:3], None, mats_d)
    with pytest.raises(TypeError):
        warp.apply(src_d.to(th.float64), None, mats_d)
    with pytest.raises(ValueError, match="mats"):
        warp.apply(src_d, None, mats_d.long())
    with pytest.raises(ValueError, match="mats"):
        warp.apply(src_d, None, mats)  # on the CPU
    with pytest.raises(ValueError, match="rows"):
        warp.apply(src_d, th.zeros(N_SRC, dtype=th.int32, device=device), mats_d)
    with pytest.raises(ValueError, match="ops"):
        warp.apply(src_d, None, mats_d, th.zeros(N_SRC, 7, dtype=th.int32, device=device))
    with pytest.raises(ValueError, match="pad mode"):
        warp.apply(src_d, None, mats_d, pad_mode="wrap")
    with pytest.raises(RuntimeError, match="GPU"):
        warp.apply(src, None, mats)
    assert warp.apply(src_d, None, mats_d[:0]).shape == (0,) + shape


def test_every_guard_of_the_c_entry(device):
    from marlclassification_amd import _lib

    lib = _lib.load()
    src = th.zeros(4, 3, 8, 8, dtype=th.uint8, device=device)
    dst = th.zeros(4, 3, 8, 8, dtype=th.uint8, device=device)
    mats = warp.identity(4, device)
    s, d, m = src.data_ptr(), dst.data_ptr(), mats.data_ptr()

    def call(src_p=s, n_src=4, dst_p=d, mats_p=m, batch=4, c=3, h=8, w=8, elt=1, pad=1, rows_p=None):
        rc = lib.marl_batch_warp(src_p, n_src, dst_p, rows_p, mats_p, None, batch, c, h, w, elt, pad, 0, None)
        return rc, lib.marl_last_error().decode()

    assert call()[0] == 0
    for kw, word in ((dict(src_p=None), "null"), (dict(dst_p=None), "null"), (dict(mats_p=None), "mats"),
                     (dict(elt=2), "elt_bytes"), (dict(pad=2), "pad_mode"), (dict(batch=0), "positive"),
                     (dict(n_src=0), "positive"), (dict(c=0), "positive"), (dict(h=-1), "positive"),
                     (dict(w=0), "positive"), (dict(n_src=3), "n_src"), (dict(dst_p=s), "overlaps"),
                     (dict(src_p=s + 1, dst_p=d + 2, elt=4, w=2), "aligned")):
        rc, msg = call(**kw)
        assert rc == EINVAL and "marl_batch_warp" in msg and word in msg, (kw, rc, msg)
    rc, msg = call(c=2, h=32768, w=32768)  # 2^31 bytes
    assert rc == ELIMIT and "2^31" in msg, (rc, msg)
    # two workgroups an image: the grid does not fit (nothing is launched, so rows is never read; the lower of two
    # one-image buffers is the source, so that the huge destination range does not reach it)
    one = [th.zeros(1, 1, 32, 256, dtype=th.uint8, device=device) for _ in range(2)]
    lo, hi = sorted(t.data_ptr() for t in one)
    rc, msg = call(src_p=lo, n_src=1, dst_p=hi, rows_p=m, batch=2**31 - 1, c=1, h=32, w=256)
    assert rc == ELIMIT and "workgroups" in msg, (rc, msg)
    info = warp.WarpPlan()
    assert lib.marl_batch_warp_plan(3, 8, 8, 1, s, d, None) == EINVAL
    assert lib.marl_batch_warp_plan(3, 8, 8, 3, s, d, C.byref(info)) == EINVAL
    assert lib.marl_batch_warp_plan(3, 8, 8, 1, None, d, C.byref(info)) == 0 and info.store_bytes == 8
    th.cuda.synchronize(device)


def test_source_offsets_are_64_bit(device):
    """A uint8 set of more than 2^32 bytes (nothing filled but the rows used): the last row and row 0."""
    n, shape = 21846, (3, 256, 256)
    assert n * 3 * 256 * 256 > 2**32
    big = th.empty((n,) + shape, dtype=th.uint8, device=device)
    two = th.randint(0, 256, (2,) + shape, dtype=th.uint8, generator=th.Generator().manual_seed(9))
    big[n - 1].copy_(two[0])
    big[0].copy_(two[1])
    mats = _random_mats(3, 256, 256, seed=51)
    mats[:, 4:6] //= 8
    rows = th.tensor([n - 1, 0, n - 1])
    got = warp.apply(big, rows.to(device), mats.to(device), fill=1)
    want = warp.reference_apply(two, th.tensor([0, 1, 0]), mats, fill=1)
    assert th.equal(got.cpu(), want)
    del big
    th.cuda.empty_cache()


def test_two_runs_give_the_same_bits_and_a_side_stream_is_respected(device):
    shape = (3, 64, 64)
    src, src_d = _framed(shape, th.float32, device)
    mats, rows = _random_mats(5, 64, 64, seed=61), _rows(5, 62)
    rows_d, mats_d = rows.to(device), mats.to(device)
    a = warp.apply(src_d, rows_d, mats_d, fill=-1.5)
    b = warp.apply(src_d, rows_d, mats_d, fill=-1.5)
    assert _same_bits(a, b)
    want = warp.reference_apply(src, rows, mats, fill=-1.5)
    # the source is produced on a side stream behind some work; the launch must queue behind it on that stream
    side = th.cuda.Stream(device=device)
    late = th.zeros_like(src_d)
    m = th.randn(2048, 2048, device=device)
    th.cuda.synchronize(device)
    with th.cuda.stream(side):
        for _ in range(8):
            m = (m @ m).clamp_(-1.0, 1.0)
        late.copy_(src_d)
        got = warp.apply(late, rows_d, mats_d, fill=-1.5)
    side.synchronize()
    assert _same_bits(got.cpu(), want)


# ---- the loaders ----------------------------------------------------------------------------------------------------
SPEC = "d4,rotate:30,scale:0.7:1.4,stretch:1.3,shift:2:zero,erase:5:0.7"


def test_draw_warp_and_a_warped_resident_batch_make_no_host_synchronisation(device):
    from marlclassification_amd.data import ResidentLoader, SyntheticImages

    ds = SyntheticImages(24, 3, 16, 5, seed=3)
    policy = augment.parse(SPEC)
    assert policy.has_warp
    g = th.Generator(device=device).manual_seed(3)
    rl = ResidentLoader(ds, range(24), [list(range(8)), list(range(8, 16))], device, augment=policy, generator=g)
    first = next(iter(rl))  # (fills the resident set: that does synchronise, once)
    th.cuda.synchronize(device)
    th.cuda.set_sync_debug_mode("error")
    try:
        drawn = [augment.parse(s).draw_warp(64, g, size=(16, 16))
                 for s in ("rotate:10", "scale:0.5:2", "stretch:2", "hflip,rotate:180", SPEC)]
        batches = list(rl)
    finally:
        th.cuda.set_sync_debug_mode("default")
    assert len(batches) == 2 and batches[0][0].shape == first[0].shape == (8, 3, 16, 16)
    for ops, mats in drawn:
        assert ops.shape == mats.shape == (64, 8) and ops.dtype == mats.dtype == th.int32 and mats.is_cuda
    zoom_only = drawn[1][1].cpu()
    assert bool((zoom_only[:, 1] == 0).all()) and ONE // 2 <= int(zoom_only[:, 0].min()) <= int(zoom_only[:, 0].max()) <= 2 * ONE


def test_both_loaders_yield_the_reference_of_the_matrices_they_drew(device):
    from torch.utils.data import DataLoader

    from marlclassification_amd import mix
    from marlclassification_amd.data import DevicePrefetcher, ResidentLoader, SyntheticImages
    from marlclassification_amd.train import ShardedBatchSampler

    policy = augment.parse(SPEC)
    ds = SyntheticImages(37, 3, 16, 5, seed=3)
    part = th.randperm(37, generator=th.Generator().manual_seed(1))[:31].tolist()
    bs = ShardedBatchSampler(part, 8, 0, 1, shuffle=True, seed=2)
    rl = ResidentLoader(ds, part, bs, device, augment=policy, generator=th.Generator(device=device).manual_seed(77))
    twin = th.Generator(device=device).manual_seed(77)
    bs.set_epoch(0)
    seen = 0
    for (x, y), idx in zip(list(rl), list(bs)):
        ops, mats = (t.cpu() for t in policy.draw_warp(len(idx), twin, size=(16, 16)))
        assert th.equal(x.cpu(), warp.reference_apply(ds.x, th.tensor(idx), mats, ops, "zero", 0))
        assert th.equal(y.cpu(), ds.y[idx])
        seen += 1
    assert seen > 1
    ds1 = SyntheticImages(20, 1, 28, 10, seed=4)
    dl = DataLoader(ds1, batch_size=8, shuffle=False)
    pf = DevicePrefetcher(dl, device, augment=policy, generator=th.Generator(device=device).manual_seed(5))
    twin = th.Generator(device=device).manual_seed(5)
    for k, (x, y) in enumerate(pf):
        ops, mats = (t.cpu() for t in policy.draw_warp(x.shape[0], twin, size=(28, 28)))
        assert th.equal(x.cpu(), warp.reference_apply(ds1.x[8 * k: 8 * k + 8], None, mats, ops, "zero", 0))
        assert th.equal(y.cpu(), ds1.y[8 * k: 8 * k + 8])
    # mixing warped views is not built: refused where the loader is made; an index-remapping policy still mixes
    for make in (lambda a: ResidentLoader(ds, part, bs, device, augment=a, mix=mix.parse("cutmix"), nb_class=5),
                 lambda a: DevicePrefetcher(dl, device, augment=a, mix=mix.parse("mixup"), nb_class=10)):
        with pytest.raises(ValueError, match="mixing warped views is not built"):
            make(policy)
        make(augment.parse("d4,shift:2"))


# ---- through the trainer and the command line -----------------------------------------------------------------------
ACTIONS = [[1, 0], [-1, 0], [0, 1], [0, -1]]


def _mnist_model(device, seed):
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import MnistCnn

    th.manual_seed(seed)
    return ModelsWrapper(MnistCnn(6), 32, 32, 8, 12, 8, 2, 4, 10, 48, 48).to(device)


def test_a_train_step_on_a_warped_batch_equals_the_step_on_the_materialised_batch(device):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.training import Trainer

    resident = th.randint(0, 256, (11, 1, 28, 28), dtype=th.uint8, generator=th.Generator().manual_seed(21))
    rows = th.tensor([10, 0, 3, 3, 7, 1, 9, 2])
    ops, mats = augment.parse("d4,rotate:25,scale:0.8:1.25,shift:3,erase:6").draw_warp(
        8, th.Generator().manual_seed(3), size=(28, 28))
    y = th.randint(0, 10, (8,), generator=th.Generator().manual_seed(4)).to(device)
    materialised = warp.reference_apply(resident, rows, mats, ops)
    assert not th.equal(materialised, resident[rows])
    params = []
    for fused in (True, False):
        model = _mnist_model(device, 99)
        sampler = EpisodeSampler(MultiAgent(3, model), Environment(ACTIONS, 6), 4)
        trainer = Trainer(model, 10, 1e-3, 0.99)
        x = (warp.apply(resident.to(device), rows.to(device), mats.to(device), ops.to(device)) if fused
             else materialised.to(device))
        trainer.train_step(x, y, sampler)
        th.cuda.synchronize(device)
        params.append({n: p.detach().clone() for n, p in model.named_parameters()})
    assert params[0].keys() == params[1].keys()
    for n in params[0]:
        assert th.equal(params[0][n], params[1][n]), n


def test_tta_over_d4_and_three_zooms_is_the_mean_of_24_explicit_episodes(device, tmp_path):
    import numpy as np
    from PIL import Image
    from torch.utils.data import DataLoader

    from marlclassification_amd.config import EvalConfig, MainConfig, ModelConfig
    from marlclassification_amd.core import EpisodeSampler
    from marlclassification_amd.data import DevicePrefetcher, ImageFolderU8
    from marlclassification_amd.eval import eval_main
    from marlclassification_amd.metrics import ConfusionMeter

    root = tmp_path / "images"
    rng = np.random.default_rng(0)
    for c in range(3):
        (root / f"class{c}").mkdir(parents=True)
        for k in range(7):
            arr = rng.integers(0, 256, (28, 28), dtype=np.uint8)
            arr[4 * c: 4 * c + 8] = 255  # a class-dependent bright band
            Image.fromarray(arr).save(root / f"class{c}" / f"img{k}.png")
    mc = ModelConfig(ft_extr_str="mnist", window_size=6, hidden_size_belief=32, hidden_size_action=32, hidden_size_msg=8,
                     hidden_size_msg_output=12, hidden_size_state=8, state_dim=2, actions=ACTIONS, nb_class=3,
                     hidden_size_linear_belief=48, hidden_size_linear_action=48)
    mc.save_marl_config(str(tmp_path / "marl.json"))
    th.manual_seed(11)
    th.save(mc.build_marl(3)[0].state_dict(), tmp_path / "sd.pt")
    main_config = MainConfig(step=4, run_id="tta", cuda=True, nb_agent=3)
    tta = "d4,zoom:0.8/1/1.25"
    ops, mats = augment.parse_tta(tta).warp_views()
    assert ops.shape == mats.shape == (24, 8) and len({tuple(r) for r in th.cat([ops, mats], 1).tolist()}) == 24

    th.manual_seed(1234)
    got = eval_main(main_config, EvalConfig(
        img_size=28, state_dict_path=str(tmp_path / "sd.pt"), batch_size=8, json_path=str(tmp_path / "marl.json"),
        dataset_path=str(root), output_dir=str(tmp_path / "out"), greedy=True, tta=tta)).conf_mat().cpu()
    # eval_main's own sequence (same seed, same random-number consumption, so the same shuffle and the same episode
    # draws), every view materialised by reference_apply on the CPU
    th.manual_seed(1234)
    dataset = ImageFolderU8(str(root), img_size=28)
    nn_models, marl_m, env = ModelConfig.load_marl_config(str(tmp_path / "marl.json")).build_marl(3)
    nn_models.load_state_dict(th.load(tmp_path / "sd.pt", map_location="cpu"))
    nn_models.eval()
    nn_models.to(device)
    nn_models.set_exploration(temperature=1.0, greedy=True)
    loader = DevicePrefetcher(DataLoader(dataset, batch_size=8, shuffle=True, num_workers=0, drop_last=False,
                                         pin_memory=True), device)
    sampler = EpisodeSampler(marl_m, env, 4)
    meter = ConfusionMeter(3)
    with th.no_grad():
        for x, y in loader:
            pred = None
            for v in range(24):
                xv = warp.reference_apply(x.cpu(), None, mats[v: v + 1].expand(x.shape[0], -1),
                                          ops[v: v + 1].expand(x.shape[0], -1)).to(device)
                p = sampler.run_episode_get_last_step(xv).prediction.mean(dim=0)
                pred = p if pred is None else pred + p
            meter.add(pred / 24, y)
    assert th.equal(got, meter.conf_mat().cpu())
    assert int(got.sum()) == 21
    assert json.loads((tmp_path / "marl.json").read_text()).get("tta") is None


def test_command_line_trains_under_a_warping_augment_spec(device, tmp_path, capsys):
    from marlclassification_amd.__main__ import main

    out = tmp_path / "run"
    spec = "d4,rotate:15,scale:0.8:1.25"
    main((f"-a 3 --step 3 --cuda --run-id w train --ft-extr mnist --f 6 --img-size 28 --nb-class 10 --nb 16 --na 16 "
          f"--nm 8 --nmo 12 --nd 4 --nlb 24 --nla 24 --batch-size 16 --nb-epoch 1 --lr 1e-3 --res-folder synthetic "
          f"--augment {spec} -o {out}").split())
    printed = capsys.readouterr().out
    assert f"augment {spec}" in printed and "epoch 0:" in printed
    cfg = json.loads((out / "marl.json").read_text())
    assert not any(k in cfg for k in ("augment", "rotate", "scale", "warp"))
    sd = th.load(out / "models" / "nn_models_epoch_0.pt", map_location="cpu")
    assert all(bool(th.isfinite(v).all()) for v in sd.values())
    with pytest.raises(ValueError, match="mixing warped views is not built"):
        main((f"-a 3 --step 3 --cuda --run-id w train --ft-extr mnist --f 6 --img-size 28 --res-folder synthetic "
              f"--augment {spec} --mix cutmix -o {out}").split())
