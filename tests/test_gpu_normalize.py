"""GPU: the per-image input normalisation ``marl_batch_stats`` / ``marl_batch_normalize`` (``transforms.stats`` /
``transforms.apply``) against its definition on the CPU (``transforms.reference_stats`` / ``reference_coef`` /
``reference_apply``).

* uint8 records are integers: ``torch.equal``.  fp32 records: min / max exact, the two sums within the worst case of
  summing N fp64 terms in any order, ``2 N 2^-53 sum|term|`` (both sides sum in fp64, in different orders).
* ``coef`` is within 1 fp32 ulp of ``reference_coef``: both sides are correctly rounded fp64 operations on (for uint8)
  the same integers, rounded once to fp32, so they can only differ at a rounding boundary.
* pixels are bit-equal to ``fadd(fmul(x, scale), offset)`` evaluated in torch (two ops) with the coefficients the
  device returned; where ``coef`` matches the definition exactly they are also bit-equal to ``reference_apply``.
Shapes are the smallest that reach every path; the ones that depend on the chunk a workgroup reduces are taken from the
plan.  Every destination sits inside a larger buffer whose guard bytes must survive."""
import ctypes as C
import functools
import json
import os

import pytest
import torch as th

from marlclassification_amd import augment, transforms
from tests.buffers import N_SRC, source
from tests.buffers import bits as _bits
from tests.buffers import guarded as _guarded
from tests.buffers import guards_intact as _guards_intact
from tests.buffers import ulps as _ulps

pytestmark = pytest.mark.gpu

ROWS = [10, 0, 3, 3, 7]
STAT_MODES = ("normal", "channel-normal", "minmax", "channel-minmax")
DTYPES = pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
_source = functools.partial(source, affine=(0.75, 1.5))  # fp32 rows with std >= 0.1 |mean|: asserted where it matters


def _user(c):
    m = [0.485, 0.456, 0.406, 0.5][:c]
    s = [0.229, 0.224, 0.225, 0.25][:c]
    lo, hi = [0.0, 0.1, -0.5, 0.2][:c], [1.0, 0.8, 2.0, 0.7][:c]
    return (transforms.Spec("user-normal", tuple(m), tuple(s)).spelling,
            transforms.Spec("user-minmax", tuple(lo), tuple(hi)).spelling)


def _factor(n):
    """(h, w) with h * w == n, as square as n allows"""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


def _check_records(src, rows, got):
    """records of the device against the definition; returns the definition's"""
    want = transforms.reference_stats(src, rows)
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape
    if src.dtype == th.uint8:
        assert th.equal(got, want)
        return want
    assert th.equal(got[:, :, 2:], want[:, :, 2:]), "min / max are exact"
    x = transforms._selected(src, rows).double().reshape(want.shape[0], want.shape[1], -1)
    n = x.shape[-1]
    for k, terms in ((0, x.abs()), (1, x * x)):
        bound = 2.0 * n * 2.0 ** -53 * terms.sum(-1)
        assert ((got[:, :, k] - want[:, :, k]).abs() <= bound).all(), k
    return want


def _check_case(device, src, rows, spec, offset=0, want_store=None):
    """stats + apply of src[rows] under spec on the device against the definition, every property of the docstring"""
    spec = transforms.parse(spec)
    nb = src.shape[0] if rows is None else rows.shape[0]
    shape = (nb,) + tuple(src.shape[1:])
    src_d, rows_d = src.to(device), None if rows is None else rows.to(device)
    buf, out = _guarded(shape, th.float32, device, offset)
    if want_store is not None:
        assert transforms.plan(src_d, out)["store_bytes"] == want_store
    u8 = src.dtype == th.uint8
    if spec.is_user:
        records = nb
        got, coef = transforms.apply(src_d, rows_d, spec, return_coef=True, out=out)
    else:
        rec_d = transforms.stats(src_d, rows_d)
        records = _check_records(src, rows, rec_d)
        got, coef = transforms.apply(src_d, rows_d, spec, return_coef=True, out=out, records=rec_d)
    assert got.data_ptr() == out.data_ptr()
    th.cuda.synchronize(device)
    assert _guards_intact(buf, offset, out.numel() * 4)
    got, coef = got.cpu(), coef.cpu()
    want_coef = transforms.reference_coef(records, spec, src.shape[1:], u8).to(th.float32)
    assert bool(th.isfinite(coef).all())
    assert int(_ulps(coef, want_coef).max()) <= 1, (spec.spelling, coef, want_coef)
    x = transforms._selected(src, rows).to(th.float32)
    prod = x * coef[:, :, 0, None, None]
    assert th.equal(_bits(got), _bits(prod + coef[:, :, 1, None, None])), spec.spelling
    exact = (_ulps(coef, want_coef) == 0).all(dim=2).all(dim=1)  # images whose pairs match the definition exactly
    want = transforms.reference_apply(src, rows, spec)
    assert th.equal(_bits(got[exact]), _bits(want[exact])), spec.spelling
    return got, coef


# ---- shapes ---------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("shape,store", [((1, 1, 1), 4), ((1, 5, 7), 4), ((3, 8, 8), 16), ((3, 33, 31), 4),
                                         ((2, 5, 6), 8)], ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else None)
def test_small_shapes_every_statistic_mode(device, shape, store, dtype):
    src = _source(shape, dtype)
    rows = th.tensor(ROWS)
    for mode in STAT_MODES:
        got, coef = _check_case(device, src, rows, mode, want_store=store)
        if shape == (1, 1, 1):  # N == 1
            assert not got.any() and not coef.any()


@DTYPES
def test_shapes_from_the_plan_two_partials_and_three(device, dtype):
    probe = th.empty(1, 1, 8, 8, dtype=dtype)
    chunk = transforms.plan(probe)["chunk_elems"]
    for elems, parts in ((chunk + 1, 2), (2 * chunk + 1, 3)):
        h, w = _factor(elems)
        src = _source((2, h, w), dtype, n=3, seed=elems)
        assert transforms.plan(src)["partials_per_plane"] == parts and h * w == elems
        rows = th.tensor([2, 0, 2])
        for mode in ("channel-normal", "minmax"):
            _check_case(device, src, rows, mode)
        # the lone element of the last partial decides: the extremes sit there
        lo, hi = (0, 255) if dtype == th.uint8 else (-50.0, 60.0)
        src[0, 0].view(-1)[-1] = hi
        src[0, 1].view(-1)[-1] = lo
        rec = _check_records(src, None, transforms.stats(src.to(device)))
        assert rec[0, 0, 3] == hi and rec[0, 1, 2] == lo


def test_sum_of_squares_beyond_32_bits(device):
    """3 x 150 x 150, every pixel 255 but one 0, mode normal: S2 = 4.389e9 > 2^32 - the smallest image at which a 32-bit
    sum of squares goes wrong."""
    src = th.full((1, 3, 150, 150), 255, dtype=th.uint8)
    src[0, 1, 77, 3] = 0
    rec = transforms.stats(src.to(device)).cpu()
    assert int(rec[0, :, 1].sum()) == (3 * 150 * 150 - 1) * 255 * 255 > 2 ** 32
    _, coef = _check_case(device, src, None, "normal")
    assert coef[0, 0, 0] > 0 and bool((coef[0] == coef[0, 0]).all())


def test_an_all_255_plane_of_exactly_one_chunk(device):
    """a lane's accumulators at their worst case; the random plane beside it is unaffected"""
    chunk = transforms.plan(th.empty(1, 1, 8, 8, dtype=th.uint8))["chunk_elems"]
    h, w = _factor(chunk)
    src = _source((2, h, w), th.uint8, n=2, seed=4)
    src[:, 0] = 255
    assert transforms.plan(src)["partials_per_plane"] == 1 and h * w == chunk
    rec = transforms.stats(src.to(device)).cpu()
    assert rec[0, 0].tolist() == [255 * chunk, 255 * 255 * chunk, 255, 255]
    got, coef = _check_case(device, src, None, "channel-normal")
    assert not got[:, 0].any() and not coef[:, 0].any() and bool(got[:, 1].any())
    _check_case(device, src, None, "normal")


# ---- modes, element types, channel counts -----------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("c", [1, 3, 4])
def test_all_six_modes(device, dtype, c):
    src = _source((c, 9, 12), dtype, seed=c)
    rows = th.tensor(ROWS)
    for spec in STAT_MODES + _user(c):
        got, coef = _check_case(device, src, rows, spec)
        if transforms.parse(spec).whole_image:
            assert bool((coef == coef[:, :1]).all()), "one pair per image"
    if dtype == th.float32:  # the inputs of the 1-ulp claim: std >= 0.1 |mean| on every plane
        flat = src.double().reshape(N_SRC, c, -1)
        assert bool((flat.std(-1) >= 0.1 * flat.mean(-1).abs()).all())


def test_user_modes_take_up_to_sixteen_channels(device):
    c = 16
    src = _source((c, 4, 4), th.uint8, n=2)
    spec = transforms.Spec("user-normal", tuple(0.03 * k for k in range(c)), tuple(0.1 + 0.05 * k for k in range(c)))
    _check_case(device, src, None, spec)
    with pytest.raises(ValueError, match="16"):
        transforms.Spec("user-normal", (0.5,) * 17, (0.5,) * 17).user(17)
    # statistic modes have no channel limit
    _check_case(device, _source((19, 4, 4), th.uint8, n=2), None, "channel-normal")


# ---- rows -------------------------------------------------------------------------------------------------------------
@DTYPES
def test_rows_given_null_repeated_and_out_of_range(device, dtype):
    src = _source((3, 8, 10), dtype)
    _check_case(device, src, None, "channel-normal")                      # rows == NULL: every image
    _check_case(device, src, th.tensor([4, 4, 4, 9]), "normal")           # repeated
    hostile = th.tensor([-1, -2 ** 62, N_SRC, 2 ** 62, 5, 2 ** 31])       # clamped to [0, n_src)
    got, _ = _check_case(device, src, hostile, "channel-minmax")
    want = transforms.reference_apply(src, th.tensor([0, 0, N_SRC - 1, N_SRC - 1, 5, N_SRC - 1]), "channel-minmax")
    assert th.equal(_bits(got), _bits(want))


def test_source_offsets_are_64_bit(device):
    """A uint8 set of more than 2^32 bytes (nothing filled but the rows used): the last row and row 0."""
    n, shape = 21846, (3, 256, 256)
    assert n * 3 * 256 * 256 > 2 ** 32
    big = th.empty((n,) + shape, dtype=th.uint8, device=device)
    two = _source(shape, th.uint8, n=2, seed=9)
    big[n - 1].copy_(two[0])
    big[0].copy_(two[1])
    rows = th.tensor([n - 1, 0, n - 1], device=device)
    rec = transforms.stats(big, rows)
    assert th.equal(rec.cpu(), transforms.reference_stats(two, th.tensor([0, 1, 0])))
    for spec in ("channel-normal", _user(3)[0]):
        got = transforms.apply(big, rows, spec)
        assert th.equal(_bits(got.cpu()), _bits(transforms.reference_apply(two, th.tensor([0, 1, 0]), spec))), spec
    del big
    th.cuda.empty_cache()


# ---- buffers, repeatability, streams --------------------------------------------------------------------------------
@DTYPES
def test_guard_bytes_around_every_buffer_of_the_c_entries(device, dtype):
    from marlclassification_amd import _lib

    lib = _lib.load()
    shape = (3, 33, 31)
    src = _source(shape, dtype)
    src_d, rows_d = src.to(device), th.tensor(ROWS, device=device)
    nb, (c, h, w), elt = len(ROWS), shape, src.element_size()
    need = lib.marl_batch_stats_scratch_bytes(nb, c, h, w, elt)
    p = transforms.plan(src_d)
    assert need == nb * c * p["partials_per_plane"] * 32 > 0
    sbuf, scratch = _guarded((need,), th.uint8, device)  # exactly sized
    rbuf, records = _guarded((nb, c, 4), th.int64 if dtype == th.uint8 else th.float64, device)
    dbuf, dst = _guarded((nb,) + shape, th.float32, device)
    cbuf, coef = _guarded((nb, c, 2), th.float32, device)
    stream = th.cuda.current_stream(device).cuda_stream
    _lib.check(lib.marl_batch_stats(src_d.data_ptr(), N_SRC, rows_d.data_ptr(), nb, c, h, w, elt, scratch.data_ptr(),
                                    records.data_ptr(), stream))
    _lib.check(lib.marl_batch_normalize(src_d.data_ptr(), N_SRC, rows_d.data_ptr(), records.data_ptr(),
                                        transforms.MODES["channel-normal"], None, nb, c, h, w, elt, dst.data_ptr(),
                                        coef.data_ptr(), stream))
    th.cuda.synchronize(device)
    assert _guards_intact(sbuf, 0, need) and _guards_intact(rbuf, 0, records.numel() * 8)
    assert _guards_intact(dbuf, 0, dst.numel() * 4) and _guards_intact(cbuf, 0, coef.numel() * 4)
    _check_records(src, th.tensor(ROWS), records)
    got, pairs = transforms.apply(src_d, rows_d, "channel-normal", return_coef=True)
    assert th.equal(_bits(dst), _bits(got)) and th.equal(_bits(coef), _bits(pairs))
    # coef == NULL: the same pixels
    dst2 = th.empty_like(dst)
    _lib.check(lib.marl_batch_normalize(src_d.data_ptr(), N_SRC, rows_d.data_ptr(), records.data_ptr(),
                                        transforms.MODES["channel-normal"], None, nb, c, h, w, elt, dst2.data_ptr(),
                                        None, stream))
    assert th.equal(_bits(dst2), _bits(dst))


def test_two_calls_give_the_same_bytes_and_a_side_stream_is_respected(device):
    chunk = transforms.plan(th.empty(1, 1, 8, 8))["chunk_elems"]
    h, w = _factor(2 * chunk + 1)
    src = _source((2, h, w), th.float32, n=4, seed=3)  # three partials a plane: fp64 sums in a fixed order
    rows = th.tensor([3, 1, 1])
    src_d, rows_d = src.to(device), rows.to(device)
    a, b = transforms.stats(src_d, rows_d), transforms.stats(src_d, rows_d)
    assert th.equal(a.view(th.int64), b.view(th.int64))
    (xa, ca), (xb, cb) = (transforms.apply(src_d, rows_d, "normal", return_coef=True) for _ in range(2))
    assert th.equal(_bits(xa), _bits(xb)) and th.equal(_bits(ca), _bits(cb))
    # the source is produced on a side stream behind some work; the three launches must queue behind it on that stream
    side = th.cuda.Stream(device=device)
    late = th.zeros_like(src_d)
    m = th.randn(2048, 2048, device=device)
    th.cuda.synchronize(device)
    with th.cuda.stream(side):
        for _ in range(8):
            m = (m @ m).clamp_(-1.0, 1.0)
        late.copy_(src_d)
        got = transforms.apply(late, rows_d, "normal")
    side.synchronize()
    assert th.equal(_bits(got), _bits(xa))


def test_every_guard_of_the_c_entries(device):
    """real device buffers (the host-only list of tests/test_transforms_host.py, with pointers that could be used): a
    refusal enqueues nothing, adjacent buffers are no overlap, and a good call after the refusals runs"""
    from marlclassification_amd import _lib

    lib = _lib.load()
    src = th.zeros(4, 3, 8, 8, dtype=th.uint8, device=device)
    arena = th.zeros(2 * 4 * 3 * 64, dtype=th.float32, device=device)
    dst = arena[: 4 * 3 * 64]
    rec = th.zeros(4, 3, 4, dtype=th.int64, device=device)
    scratch = th.zeros(lib.marl_batch_stats_scratch_bytes(4, 3, 8, 8, 1), dtype=th.uint8, device=device)
    coef = th.zeros(4, 3, 2, device=device)
    s, d, r, k, q = (t.data_ptr() for t in (src, dst, rec, scratch, coef))
    user = (C.c_double * 6)(0.5, 0.25, 0.5, 0.25, 0.5, 0.25)

    def norm(src_p=s, n_src=4, rows=None, rec_p=r, mode=1, usr=None, batch=4, c=3, h=8, w=8, elt=1, dst_p=d, coef_p=q):
        rc = lib.marl_batch_normalize(src_p, n_src, rows, rec_p, mode, usr, batch, c, h, w, elt, dst_p, coef_p, None)
        return rc, lib.marl_last_error().decode()

    def stat(src_p=s, n_src=4, rows=None, batch=4, c=3, h=8, w=8, elt=1, scratch_p=k, rec_p=r):
        rc = lib.marl_batch_stats(src_p, n_src, rows, batch, c, h, w, elt, scratch_p, rec_p, None)
        return rc, lib.marl_last_error().decode()

    bad_s = (C.c_double * 6)(0.5, 0.25, 0.5, 0.0, 0.5, 0.25)
    bad_w = (C.c_double * 6)(0.5, 0.9, 0.3, 0.3, 0.5, 0.9)
    nan = (C.c_double * 6)(float("nan"), 0.9, 0.3, 0.4, 0.5, 0.9)
    for kw, word in ((dict(src_p=None), "null"), (dict(dst_p=None), "null"), (dict(rec_p=None), "records"),
                     (dict(mode=5, usr=None), "user"), (dict(mode=6), "mode"), (dict(elt=2), "elt_bytes"),
                     (dict(batch=0), "positive"), (dict(n_src=0), "positive"), (dict(c=0), "positive"),
                     (dict(h=-1), "positive"), (dict(w=0), "positive"), (dict(n_src=3), "n_src"),
                     (dict(mode=4, usr=user, c=17), "16"), (dict(mode=4, usr=bad_s), "s must"),
                     (dict(mode=5, usr=bad_w), "hi - lo"), (dict(mode=4, usr=nan), "finite"),
                     (dict(dst_p=s), "overlaps"), (dict(src_p=d + 4 * (4 * 3 * 64 - 1), n_src=4), "overlaps"),
                     (dict(src_p=s + 2, elt=4, w=2), "aligned"), (dict(dst_p=d + 2), "aligned"),
                     (dict(rec_p=r + 4), "records"), (dict(coef_p=q + 2), "coef")):
        rc, msg = norm(**kw)
        assert rc == -1 and msg.startswith("marl_batch_normalize:") and word in msg, (kw, rc, msg)
    for kw, word in ((dict(c=2, h=32768, w=32768), "2^31"), (dict(c=3, h=2048, w=2048), "2^23")):
        assert norm(**kw)[0] == -2 and word in norm(**kw)[1]
        assert stat(**kw)[0] == -2 and word in stat(**kw)[1]
    for kw, word in ((dict(src_p=None), "null"), (dict(scratch_p=None), "null"), (dict(rec_p=None), "null"),
                     (dict(elt=3), "elt_bytes"), (dict(batch=0), "positive"), (dict(h=0), "positive"),
                     (dict(n_src=2), "n_src"), (dict(scratch_p=k + 4), "8-byte"), (dict(rec_p=r + 4), "8-byte")):
        rc, msg = stat(**kw)
        assert rc == -1 and msg.startswith("marl_batch_stats:") and word in msg, (kw, rc, msg)
    th.cuda.synchronize(device)
    assert not dst.any() and not rec.any() and not coef.any(), "a refused call wrote"
    # the source directly behind the destination is no overlap; after all those refusals the entries still run
    src.copy_(_source((3, 8, 8), th.uint8, n=4))
    tail = arena[4 * 3 * 64:].view(th.uint8)[: src.numel()].view(src.shape)
    tail.copy_(src)
    assert stat(src_p=tail.data_ptr())[0] == 0
    assert norm(src_p=tail.data_ptr())[0] == 0
    th.cuda.synchronize(device)
    assert th.equal(_bits(dst.view(4, 3, 8, 8).cpu()), _bits(transforms.reference_apply(src.cpu(), None, "channel-normal")))
    with pytest.raises(RuntimeError, match="GPU"):
        transforms.apply(src.cpu(), None, "normal")
    with pytest.raises(ValueError, match="rows"):
        transforms.stats(src, th.zeros(2, dtype=th.int32, device=device))
    with pytest.raises(ValueError, match="out"):
        transforms.apply(src, None, "normal", out=th.empty(4, 3, 8, 8, dtype=th.uint8, device=device))


# ---- constants ------------------------------------------------------------------------------------------------------
@DTYPES
def test_constant_planes_and_images_give_zeros(device, dtype):
    src = _source((3, 12, 10), dtype, n=3)
    src[0] = 77 if dtype == th.uint8 else 0.3
    src[1, 1] = 255 if dtype == th.uint8 else -2.5
    for mode in STAT_MODES:
        got, coef = _check_case(device, src, None, mode)
        assert bool(th.isfinite(got).all()) and not got[0].any() and not coef[0].any(), mode
        if mode.startswith("channel"):
            assert not got[1, 1].any() and bool(got[1, 0].any()) and bool(got[1, 2].any()), mode
        else:
            assert bool(got[1].any()), mode
        assert bool(got[2].any()), mode


@DTYPES
def test_statistics_of_a_dihedral_view_equal_those_of_its_source(device, dtype):
    """a flip or quarter turn permutes the pixels of every plane: the integer records are those of the source, and the
    exact fp32 extremes too - a cross-check of the two kernels that share no code but the row clamp"""
    src = _source((3, 24, 24), dtype).to(device)
    rows = th.tensor(ROWS + ROWS[:3], device=device)
    ops = th.zeros(8, 8, dtype=th.int32, device=device)
    ops[:, 0] = th.arange(8)
    view = augment.apply(src, rows, ops)
    a, b = transforms.stats(view), transforms.stats(src, rows)
    if dtype == th.uint8:
        assert th.equal(a, b)
    else:
        assert th.equal(a[:, :, 2:], b[:, :, 2:])
        _check_records(view.cpu(), None, a)  # (the sums: each side against the definition, in its own order)
        _check_records(src.cpu(), rows.cpu(), b)


# ---- the loaders ----------------------------------------------------------------------------------------------------
AUG, MIX = "d4,shift:2:zero,erase:5:0.7", "cutmix:1.0"


def test_resident_loader_normalises_plain_augmented_and_mixed_batches(device):
    from marlclassification_amd import mix
    from marlclassification_amd.data import ResidentLoader, SyntheticImages
    from marlclassification_amd.train import ShardedBatchSampler

    ds = SyntheticImages(37, 3, 16, 5, seed=3)
    part = th.randperm(37, generator=th.Generator().manual_seed(1))[:31].tolist()
    bs = ShardedBatchSampler(part, 8, 0, 1, shuffle=True, seed=2)
    policy, mix_policy = augment.parse(AUG), mix.parse(MIX)
    spec = "channel-normal"

    def loader(**kw):
        if kw:
            kw["generator"] = th.Generator(device=device).manual_seed(77)
        return ResidentLoader(ds, part, bs, device, **kw)

    plain, plain_n = loader(), loader(normalize=spec)
    aug, aug_n = loader(augment=policy), loader(augment=policy, normalize=transforms.parse(spec))
    mixed = loader(augment=policy, mix=mix_policy, nb_class=5)
    mixed_n = loader(augment=policy, mix=mix_policy, nb_class=5, normalize=spec)
    for (x, y), (xn, yn), idx in zip(list(plain), list(plain_n), list(bs)):
        assert x.dtype == th.uint8 and xn.dtype == th.float32 and th.equal(y, yn)
        assert th.equal(_bits(xn.cpu()), _bits(transforms.reference_apply(ds.x, th.tensor(idx), spec)))
    # the policies draw from generators in the same state: the normalised batch is the definition of what they made
    for (x, y), (xn, yn) in zip(list(aug), list(aug_n)):
        assert th.equal(y, yn)
        assert th.equal(_bits(xn.cpu()), _bits(transforms.reference_apply(x.cpu(), None, spec)))
    for (x, y, q), (xn, yn, qn) in zip(list(mixed), list(mixed_n)):
        assert th.equal(y, yn) and th.equal(q, qn)
        assert th.equal(_bits(xn.cpu()), _bits(transforms.reference_apply(x.cpu(), None, spec)))
    with pytest.raises(ValueError, match="dataset"):
        loader(normalize="dataset")


def test_device_prefetcher_normalises_plain_augmented_and_mixed_batches(device):
    from torch.utils.data import DataLoader

    from marlclassification_amd import mix
    from marlclassification_amd.data import DevicePrefetcher, SyntheticImages

    ds = SyntheticImages(20, 1, 28, 10, seed=4)
    dl = DataLoader(ds, batch_size=8, shuffle=False)
    policy, mix_policy = augment.parse(AUG), mix.parse(MIX)
    spec = "minmax"

    def loader(**kw):
        if kw.keys() - {"normalize"}:
            kw["generator"] = th.Generator(device=device).manual_seed(5)
        return DevicePrefetcher(dl, device, **kw)

    for k, ((x, y), (xn, yn)) in enumerate(zip(list(loader()), list(loader(normalize=spec)))):
        assert th.equal(x.cpu(), ds.x[8 * k: 8 * k + 8]) and th.equal(y, yn) and xn.dtype == th.float32
        assert th.equal(_bits(xn.cpu()), _bits(transforms.reference_apply(x.cpu(), None, spec)))
    for (x, y), (xn, yn) in zip(list(loader(augment=policy)), list(loader(augment=policy, normalize=spec))):
        assert th.equal(y, yn)
        assert th.equal(_bits(xn.cpu()), _bits(transforms.reference_apply(x.cpu(), None, spec)))
    for (x, y, q), (xn, yn, qn) in zip(list(loader(mix=mix_policy, nb_class=10)),
                                       list(loader(mix=mix_policy, nb_class=10, normalize=spec))):
        assert th.equal(y, yn) and th.equal(q, qn)
        assert th.equal(_bits(xn.cpu()), _bits(transforms.reference_apply(x.cpu(), None, spec)))


def test_dataset_spec_on_the_device_is_the_definition(device):
    x = _source((3, 16, 16), th.uint8, n=37, seed=8)
    assert transforms.dataset_spec(x.to(device), chunk=16) == transforms.dataset_spec(x)


# ---- through the trainer and the command line -----------------------------------------------------------------------
ACTIONS = [[1, 0], [-1, 0], [0, 1], [0, -1]]


def _mnist_model(device, seed):
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import MnistCnn

    th.manual_seed(seed)
    return ModelsWrapper(MnistCnn(6), 32, 32, 8, 12, 8, 2, 4, 10, 48, 48).to(device)


def test_a_train_step_on_a_normalised_batch_equals_the_step_on_the_definitions_tensor(device):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.training import Trainer

    resident = _source((1, 28, 28), th.uint8, seed=21)
    rows = th.tensor([10, 0, 3, 3, 7, 1, 9, 2])
    y = th.randint(0, 10, (8,), generator=th.Generator().manual_seed(4)).to(device)
    want = transforms.reference_apply(resident, rows, "normal")
    fused_x = transforms.apply(resident.to(device), rows.to(device), "normal")
    assert th.equal(_bits(fused_x.cpu()), _bits(want)), "the two steps would not see the same bytes"
    params = []
    for x in (fused_x, want.to(device)):
        model = _mnist_model(device, 99)
        sampler = EpisodeSampler(MultiAgent(3, model), Environment(ACTIONS, 6), 4)
        trainer = Trainer(model, 10, 1e-3, 0.99)
        trainer.train_step(x, y, sampler)
        th.cuda.synchronize(device)
        params.append({n: p.detach().clone() for n, p in model.named_parameters()})
    assert params[0].keys() == params[1].keys()
    for n in params[0]:
        assert th.equal(params[0][n], params[1][n]), n


def _image_folder(root, classes=3, per_class=7):
    import numpy as np
    from PIL import Image

    rng = np.random.default_rng(0)
    for c in range(classes):
        (root / f"class{c}").mkdir(parents=True)
        for k in range(per_class):
            arr = rng.integers(0, 256, (28, 28), dtype=np.uint8)
            arr[4 * c: 4 * c + 8] = 255  # a class-dependent bright band
            Image.fromarray(arr).save(root / f"class{c}" / f"img{k}.png")


def test_train_writes_the_key_and_test_and_infer_pick_it_up(device, tmp_path, capsys, monkeypatch):
    from marlclassification_amd import transforms as tr
    from marlclassification_amd.__main__ import main

    out = str(tmp_path / "run")
    head = ["--run-id", "r", "-a", "3", "--step", "3", "--cuda"]
    main(head + ["train", "--res-folder", "synthetic", "--nb-epoch", "1", "--batch-size", "8", "--nb-class", "3",
                 "--normalize", "channel-normal", "-o", out])
    capsys.readouterr()
    marl_json = os.path.join(out, "marl.json")
    assert json.load(open(marl_json))["normalize"] == "channel-normal"
    weights = os.path.join(out, "models", "nn_models_epoch_0.pt")
    assert os.path.exists(weights)
    root = tmp_path / "images"
    _image_folder(root)
    calls = []
    real_apply = tr.apply
    monkeypatch.setattr(tr, "apply", lambda src, rows, spec, *a, **kw: (calls.append(tr.parse(spec).spelling),
                                                                        real_apply(src, rows, spec, *a, **kw))[1])
    test_mode = ["test", "--dataset-path", str(root), "--json-path", marl_json, "--state-dict-path", weights,
                 "--batch-size", "8", "--img-size", "28"]
    main(head + test_mode + ["-o", str(tmp_path / "t0")])
    assert calls and set(calls) == {"channel-normal"}  # 21 images in batches of 8: three batches
    n_default = len(calls)
    assert n_default == 3
    del calls[:]
    main(head + test_mode + ["-o", str(tmp_path / "t1"), "--normalize", "none"])  # the override: today's uint8 path
    assert calls == []
    main(head + test_mode + ["-o", str(tmp_path / "t2"), "--normalize", "minmax"])
    assert set(calls) == {"minmax"} and len(calls) == 3
    del calls[:]
    main(head + test_mode + ["-o", str(tmp_path / "t3"), "--tta", "hflip"])  # every view with its own statistics
    assert set(calls) == {"channel-normal"} and len(calls) == 6
    del calls[:]
    class_json = os.path.join(out, "class_to_idx.json")
    image = str(root / "class1" / "img0.png")
    main(head + ["infer", "--images", image, "--json-path", marl_json, "--state-dict-path", weights, "--class2idx",
                 class_json, "-o", str(tmp_path / "frames"), "--saliency"])
    assert calls == ["channel-normal", "channel-normal"]  # the episode of the frames, and the saliency map's
    frames = tmp_path / "frames" / "img0.png"
    assert (frames / "pred_original.png").exists() and (frames / "saliency.png").exists()
    # the frames paint the original uint8 image, not the normalised one
    import numpy as np
    from PIL import Image

    painted = np.asarray(Image.open(frames / "pred_original.png").convert("L"))
    assert painted.min() < 64 and painted.max() > 192
    capsys.readouterr()


def test_train_normalize_dataset_stores_the_resolved_user_normal(device, tmp_path, capsys):
    from marlclassification_amd.__main__ import main
    from marlclassification_amd.data import SyntheticImages

    out = str(tmp_path / "run")
    os.environ["MARL_SEED"] = "5"
    try:
        main(["--run-id", "r", "-a", "3", "--step", "3", "--cuda", "train", "--res-folder", "synthetic", "--nb-epoch",
              "1", "--batch-size", "8", "--nb-class", "3", "--normalize", "dataset", "-o", out])
    finally:
        del os.environ["MARL_SEED"]
    capsys.readouterr()
    stored = json.load(open(os.path.join(out, "marl.json")))["normalize"]
    assert stored.startswith("user-normal:")
    spec = transforms.parse(stored)
    # the training split of that run: 85 % of the synthetic set under the run's seed
    ds = SyntheticImages(64, 1, 28, 3)
    idx = th.randperm(len(ds), generator=th.Generator().manual_seed(5))
    assert spec == transforms.dataset_spec(ds.x[idx[: int(0.85 * len(ds))]])
