"""GPU: the mixing batch gather ``marl_batch_mix`` (``mix.apply``) against its definition ``mix.reference_apply`` on the
CPU.  Every comparison is bit for bit - uint8 as values, fp32 as bit patterns (the Mixup blend is two rounded products
and a rounded sum on both sides).  Shapes are the smallest at which the addressing changes; each case asserts the store
width ``marl_batch_mix_plan`` reports.  Every destination sits inside a larger buffer whose guard bytes must survive."""
import pytest
import torch as th

from marlclassification_amd import augment, mix
from tests.buffers import N_SRC, SENTINEL
from tests.buffers import guarded as _guarded
from tests.buffers import guards_intact as _guards_intact
from tests.buffers import same_bits as _same_bits
from tests.buffers import source as _source

pytestmark = pytest.mark.gpu

ROWS = [10, 0, 3, 3, 7]  # batch 5 from a resident set of 11 rows: repeated, unsorted
NB = len(ROWS)
FILL = {th.uint8: 200, th.float32: -1.5}
DTYPES = [th.uint8, th.float32]

# shape -> store bytes (uint8, fp32) with a 16-byte aligned destination
SHAPES = {
    (1, 5, 7): (1, 4),      # uint8 rows of odd bytes: byte stores
    (3, 8, 8): (8, 16),
    (3, 12, 20): (4, 16),   # non-square: bit 0 of d4 is dropped
    (1, 28, 28): (4, 16),
    (3, 64, 64): (16, 16),  # 16-byte stores; 3 bands per fp32 image
}


def _op_sets(c, h, w):
    """ops [NB, 8] per set: every d4 code on either view (a transposing b with a plain p and the reverse come from the
    partner cycle b -> b + 1 over these rows), shifts of +-1 and +-(W - 1), an erase rectangle in the middle (it
    crosses the boxes below)"""
    codes = list(range(8)) if h == w else [0, 2, 4, 6]
    sets = []
    for r in range(len(codes)):
        ops = th.zeros(NB, 8, dtype=th.int32)
        for b in range(NB):
            ops[b, 0] = codes[(r + 3 * b) % len(codes)] if b % 2 == 0 else codes[r]
        sets.append(ops)
    plain_vs_turned = th.zeros(NB, 8, dtype=th.int32)
    plain_vs_turned[::2, 0] = 1 if h == w else 2  # b transposing, p plain - and the reverse for odd b
    sets.append(plain_vs_turned)
    shifts = th.tensor([[2, 0, 1], [0, 0, -1], [6, 1, w - 1], [4, -1, -(w - 1)], [0, h - 1, 0]], dtype=th.int32)
    shifted = th.zeros(NB, 8, dtype=th.int32)
    shifted[:, :3] = shifts
    sets.append(shifted)
    erased = shifted.clone()
    erased[:, 0] = th.tensor([0, 2, 4, 6, 0], dtype=th.int32)
    erased[:, 3:7] = th.tensor([h // 2 - 1, w // 2 - 2, 3, 5], dtype=th.int32)
    sets.append(erased)
    return sets


def _mix_sets(c, h, w):
    """mix [NB, 8] per set: a partner cycle, partner == b, repeats; boxes empty / one pixel / clipped at each edge /
    the whole image / with edges inside a vector store; every k of the issue; all three modes in one batch"""
    cyc = [1, 2, 3, 4, 0]
    boxes = [(0, 0, 0, 0), (h // 2, w // 2, 1, 1), (-2, 1, 4, w - 2), (h - 2, 1, 5, w - 2), (1, -3, h - 2, 5),
             (1, w - 2, h - 2, 7), (0, 0, h, w), (1, 1, h - 2, 3), (2, 3, 3, w - 5), (0, 2, h, 1), (3, 0, 1, w),
             (h // 2 - 1, w // 2 - 1, 3, 4)]
    sets = []
    for r in range(0, len(boxes), 2):
        m = th.zeros(NB, 8, dtype=th.int32)
        for b in range(NB):
            by, bx, bh, bw = boxes[(r + b) % len(boxes)]
            m[b] = th.tensor([cyc[b], 1, by, bx, bh, bw, 256, 0], dtype=th.int32)
        sets.append(m)
    ks = th.zeros(NB, 8, dtype=th.int32)
    ks[:, 0] = th.tensor(cyc, dtype=th.int32)
    ks[:, 1] = 2
    ks[:, 6] = th.tensor([0, 1, 128, 255, 256], dtype=th.int32)
    sets.append(ks)
    both = ks.clone()  # partner == b, a repeated partner, all three modes side by side
    both[:, 0] = th.tensor([0, 0, 4, 4, 4], dtype=th.int32)
    both[:, 1] = th.tensor([2, 1, 0, 2, 1], dtype=th.int32)
    both[:, 2:6] = th.tensor([1, 2, h - 1, w - 3], dtype=th.int32)
    both[:, 6] = th.tensor([77, 256, 3, 200, 19], dtype=th.int32)
    sets.append(both)
    return sets


def _compare(device, src, src_d, rows, ops, m, mode, dtype, buf, dst, offset, what):
    buf.fill_(SENTINEL)
    rows_d = None if rows is None else rows.to(device)
    got = mix.apply(src_d, rows_d, None if ops is None else ops.to(device), None if m is None else m.to(device),
                    pad_mode=mode, fill=FILL[dtype], out=dst)
    assert got is dst
    want = mix.reference_apply(src, rows, ops, m, mode, FILL[dtype])
    out = dst.cpu()
    if not _same_bits(out, want):
        bad = [(b, None if ops is None else ops[b].tolist(), None if m is None else m[b].tolist())
               for b in range(want.shape[0]) if not _same_bits(out[b], want[b])]
        pytest.fail(f"{what} {mode}: images differ under (b, ops, mix) {bad}")
    assert _guards_intact(buf, offset, out.numel() * out.element_size()), f"{what} {mode}: guard bytes overwritten"


def _run_cases(device, shape, dtype, offset, want_store):
    src = _source(shape, dtype)
    src_d = src.to(device)
    rows = th.tensor(ROWS)
    buf, dst = _guarded((NB,) + tuple(shape), dtype, device, offset)
    info = mix.plan(src_d, dst)
    assert info["store_bytes"] == want_store and info["band_vectors"] == 1024 and info["lds_bytes"] == 0, info
    total = shape[0] * shape[1] * (shape[2] * src.element_size() // want_store)
    assert info["blocks_per_image"] == -(-total // 1024), info
    op_sets, mix_sets = _op_sets(*shape), _mix_sets(*shape)
    what = f"{shape} {dtype}"
    for i, ops in enumerate(op_sets):  # every op set under two mix sets, every mix set under two op sets
        for j in {i % len(mix_sets), (i + 3) % len(mix_sets), len(mix_sets) - 1 - (i % 2)}:
            _compare(device, src, src_d, rows, ops, mix_sets[j], "reflect" if (i + j) % 2 else "zero", dtype, buf, dst,
                     offset, what)
    for j, m in enumerate(mix_sets):
        for mode in ("reflect", "zero"):
            _compare(device, src, src_d, rows, op_sets[-1 - (j % 2)], m, mode, dtype, buf, dst, offset, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_every_view_box_and_blend_is_the_reference_bit_for_bit(device, shape, dtype):
    _run_cases(device, shape, dtype, 0, SHAPES[shape][dtype == th.float32])


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32"])
def test_destination_offset_by_four_bytes_takes_narrow_stores(device, dtype):
    _run_cases(device, (3, 8, 8), dtype, 4, 4)


def test_several_bands_per_image(device):
    """3 x 256 x 256 uint8, batch 3: 12 bands of 16-byte stores per image; boxes across band edges"""
    shape, dtype = (3, 256, 256), th.uint8
    src = _source(shape, dtype, n=4)
    src_d = src.to(device)
    rows = th.tensor([3, 0, 3])
    ops = th.tensor([[2, 3, -5, 100, 90, 40, 50, 0], [5, -1, 1, 0, 0, 0, 0, 0], [0, 0, 17, 0, 0, 0, 0, 0]], dtype=th.int32)
    m = th.tensor([[1, 1, 50, 37, 150, 101, 256, 0], [2, 2, 0, 0, 0, 0, 100, 0], [0, 1, 60, 16, 70, 64, 256, 0]],
                  dtype=th.int32)
    buf, dst = _guarded((3,) + shape, dtype, device)
    info = mix.plan(src_d, dst)
    assert info["store_bytes"] == 16 and info["blocks_per_image"] == 12, info
    _compare(device, src, src_d, rows, ops, m, "reflect", dtype, buf, dst, 0, "3x256x256")


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32"])
def test_null_mix_is_the_augmenting_gather_byte_for_byte(device, dtype):
    for shape in ((3, 64, 64), (3, 12, 20), (1, 5, 7)):
        src_d = _source(shape, dtype).to(device)
        rows = th.tensor(ROWS).to(device)
        codes = [0, 1, 2, 3, 4] if shape[1] == shape[2] else [0, 2, 4, 6, 2]
        ops = th.tensor([[codes[b], b - 2, 2 - b, 1, 1, b, 3, 0] for b in range(NB)], dtype=th.int32).to(device)
        for mode in ("reflect", "zero"):
            want = augment.apply(src_d, rows, ops, pad_mode=mode, fill=FILL[dtype])
            assert _same_bits(mix.apply(src_d, rows, ops, None, pad_mode=mode, fill=FILL[dtype]), want)
            zeros = th.zeros(NB, 8, dtype=th.int32, device=device)
            assert _same_bits(mix.apply(src_d, rows, ops, zeros, pad_mode=mode, fill=FILL[dtype]), want)
        assert _same_bits(mix.apply(src_d, rows), src_d.index_select(0, rows))
        assert _same_bits(mix.apply(src_d), src_d)
    src_d = _source((3, 8, 8), dtype).to(device)
    with pytest.raises(RuntimeError, match="overlaps"):
        mix.apply(src_d, out=src_d)
    with pytest.raises(TypeError):
        mix.apply(src_d.to(th.float64))
    with pytest.raises(ValueError):
        mix.apply(src_d, mix=th.zeros(N_SRC, 8, dtype=th.int64, device=device))
    with pytest.raises(ValueError):
        mix.apply(src_d, rows=th.tensor(ROWS).to(device), mix=th.zeros(NB + 1, 8, dtype=th.int32, device=device))
    with pytest.raises(RuntimeError, match="GPU"):
        mix.apply(src_d.cpu())


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("shape", [(3, 8, 8), (2, 12, 20)], ids=lambda s: "x".join(map(str, s)))
def test_hostile_device_values_are_sanitised(device, shape, dtype):
    """Built so that nothing can leave an allocation even if the clamping were wrong: ``src`` is rows 2 .. 8 of a
    12-row buffer whose other rows hold a value the images do not contain, and the destination of 8 images sits in the
    middle of a buffer of 24; the hostile values are small multiples of the sizes, or so large that an unclamped use
    would show as a wrong pixel, not as an address (partner and the box only select between in-range candidates)."""
    c, h, w = shape
    mark = 7 if dtype == th.uint8 else 12345.0
    whole = _source(shape, dtype, n=12, seed=5)
    if dtype == th.uint8:
        whole[whole == mark] = 8
    whole[:2], whole[9:] = mark, mark
    whole_d = whole.to(device)
    src, src_d = whole[2:9], whole_d[2:9]
    n_src = src.shape[0]
    rows = th.tensor([-1, n_src + 1, n_src, 3, -2, 0, n_src - 1, 5])
    ops = th.tensor([[11, h + 3, 0, 0, 0, 0, 0, 0], [0, 0, -(w + 3), 0, 0, 0, 0, 0], [15, -(h + 3), w + 3, 0, 0, 0, 0, 0],
                     [2, 0, 0, h - 2, w - 3, 9, 9, 0], [9, 0, 0, -4, -4, 7, 7, 0], [-1, 1, 1, 2, 2, -3, 4, 0],
                     [6, 2, -2, -3, 1, h + 9, w + 9, 5], [4, h + 3, w + 3, h + 2, w + 2, 3, 3, 0]], dtype=th.int32)
    big = 2**31 - 1
    m = th.tensor([[-5, 1, 0, 0, h, w, 256, 0], [10**9, 1, 0, 0, h, w, 256, 0], [3, 7, 0, 0, h, w, 0, 0],
                   [1, 1, -big - 1, -big - 1, big, big, 256, 0], [2, 1, -4, -3, big, big, 256, 0],
                   [6, 2, 0, 0, 0, 0, -1, 0], [5, 2, 0, 0, 0, 0, 999, 0], [0, 5, 1, 1, big, -big, 40, 0]], dtype=th.int32)
    nb = rows.shape[0]
    pad = th.full((3 * nb,) + tuple(shape), mark, dtype=dtype, device=device)
    dst = pad[nb: 2 * nb]
    for mode in ("reflect", "zero"):
        pad.fill_(mark)
        mix.apply(src_d, rows.to(device), ops.to(device), m.to(device), pad_mode=mode, fill=FILL[dtype], out=dst)
        got = dst.cpu()
        assert _same_bits(got, mix.reference_apply(src, rows, ops, m, mode, FILL[dtype])), mode
        assert not bool((got == mark).any()), "a pixel from outside the source rows"
        assert bool((pad[:nb] == mark).all()) and bool((pad[2 * nb:] == mark).all()), "a store outside the destination"


def test_source_offsets_are_64_bit(device):
    """A uint8 set of more than 2^32 bytes (nothing filled but the rows used): the last row mixed with row 0."""
    n, shape = 21846, (3, 256, 256)
    assert n * 3 * 256 * 256 > 2**32
    big = th.empty((n,) + shape, dtype=th.uint8, device=device)
    two = _source(shape, th.uint8, n=2, seed=9)
    big[n - 1].copy_(two[0])
    big[0].copy_(two[1])
    rows = th.tensor([n - 1, 0])
    ops = th.tensor([[2, 3, -5, 0, 0, 0, 0, 0], [4, 0, 0, 9, 9, 30, 30, 0]], dtype=th.int32)
    m = th.tensor([[1, 1, 20, 30, 100, 99, 256, 0], [0, 2, 0, 0, 0, 0, 90, 0]], dtype=th.int32)
    got = mix.apply(big, rows.to(device), ops.to(device), m.to(device), fill=1)
    want = mix.reference_apply(two, th.tensor([0, 1]), ops, m, fill=1)
    assert th.equal(got.cpu(), want)
    del big
    th.cuda.empty_cache()


def test_two_runs_give_the_same_bits_and_a_side_stream_is_respected(device):
    shape = (3, 64, 64)
    src = _source(shape, th.float32, seed=3)
    rows = th.tensor(ROWS)
    ops, m = _op_sets(*shape)[3], _mix_sets(*shape)[-1]
    src_d, rows_d, ops_d, m_d = src.to(device), rows.to(device), ops.to(device), m.to(device)
    a = mix.apply(src_d, rows_d, ops_d, m_d, fill=-1.5)
    b = mix.apply(src_d, rows_d, ops_d, m_d, fill=-1.5)
    assert _same_bits(a, b)
    want = mix.reference_apply(src, rows, ops, m, fill=-1.5)
    # the source is produced on a side stream behind some work; the launch must queue behind it on that stream
    side = th.cuda.Stream(device=device)
    late = th.zeros_like(src_d)
    mm = th.randn(2048, 2048, device=device)
    th.cuda.synchronize(device)
    with th.cuda.stream(side):
        for _ in range(8):
            mm = (mm @ mm).clamp_(-1.0, 1.0)
        late.copy_(src_d)
        got = mix.apply(late, rows_d, ops_d, m_d, fill=-1.5)
    side.synchronize()
    assert _same_bits(got.cpu(), want)


# ---- the loaders ----------------------------------------------------------------------------------------------------
AUG, MIX, NC = "d4,shift:2:zero,erase:5:0.7", "cutmix:1.0,mixup:0.4:0.3", 5


def test_resident_loader_yields_the_mixed_batch_its_primary_labels_and_targets(device):
    from marlclassification_amd.data import ResidentLoader, SyntheticImages
    from marlclassification_amd.train import ShardedBatchSampler

    ds = SyntheticImages(37, 3, 16, NC, seed=3)
    part = th.randperm(37, generator=th.Generator().manual_seed(1))[:31].tolist()
    bs = ShardedBatchSampler(part, 8, 0, 1, shuffle=True, seed=2)
    policy, mpolicy = augment.parse(AUG), mix.parse(MIX)
    for aug in (policy, None):
        rl = ResidentLoader(ds, part, bs, device, augment=aug, mix=mpolicy, nb_class=NC,
                            generator=th.Generator(device=device).manual_seed(77))
        twin = th.Generator(device=device).manual_seed(77)
        mixed = 0
        for e in range(2):
            bs.set_epoch(e)
            for (x, y, q), idx in zip(list(rl), list(bs)):
                ops = aug.draw(len(idx), twin, size=(16, 16)).cpu() if aug is not None else None
                m = mpolicy.draw(len(idx), twin, (16, 16)).cpu()
                want = mix.reference_apply(ds.x, th.tensor(idx), ops, m, "zero" if aug is not None else "reflect", 0)
                assert th.equal(x.cpu(), want)
                assert th.equal(y.cpu(), mix.primary_labels(ds.y[idx], m, 16, 16))
                assert th.equal(q.cpu(), mix.soft_targets(ds.y[idx], m, 16, 16, NC))
                assert q.dtype == th.float32 and q.is_cuda and q.shape == (len(idx), NC)
                mixed += int((m[:, 1] != 0).sum())
        assert mixed > 0, "no image was mixed"
    plain = ResidentLoader(ds, part, bs, device)
    assert all(len(batch) == 2 for batch in plain), "without a mix policy nothing changes"
    with pytest.raises(ValueError, match="nb_class"):
        ResidentLoader(ds, part, bs, device, mix=mpolicy)


def test_device_prefetcher_mixes_the_uploaded_batch(device):
    from torch.utils.data import DataLoader

    from marlclassification_amd.data import DevicePrefetcher, SyntheticImages

    ds = SyntheticImages(20, 1, 28, 10, seed=4)
    policy, mpolicy = augment.parse(AUG), mix.parse(MIX)
    dl = DataLoader(ds, batch_size=8, shuffle=False)
    pf = DevicePrefetcher(dl, device, augment=policy, mix=mpolicy, nb_class=10,
                          generator=th.Generator(device=device).manual_seed(5))
    twin = th.Generator(device=device).manual_seed(5)
    got = list(pf)
    assert len(got) == 3
    for k, (x, y, q) in enumerate(got):
        lo = 8 * k
        ops = policy.draw(x.shape[0], twin, size=(28, 28)).cpu()
        m = mpolicy.draw(x.shape[0], twin, (28, 28)).cpu()
        assert th.equal(x.cpu(), mix.reference_apply(ds.x[lo: lo + 8], None, ops, m, "zero", 0))
        assert th.equal(y.cpu(), mix.primary_labels(ds.y[lo: lo + 8], m, 28, 28))
        assert th.equal(q.cpu(), mix.soft_targets(ds.y[lo: lo + 8], m, 28, 28, 10))
    assert all(len(batch) == 2 for batch in DevicePrefetcher(dl, device, augment=policy))


def test_draw_targets_and_a_mixed_batch_make_no_host_synchronisation(device):
    from marlclassification_amd.data import ResidentLoader, SyntheticImages

    ds = SyntheticImages(24, 3, 16, NC, seed=3)
    g = th.Generator(device=device).manual_seed(3)
    rl = ResidentLoader(ds, range(24), [list(range(8)), list(range(8, 16))], device, augment=augment.parse(AUG),
                        mix=mix.parse(MIX), nb_class=NC, generator=g)
    first = next(iter(rl))  # (fills the resident set: that does synchronise, once)
    y = th.arange(8, device=device) % NC
    th.cuda.synchronize(device)
    th.cuda.set_sync_debug_mode("error")
    try:
        m = mix.parse(MIX).draw(8, g, (16, 16))
        lam, q, yp = mix.label_weights(m, 16, 16), mix.soft_targets(y, m, 16, 16, NC), mix.primary_labels(y, m, 16, 16)
        batches = list(rl)
    finally:
        th.cuda.set_sync_debug_mode("default")
    assert len(batches) == 2 and len(batches[0]) == 3 and batches[0][0].shape == first[0].shape == (8, 3, 16, 16)
    assert lam.shape == (8,) and q.shape == (8, NC) and yp.shape == (8,)
