"""GPU: the augmenting batch gather ``marl_batch_augment`` (``augment.apply``) against its definition
``augment.reference_apply`` on the CPU.  Every operation is data movement, so every comparison is ``torch.equal`` -
uint8 and fp32 (compared as bit patterns) alike.  Shapes are the smallest that reach every path of the launcher; each
case asserts the store width ``marl_batch_augment_plan`` reports.  Every destination sits inside a larger buffer whose
guard bytes must survive."""
import json

import pytest
import torch as th

from marlclassification_amd import augment
from tests.buffers import N_SRC, SENTINEL
from tests.buffers import guarded as _guarded
from tests.buffers import guards_intact as _guards_intact
from tests.buffers import same_bits as _same_bits
from tests.buffers import source as _source

pytestmark = pytest.mark.gpu

ROWS = [10, 0, 3, 3, 7]  # batch 5 from a resident set of 11 rows: repeated, unsorted
FILL = {th.uint8: 200, th.float32: -1.5}

# shape -> store bytes (uint8, fp32) with a 16-byte aligned destination
SHAPES = {
    (1, 28, 28): (4, 16),     # MNIST: W % 16 != 0
    (3, 33, 47): (1, 4),      # odd, non-square: element-wide stores; non-transposing codes only
    (3, 64, 64): (16, 16),
    (3, 256, 256): (16, 16),  # full 16-byte stores
    (3, 600, 600): (8, 16),   # AID: W * elt % 16 == 8 for uint8
}


def _op_cases(c, h, w):
    """every code alone and under an odd shift, the extreme shifts, rectangles; the 600 x 600 images take the extremes
    and the rectangles under fewer codes (the CPU reference is what costs time there)"""
    codes = tuple(range(8)) if h == w else (0, 2, 4, 6)
    small = h <= 256
    cases = []
    for d4 in codes:
        shifts = [(0, 0), (3, -5)]
        if small or d4 in (codes[1], codes[-1]):
            shifts += [(h - 1, w - 1), (-(h - 1), -(w - 1)), (-(h - 1), 2)]
        for dy, dx in shifts:
            cases.append([d4, dy, dx, 0, 0, 0, 0, 0])
    s = min(7, h, w)
    rects = [(0, 0, s, s), (0, w - s, s, s), (h - s, 0, s, s), (h - s, w - s, s, s),  # the four corners
             (h // 2 - 3, w // 2 - 3, 9, 9), (0, 0, h, w), (2, 3, 0, 5), (2, 3, 5, 0)]  # middle, full image, empty
    if h > 70:
        rects += [(60, 58, 10, 13), (1, 60, 3, 9)]  # over the edge of a 64-pixel tile / a band of stores
    if h > 140:
        rects += [(122, 120, 14, 12), (250, 250, 12, 12)]  # over the edge of a 128-pixel tile
    under = ((0, 0, 0), (codes[-1], 2, -1), (codes[1], -3, 4))
    for k, (ey, ex, eh, ew) in enumerate(rects):
        for d4, dy, dx in (under if small else (under[0], under[1 + k % 2])):
            cases.append([d4, dy, dx, ey, ex, eh, ew, 0])
    return th.tensor(cases, dtype=th.int32)


def _run_cases(device, shape, dtype, offset, want_store):
    src = _source(shape, dtype)
    src_d = src.to(device)
    cases = _op_cases(*shape)
    rows = th.tensor(ROWS)
    rows_d = rows.to(device)
    nb = len(ROWS)
    out_shape = (nb,) + tuple(shape)
    nbytes = th.Size(out_shape).numel() * src.element_size()
    buf, dst = _guarded(out_shape, dtype, device, offset)
    info = augment.plan(src_d, dst)
    assert info["store_bytes"] == want_store, info
    for mode in ("reflect", "zero"):
        for lo in range(0, cases.shape[0], nb):
            ops = cases[lo: lo + nb]
            if ops.shape[0] < nb:
                ops = th.cat([ops, cases[: nb - ops.shape[0]]])
            buf.fill_(SENTINEL)
            got = augment.apply(src_d, rows_d, ops.to(device), pad_mode=mode, fill=FILL[dtype], out=dst)
            assert got is dst
            want = augment.reference_apply(src, rows, ops, mode, FILL[dtype])
            same = _same_bits(dst.cpu(), want)
            if not same:
                bad = [(b, ops[b].tolist()) for b in range(nb) if not _same_bits(dst[b].cpu(), want[b])]
                pytest.fail(f"{shape} {dtype} {mode}: images differ under ops {bad}")
            assert _guards_intact(buf, offset, nbytes), f"{shape} {dtype} {mode}: guard bytes overwritten, ops {ops.tolist()}"


@pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_every_code_shift_pad_mode_and_rectangle(device, shape, dtype):
    _run_cases(device, shape, dtype, 0, SHAPES[shape][dtype == th.float32])


@pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", [(3, 64, 64), (1, 28, 28)], ids=lambda s: "x".join(map(str, s)))
def test_destination_offset_by_four_bytes_takes_narrow_stores(device, shape, dtype):
    _run_cases(device, shape, dtype, 4, 4)


@pytest.mark.parametrize("shape,dtype,store", [((3, 33, 33), th.uint8, 1), ((3, 33, 33), th.float32, 4),
                                               ((1, 3, 3), th.uint8, 1), ((2, 7, 7), th.uint8, 1)],
                         ids=["3x33x33-u8", "3x33x33-f32", "1x3x3-u8", "2x7x7-u8"])
def test_odd_square_images_take_the_transposing_paths_with_narrow_stores(device, shape, dtype, store):
    """Square, so all eight codes run: uint8 rows that are no multiple of 4 bytes (byte stores behind the tile, ragged
    last quads of the dword loads, columns past the image inside a dword), and images narrower than 4 pixels (the
    per-pixel tile loop in its uint8 form)."""
    _run_cases(device, shape, dtype, 0, store)


@pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
def test_null_rows_and_null_ops(device, dtype):
    shape = (3, 64, 64)
    src = _source(shape, dtype)
    src_d = src.to(device)
    rows = th.tensor(ROWS)
    ops = _op_cases(*shape)[7: 7 + N_SRC]
    # ops == NULL: index_select, bit for bit
    assert _same_bits(augment.apply(src_d, rows.to(device)), src_d.index_select(0, rows.to(device)))
    # rows == NULL: row b for image b (an uploaded batch)
    got = augment.apply(src_d, None, ops.to(device), fill=FILL[dtype])
    assert _same_bits(got.cpu(), augment.reference_apply(src, None, ops, fill=FILL[dtype]))
    # both NULL: a copy
    assert _same_bits(augment.apply(src_d), src_d)
    with pytest.raises(RuntimeError, match="overlaps"):
        augment.apply(src_d, out=src_d)
    with pytest.raises(RuntimeError, match="overlaps"):
        augment.apply(src_d, rows.to(device)[:2], out=src_d[4:6])
    with pytest.raises(TypeError):
        augment.apply(src_d.to(th.float64))
    with pytest.raises(ValueError):
        augment.apply(src_d, rows.to(device).int())
    with pytest.raises(RuntimeError, match="GPU"):
        augment.apply(src)


@pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", [(3, 64, 64), (2, 33, 47)], ids=lambda s: "x".join(map(str, s)))
def test_hostile_device_values_are_sanitised(device, shape, dtype):
    """Built so that nothing can leave an allocation even if the clamping were wrong: ``src`` is rows 2 .. 8 of a
    12-row buffer whose other rows hold a value the images do not contain, and the hostile values are small."""
    c, h, w = shape
    mark = 7 if dtype == th.uint8 else 12345.0
    whole = _source(shape, dtype, n=12, seed=5)
    if dtype == th.uint8:
        whole[whole == mark] = 8
    whole[:2], whole[9:] = mark, mark
    whole_d = whole.to(device)
    src, src_d = whole[2:9], whole_d[2:9]
    n_src = src.shape[0]
    assert src_d.is_contiguous() and src_d.data_ptr() == whole_d.data_ptr() + 2 * whole_d[0].numel() * whole.element_size()
    rows = th.tensor([-1, n_src + 1, n_src, 3, -2, 0, n_src - 1, 5])
    ops = th.tensor([[11, h + 3, 0, 0, 0, 0, 0, 0],
                     [0, 0, -(w + 3), 0, 0, 0, 0, 0],
                     [15, -(h + 3), w + 3, 0, 0, 0, 0, 0],
                     [2, 0, 0, h - 2, w - 3, 9, 9, 0],
                     [9, 0, 0, -4, -4, 7, 7, 0],
                     [-1, 1, 1, 2, 2, -3, 4, 0],
                     [6, 2, -2, -3, 1, h + 9, w + 9, 5],
                     [4, h + 3, w + 3, h + 2, w + 2, 3, 3, 0]], dtype=th.int32)
    for mode in ("reflect", "zero"):
        buf, dst = _guarded((rows.shape[0],) + tuple(shape), dtype, device)
        augment.apply(src_d, rows.to(device), ops.to(device), pad_mode=mode, fill=FILL[dtype], out=dst)
        got = dst.cpu()
        assert _same_bits(got, augment.reference_apply(src, rows, ops, mode, FILL[dtype])), mode
        assert not bool((got == mark).any()), "a pixel from outside the source rows"
        assert _guards_intact(buf, 0, got.numel() * got.element_size())


def test_source_offsets_are_64_bit(device):
    """A uint8 set of more than 2^32 bytes (nothing filled but the rows used): the last row and row 0."""
    n, shape = 21846, (3, 256, 256)
    assert n * 3 * 256 * 256 > 2**32
    big = th.empty((n,) + shape, dtype=th.uint8, device=device)
    two = _source(shape, th.uint8, n=2, seed=9)
    big[n - 1].copy_(two[0])
    big[0].copy_(two[1])
    for code in (0, 2, 3):
        rows = th.tensor([n - 1, 0, n - 1])
        ops = th.tensor([[code, 0, 0, 0, 0, 0, 0, 0], [code, 3, -5, 0, 0, 0, 0, 0], [code ^ 4, -2, 7, 9, 9, 30, 30, 0]],
                        dtype=th.int32)
        got = augment.apply(big, rows.to(device), ops.to(device), fill=1)
        want = augment.reference_apply(two, th.tensor([0, 1, 0]), ops, fill=1)
        assert th.equal(got.cpu(), want), code
    del big
    th.cuda.empty_cache()


def test_two_runs_give_the_same_bits_and_a_side_stream_is_respected(device):
    shape = (3, 64, 64)
    src = _source(shape, th.float32, seed=3)
    ops = _op_cases(*shape)[11: 11 + len(ROWS)]
    rows = th.tensor(ROWS)
    src_d, rows_d, ops_d = src.to(device), rows.to(device), ops.to(device)
    a = augment.apply(src_d, rows_d, ops_d, fill=-1.5)
    b = augment.apply(src_d, rows_d, ops_d, fill=-1.5)
    assert _same_bits(a, b)
    want = augment.reference_apply(src, rows, ops, fill=-1.5)
    # the source is produced on a side stream behind some work; the launch must queue behind it on that stream
    side = th.cuda.Stream(device=device)
    late = th.zeros_like(src_d)
    m = th.randn(2048, 2048, device=device)
    th.cuda.synchronize(device)
    with th.cuda.stream(side):
        for _ in range(8):
            m = (m @ m).clamp_(-1.0, 1.0)
        late.copy_(src_d)
        got = augment.apply(late, rows_d, ops_d, fill=-1.5)
    side.synchronize()
    assert _same_bits(got.cpu(), want)


# ---- the loaders ----------------------------------------------------------------------------------------------------
SPEC = "d4,shift:2:zero,erase:5:0.7"


def test_resident_loader_draws_and_gathers_in_one_launch(device):
    from marlclassification_amd.data import ResidentLoader, SyntheticImages
    from marlclassification_amd.train import ShardedBatchSampler

    ds = SyntheticImages(37, 3, 16, 5, seed=3)
    part = th.randperm(37, generator=th.Generator().manual_seed(1))[:31].tolist()
    bs = ShardedBatchSampler(part, 8, 0, 1, shuffle=True, seed=2)
    policy = augment.parse(SPEC)
    rl = ResidentLoader(ds, part, bs, device, augment=policy,
                        generator=th.Generator(device=device).manual_seed(77))
    twin = th.Generator(device=device).manual_seed(77)
    plain = ResidentLoader(ds, part, bs, device)
    seen = 0
    for e in range(2):
        bs.set_epoch(e)
        for (x, y), (xp, yp), idx in zip(list(rl), list(plain), list(bs)):
            ops = policy.draw(len(idx), twin, size=(16, 16)).cpu()
            assert th.equal(x.cpu(), augment.reference_apply(ds.x, th.tensor(idx), ops, "zero", 0))
            assert th.equal(y.cpu(), ds.y[idx]) and th.equal(yp.cpu(), ds.y[idx])
            assert th.equal(xp.cpu(), ds.x[idx])  # augment=None: today's batches
            seen += int(not th.equal(x.cpu(), ds.x[idx]))
    assert seen > 0, "no batch was augmented"
    with pytest.raises(ValueError, match="square"):
        wide = SyntheticImages(8, 3, 16, 5)
        wide.x = wide.x[:, :, :, :12].contiguous()
        next(iter(ResidentLoader(wide, range(8), [[0, 1]], device, augment=policy)))


def test_draw_and_an_augmented_batch_make_no_host_synchronisation(device):
    """The trainer runs ahead of the device; a draw that uploaded a host tensor would make the host wait for the previous
    step at every batch.  Every spec form draws, and a resident loader yields a batch, with torch's synchronisation
    debugging set to raise."""
    from marlclassification_amd.data import ResidentLoader, SyntheticImages

    ds = SyntheticImages(24, 3, 16, 5, seed=3)
    policy = augment.parse(SPEC)
    g = th.Generator(device=device).manual_seed(3)
    rl = ResidentLoader(ds, range(24), [list(range(8)), list(range(8, 16))], device, augment=policy, generator=g)
    first = next(iter(rl))  # (fills the resident set: that does synchronise, once)
    pinned = th.tensor([3, 1, 2, 0], dtype=th.long).pin_memory()
    th.cuda.synchronize(device)
    th.cuda.set_sync_debug_mode("error")
    try:
        drawn = [augment.parse(s).draw(64, g, size=(16, 16))
                 for s in ("hflip", "vflip", "hflip,vflip", "rot90", "d4", "shift:3", "erase:4", SPEC)]
        rows = pinned.to(device, non_blocking=True)
        ops = policy.draw(4, g, size=(16, 16))
        out = augment.apply(rl._x, rows, ops, pad_mode=policy.pad_mode, fill=policy.fill)
        batches = list(rl)
    finally:
        th.cuda.set_sync_debug_mode("default")
    assert len(batches) == 2 and batches[0][0].shape == first[0].shape == (8, 3, 16, 16)
    assert out.shape == (4, 3, 16, 16)
    for s, d in zip(("hflip", "vflip", "hflip,vflip", "rot90", "d4"), drawn):
        assert set(d[:, 0].tolist()) == set(augment.parse(s).group())


def test_device_prefetcher_augments_the_uploaded_batch(device):
    from torch.utils.data import DataLoader

    from marlclassification_amd.data import DevicePrefetcher, SyntheticImages

    ds = SyntheticImages(20, 1, 28, 10, seed=4)
    policy = augment.parse(SPEC)
    dl = DataLoader(ds, batch_size=8, shuffle=False)
    pf = DevicePrefetcher(dl, device, augment=policy, generator=th.Generator(device=device).manual_seed(5))
    twin = th.Generator(device=device).manual_seed(5)
    got, plain = list(pf), list(DevicePrefetcher(dl, device))
    assert len(got) == len(plain) == 3
    for k, ((x, y), (xp, yp)) in enumerate(zip(got, plain)):
        lo = 8 * k
        ops = policy.draw(x.shape[0], twin, size=(28, 28)).cpu()
        assert th.equal(x.cpu(), augment.reference_apply(ds.x[lo: lo + 8], None, ops, "zero", 0))
        assert th.equal(xp.cpu(), ds.x[lo: lo + 8]) and th.equal(y.cpu(), ds.y[lo: lo + 8]) and th.equal(yp.cpu(), y.cpu())


# ---- through the trainer and the command line -----------------------------------------------------------------------
ACTIONS = [[1, 0], [-1, 0], [0, 1], [0, -1]]


def _mnist_model(device, seed):
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import MnistCnn

    th.manual_seed(seed)
    return ModelsWrapper(MnistCnn(6), 32, 32, 8, 12, 8, 2, 4, 10, 48, 48).to(device)


def test_a_train_step_on_an_augmented_batch_equals_the_step_on_the_materialised_batch(device):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.training import Trainer

    resident = _source((1, 28, 28), th.uint8, seed=21)
    rows = th.tensor([10, 0, 3, 3, 7, 1, 9, 2])
    ops = augment.parse("d4,shift:3,erase:6").draw(8, th.Generator().manual_seed(3), size=(28, 28))
    y = th.randint(0, 10, (8,), generator=th.Generator().manual_seed(4)).to(device)
    materialised = augment.reference_apply(resident, rows, ops)
    assert not th.equal(materialised, resident[rows])
    params = []
    for fused in (True, False):
        model = _mnist_model(device, 99)
        sampler = EpisodeSampler(MultiAgent(3, model), Environment(ACTIONS, 6), 4)
        trainer = Trainer(model, 10, 1e-3, 0.99)
        x = (augment.apply(resident.to(device), rows.to(device), ops.to(device)) if fused
             else materialised.to(device))
        trainer.train_step(x, y, sampler)
        th.cuda.synchronize(device)
        params.append({n: p.detach().clone() for n, p in model.named_parameters()})
    assert params[0].keys() == params[1].keys()
    for n in params[0]:
        assert th.equal(params[0][n], params[1][n]), n


def test_tta_over_the_d4_views_is_the_mean_of_eight_explicit_episodes(device, tmp_path):
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

    def config(tta):
        return EvalConfig(img_size=28, state_dict_path=str(tmp_path / "sd.pt"), batch_size=8,
                          json_path=str(tmp_path / "marl.json"), dataset_path=str(root),
                          output_dir=str(tmp_path / f"out_{tta}"), greedy=True, tta=tta)

    def explicit(views):
        """eval_main's own sequence (same seed, same random-number consumption, so the same shuffle and the same
        episode draws), every view materialised by reference_apply on the CPU"""
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
                preds = []
                for v in range(views.shape[0]):
                    xv = augment.reference_apply(x.cpu(), None, views[v: v + 1].expand(x.shape[0], -1)).to(device)
                    preds.append(sampler.run_episode_get_last_step(xv).prediction.mean(dim=0))
                pred = preds[0]
                for p in preds[1:]:
                    pred = pred + p
                meter.add(pred / len(preds) if len(preds) > 1 else pred, y)
        return meter.conf_mat().cpu()

    for tta in ("d4", None):
        th.manual_seed(1234)
        got = eval_main(main_config, config(tta)).conf_mat().cpu()
        th.manual_seed(1234)
        views = augment.parse(tta).views() if tta else th.zeros(1, 8, dtype=th.int32)
        assert views.shape[0] == (8 if tta else 1)
        assert th.equal(got, explicit(views)), tta
        assert int(got.sum()) == 21
    assert json.loads((tmp_path / "marl.json").read_text()).get("tta") is None
