"""Host side of the device-side augmentation (no GPU): the definition ``augment.reference_apply`` against torch's own
flips / rotations / padding, its sanitising, the spec grammar and the draws of ``augment.Policy``, the entries' place
beside the versioned ABI, the library's guards (host checks that return before any HIP call), the command line, and the
loaders with ``augment=None``."""
import ctypes as C
import json
import math
import os
import re

import pytest
import torch as th
import torch.nn.functional as F

from marlclassification_amd import _lib, augment
from marlclassification_amd.__main__ import build_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _images(n, c, h, w, seed=0, dtype=th.uint8):
    g = th.Generator().manual_seed(seed)
    if dtype == th.uint8:
        return th.randint(0, 256, (n, c, h, w), dtype=th.uint8, generator=g)
    return th.randn(n, c, h, w, generator=g)


def _ops(*rows):
    return th.tensor([list(r) + [0] * (8 - len(r)) for r in rows], dtype=th.int32)


# ---- the definition -------------------------------------------------------------------------------------------------
TORCH_FORM = {
    0: lambda x: x,
    2: lambda x: x.flip(-1),
    4: lambda x: x.flip(-2),
    6: lambda x: th.rot90(x, 2, (-2, -1)),
    1: lambda x: x.transpose(-2, -1),
    3: lambda x: th.rot90(x, 1, (-2, -1)),
    5: lambda x: th.rot90(x, -1, (-2, -1)),
    7: lambda x: x.transpose(-2, -1).flip(-1).flip(-2),
}


@pytest.mark.parametrize("dtype", [th.uint8, th.float32])
@pytest.mark.parametrize("code", range(8))
def test_the_eight_codes_are_torchs_flips_and_rotations(code, dtype):
    x = _images(2, 3, 7, 7, seed=code, dtype=dtype)
    got = augment.reference_apply(x, None, _ops([code], [code]))
    assert th.equal(got, TORCH_FORM[code](x))


@pytest.mark.parametrize("code", [0, 2, 4, 6])
def test_non_transposing_codes_on_a_non_square_image(code):
    x = _images(2, 3, 5, 9, seed=10 + code)
    assert th.equal(augment.reference_apply(x, None, _ops([code], [code])), TORCH_FORM[code](x))


def test_transposing_bit_is_dropped_on_a_non_square_image():
    x = _images(1, 2, 5, 9, seed=3)
    for code in (1, 3, 5, 7):
        assert th.equal(augment.reference_apply(x, None, _ops([code])), TORCH_FORM[code & 6](x))


@pytest.mark.parametrize("dy,dx", [(0, 0), (2, -3), (-4, 1), (6, 6), (-6, -6), (3, -5)])
def test_shift_is_a_crop_of_the_padded_image(dy, dx):
    h, w, t = 7, 9, 6
    x = _images(2, 3, h, w, seed=5, dtype=th.float32)
    # out[y, x] = padded[y - dy + t, x - dx + t]
    pad_r = F.pad(x, (t, t, t, t), mode="reflect")
    pad_z = F.pad(x, (t, t, t, t), mode="constant", value=0.25)
    crop = (slice(None), slice(None), slice(t - dy, t - dy + h), slice(t - dx, t - dx + w))
    ops = _ops([0, dy, dx], [0, dy, dx])
    assert th.equal(augment.reference_apply(x, None, ops, "reflect"), pad_r[crop])
    assert th.equal(augment.reference_apply(x, None, ops, "zero", fill=0.25), pad_z[crop])
    xu = _images(2, 1, h, w, seed=6)
    assert th.equal(augment.reference_apply(xu, None, ops, "zero", fill=77),
                    F.pad(xu, (t, t, t, t), mode="constant", value=77)[crop])


def test_shift_then_code_then_erase_last():
    x = _images(3, 2, 7, 7, seed=8)
    ops = _ops([3, 1, -2, 2, 3, 3, 2])
    rows = th.tensor([2])
    # the shift acts on OUTPUT coordinates, the code maps them into the source: out = crop_of_padded(rot90(src))
    want = F.pad(th.rot90(x[2:3], 1, (-2, -1)).float(), (3, 3, 3, 3), mode="reflect")[:, :, 2: 9, 5: 12].to(th.uint8)
    want[:, :, 2:5, 3:5] = 9
    assert th.equal(augment.reference_apply(x, rows, ops, "reflect", fill=9), want)


def test_rows_gather_and_defaults():
    x = _images(6, 2, 4, 4, seed=1)
    rows = th.tensor([5, 0, 5, 3])
    assert th.equal(augment.reference_apply(x, rows), x[rows])
    assert th.equal(augment.reference_apply(x), x)
    assert th.equal(augment.reference_apply(x, None, _ops([2], [0])), th.stack([x[0].flip(-1), x[1]]))
    with pytest.raises(ValueError):
        augment.reference_apply(x, rows, _ops([0]))
    with pytest.raises(ValueError, match="wrap"):
        augment.reference_apply(x, pad_mode="wrap")


def test_sanitising_of_hostile_values():
    h, w = 5, 5
    x = _images(4, 2, h, w, seed=2)
    big = 2**31 - 1
    # d4 & 7; rows clamped; shifts clamped to n - 1; rectangles intersected with the image (64-bit sum)
    assert th.equal(augment.reference_apply(x, th.tensor([0]), _ops([11])), TORCH_FORM[3](x[0:1]))
    assert th.equal(augment.reference_apply(x, th.tensor([-1, 5, 2**40]), None), x[[0, 3, 3]])
    for mode in ("reflect", "zero"):
        assert th.equal(augment.reference_apply(x, None, _ops([0, h + 3, -big]), mode, fill=1),
                        augment.reference_apply(x, None, _ops([0, h - 1, -(w - 1)]), mode, fill=1))
    got = augment.reference_apply(x, th.tensor([1]), _ops([0, 0, 0, 3, -2, big, 4]), fill=200)
    want = x[1:2].clone()
    want[:, :, 3:, :2] = 200
    assert th.equal(got, want)
    for rect in ([0, 0, 0, 1, 1, 0, 3], [0, 0, 0, 1, 1, 3, 0], [0, 0, 0, 1, 1, -2, 3], [0, 0, 0, 7, 1, 2, 2],
                 [0, 0, 0, -big, -big, 5, 5]):
        assert th.equal(augment.reference_apply(x, th.tensor([1]), _ops(rect), fill=200), x[1:2]), rect
    one = _images(1, 1, 1, 1, seed=0)
    assert th.equal(augment.reference_apply(one, None, _ops([7, 5, -5])), one)


# ---- the spec grammar -----------------------------------------------------------------------------------------------
def test_parse_every_token_and_defaults():
    p = augment.parse("hflip")
    assert (p.hflip, p.vflip, p.rot90, p.d4, p.shift, p.erase) == (True, False, False, False, 0, 0)
    assert p.pad_mode == "reflect" and p.erase_p == 0.5 and p.fill == 0 and p.spec == "hflip"
    p = augment.parse("vflip, rot90,d4,shift:4:zero,erase:8:0.25")
    assert (p.hflip, p.vflip, p.rot90, p.d4) == (False, True, True, True)
    assert (p.shift, p.pad_mode, p.erase, p.erase_p) == (4, "zero", 8, 0.25)
    assert augment.parse("shift:3").pad_mode == "reflect" and augment.parse("shift:3:reflect").shift == 3
    assert augment.parse("erase:5").erase_p == 0.5 and augment.parse("erase:5:1").erase_p == 1.0
    with pytest.raises(Exception):
        p.shift = 1  # frozen


@pytest.mark.parametrize("bad,token", [("flip", "flip"), ("hflip,rot", "rot"), ("", ""), ("hflip,,vflip", ""),
                                       ("shift", "shift"), ("shift:x", "shift:x"), ("shift:-1", "shift:-1"),
                                       ("shift:2:wrap", "shift:2:wrap"), ("shift:2:zero:1", "shift:2:zero:1"),
                                       ("erase:0", "erase:0"), ("erase:4:1.5", "erase:4:1.5"),
                                       ("erase:4:nan", "erase:4:nan"), ("erase:4:p", "erase:4:p"),
                                       ("hflip:1", "hflip:1"), ("d4,rot180", "rot180")])
def test_parse_names_the_bad_token(bad, token):
    with pytest.raises(ValueError, match=re.escape(f'"{token}"')):
        augment.parse(bad)


def test_groups():
    g = lambda s: augment.parse(s).group()  # noqa: E731
    assert g("hflip") == (0, 2) and g("vflip") == (0, 4) and g("hflip,vflip") == (0, 2, 4, 6)
    assert g("rot90") == (0, 3, 6, 5)
    for s in ("d4", "rot90,hflip", "rot90,vflip", "rot90,hflip,vflip", "d4,hflip"):
        assert sorted(g(s)) == list(range(8)), s
    assert g("shift:2") == (0,) and g("erase:3") == (0,)


def test_views_are_deterministic_without_repeats_and_refuse_random_parts():
    for s in ("hflip", "vflip", "hflip,vflip", "rot90", "d4"):
        p = augment.parse(s)
        v = p.views()
        assert v.dtype == th.int32 and v.shape == (len(p.group()), 8) and th.equal(v, p.views())
        assert tuple(v[:, 0].tolist()) == p.group() and len(set(p.group())) == len(p.group())
        assert not v[:, 1:].any()
    for s in ("hflip,shift:2", "d4,erase:4", "shift:0,erase:1"):
        with pytest.raises(ValueError):
            augment.parse(s).views()
        with pytest.raises(ValueError):
            augment.parse_tta(s)
    assert augment.parse("hflip,shift:0").views().shape == (2, 8)


def test_a_transposing_group_refuses_non_square_images():
    for s in ("rot90", "d4", "rot90,hflip"):
        with pytest.raises(ValueError, match="square"):
            augment.parse(s).check_size(33, 47)
        augment.parse(s).check_size(47, 47)
    augment.parse("hflip,vflip,shift:3,erase:4").check_size(33, 47)


# ---- the draws ------------------------------------------------------------------------------------------------------
def test_draw_repeats_under_a_seed_and_covers_the_group_and_the_shift_range():
    n, t, s, prob = 4096, 3, 6, 0.3
    for spec, group in (("rot90", (0, 3, 6, 5)), ("hflip", (0, 2)), ("d4", tuple(range(8)))):
        p = augment.parse(f"{spec},shift:{t},erase:{s}:{prob}")
        a = p.draw(n, th.Generator().manual_seed(5), size=(32, 40))
        b = p.draw(n, th.Generator().manual_seed(5), size=(32, 40))
        c = p.draw(n, th.Generator().manual_seed(6), size=(32, 40))
        assert a.dtype == th.int32 and a.shape == (n, 8) and th.equal(a, b) and not th.equal(a, c)
        assert set(a[:, 0].tolist()) == set(group)  # every code of the group, none outside it
        for col in (1, 2):
            assert a[:, col].min().item() == -t and a[:, col].max().item() == t
        on = a[:, 5] != 0
        assert th.equal(a[:, 5], a[:, 6]) and set(a[:, 5].tolist()) <= {0, s}
        assert abs(on.float().mean().item() - prob) <= 4.0 * math.sqrt(prob * (1 - prob) / n)
        assert a[:, 3].min().item() == 0 and a[:, 3].max().item() == 32 - s
        assert a[:, 4].min().item() == 0 and a[:, 4].max().item() == 40 - s
        assert not a[:, 7].any()
        counts = th.bincount(a[:, 0].long(), minlength=8)[list(group)].float()
        pg = 1.0 / len(group)
        assert (counts / n - pg).abs().max().item() <= 4.0 * math.sqrt(pg * (1 - pg) / n)  # uniform over the group


def test_draw_without_random_parts_and_without_a_size():
    p = augment.parse("hflip")
    a = p.draw(64, th.Generator().manual_seed(1))
    assert set(a[:, 0].tolist()) == {0, 2} and not a[:, 1:].any()
    with pytest.raises(ValueError, match="size"):
        augment.parse("erase:4").draw(8, th.Generator().manual_seed(1))
    assert not augment.parse("shift:0").draw(8, th.Generator().manual_seed(1)).any()


# ---- the library: a header of its own, the versioned ABI untouched, guards without a device -------------------------
def _declared(header):
    with open(os.path.join(ROOT, "include", header), "r", encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(marl_[a-z0-9_]+)\s*\(", text))


def test_entries_live_beside_the_versioned_abi():
    assert _declared("marl_hip_augment.h") == set(_lib.AUGMENT_ENTRIES) == {"marl_batch_augment",
                                                                           "marl_batch_augment_plan"}
    assert not set(_lib.AUGMENT_ENTRIES) & _declared("marl_hip.h")
    assert len(_lib.EXPORTS) == 57 and not set(_lib.AUGMENT_ENTRIES) & set(_lib.EXPORTS)
    assert _lib.MARL_ABI_VERSION == 5 and _lib.load().marl_abi_version() == 5
    assert set(_lib.AUGMENT_ENTRIES) <= set(_lib._HOOKS)


def _codes():
    with open(os.path.join(ROOT, "include", "marl_hip.h"), "r", encoding="utf-8") as f:
        text = f.read()
    return tuple(int(re.search(rf"#define {n} \((-?\d+)\)", text).group(1)) for n in ("MARL_EINVAL", "MARL_ELIMIT"))


def test_library_guards_answer_without_a_device():
    """Every refusal below is host arithmetic on the arguments: no pointer is dereferenced, no HIP call is made."""
    lib = _lib.load()
    einval, elimit = _codes()
    src, dst = 0x10000000, 0x20000000  # (never dereferenced)

    def call(src=src, n_src=4, dst=dst, batch=2, c=3, h=8, w=8, elt=1, pad=1):
        return lib.marl_batch_augment(src, n_src, dst, None, None, batch, c, h, w, elt, pad, 0, None)

    for kw in ({"elt": 2}, {"elt": 0}, {"elt": 8}, {"pad": 2}, {"pad": -1}, {"batch": 0}, {"n_src": 0}, {"c": 0},
               {"h": -1}, {"w": 0}, {"src": None}, {"dst": None},
               {"dst": src}, {"dst": src + 4 * 192 - 1}, {"dst": src - 2 * 192 + 1},  # overlap at either end
               {"elt": 4, "dst": dst + 2},  # a misaligned fp32 pointer
               {"n_src": 1}):  # rows == NULL needs a row per image
        assert call(**kw) == einval, kw
        assert b"batch_augment" in lib.marl_last_error(), kw
    assert call(c=1, h=1 << 16, w=1 << 15) == elimit and b"batch_augment" in lib.marl_last_error()
    assert call(batch=1 << 30, n_src=1 << 30, c=64, h=512, w=512, dst=1 << 60) == elimit


def test_plan_is_host_arithmetic():
    lib = _lib.load()
    einval, _ = _codes()
    info = augment.AugmentPlan()

    def store(c, h, w, elt, dst=0x20000000):
        assert lib.marl_batch_augment_plan(c, h, w, elt, 0x10000000, dst, C.byref(info)) == 0
        d = info.as_dict()
        assert d["lds_bytes"] == 128 * 132 and d["tr_tile"] == (128 if elt == 1 else 64) and d["tile_w"] == w
        return d["store_bytes"]

    assert [store(1, 28, 28, e) for e in (1, 4)] == [4, 16]
    assert [store(3, 33, 47, e) for e in (1, 4)] == [1, 4]
    assert [store(3, 64, 64, e) for e in (1, 4)] == [16, 16]
    assert [store(3, 600, 600, e) for e in (1, 4)] == [8, 16]
    assert [store(3, 256, 256, e, 0x20000004) for e in (1, 4)] == [4, 4]
    assert store(3, 256, 256, 1, 0x20000008) == 8 and store(3, 256, 256, 1, 0x20000001) == 1
    assert store(1, 6, 6, 1) == 1 and store(1, 6, 6, 4) == 8
    # one grid serves both forms: bands of 1024 stores, or (square images) tiles
    assert lib.marl_batch_augment_plan(3, 256, 256, 1, 0, 0x20000000, C.byref(info)) == 0
    assert info.blocks_per_image == 12 and info.band_vectors == 1024 and info.tile_h == 64
    assert lib.marl_batch_augment_plan(3, 256, 256, 4, 0, 0x20000000, C.byref(info)) == 0
    assert info.blocks_per_image == 48
    assert lib.marl_batch_augment_plan(3, 8, 8, 2, 0, 0x20000000, C.byref(info)) == einval
    assert lib.marl_batch_augment_plan(3, 8, 8, 1, 0, 0x20000000, None) == einval
    assert b"batch_augment_plan" in lib.marl_last_error()


def test_apply_refuses_cpu_tensors_and_bad_arguments():
    x = _images(2, 1, 4, 4)
    with pytest.raises(RuntimeError, match="GPU"):
        augment.apply(x)
    with pytest.raises(ValueError, match="wrap"):
        augment.apply(x, pad_mode="wrap")


# ---- the command line -----------------------------------------------------------------------------------------------
def _parse(*mode):
    return build_parser().parse_args(["--run-id", "x", *mode])


TEST_MODE = ["test", "--dataset-path", "d", "--json-path", "j", "--state-dict-path", "s", "-o", "o"]


def test_parser_flags():
    assert _parse("train", "-o", "out").augment is None and _parse(*TEST_MODE).tta is None
    assert _parse("train", "-o", "out", "--augment", "d4,shift:8,erase:32").augment == "d4,shift:8,erase:32"
    assert _parse(*TEST_MODE, "--tta", "d4").tta == "d4"
    for bad in (["--augment", "flip"], ["--augment", "shift:x"], ["--augment", ""], ["--tta", "d4"]):
        with pytest.raises(SystemExit):
            _parse("train", "-o", "out", *bad)
    for bad in (["--tta", "rot"], ["--tta", "hflip,shift:2"], ["--tta", "erase:4"], ["--augment", "d4"]):
        with pytest.raises(SystemExit):
            _parse(*TEST_MODE, *bad)
    infer = ["infer", "--images", "i", "--json-path", "j", "--state-dict-path", "s", "--class2idx", "c", "-o", "o"]
    with pytest.raises(SystemExit):
        _parse(*infer, "--tta", "d4")


def test_the_flags_reach_the_configs_and_stay_out_of_marl_json(tmp_path, monkeypatch):
    from marlclassification_amd import __main__ as cli
    from marlclassification_amd import eval as eval_mod
    from marlclassification_amd import train as train_mod
    from marlclassification_amd.config import EvalConfig, ModelConfig, TrainConfig

    seen = {}
    monkeypatch.setattr(train_mod, "train_main", lambda m, mc, tc, **kw: seen.update(train=tc, model=mc))
    monkeypatch.setattr(eval_mod, "eval_main", lambda m, ec: seen.update(eval=ec))
    cli.main(["--run-id", "x", "train", "-o", str(tmp_path), "--augment", "hflip,shift:2:zero"])
    cli.main(["--run-id", "x", *TEST_MODE, "--tta", "hflip,vflip"])
    assert seen["train"].augment == "hflip,shift:2:zero" and seen["eval"].tta == "hflip,vflip"
    cli.main(["--run-id", "x", "train", "-o", str(tmp_path)])
    cli.main(["--run-id", "x", *TEST_MODE])
    assert seen["train"].augment is None and seen["eval"].tta is None
    assert TrainConfig(img_size=28, nb_epoch=1, learning_rate=1e-3, batch_size=2, resources_dir="r", output_dir="o",
                       gamma=0.9).augment is None
    assert EvalConfig(img_size=28, state_dict_path="s", batch_size=2, json_path="j", dataset_path="d",
                      output_dir="o").tta is None
    path = tmp_path / "marl.json"
    seen["model"].save_marl_config(str(path))
    raw = json.loads(path.read_text())
    assert "augment" not in raw and "tta" not in raw and not hasattr(ModelConfig, "augment")


# ---- the loaders with augment=None ----------------------------------------------------------------------------------
def test_resident_loader_without_a_policy_yields_what_it_yielded():
    from marlclassification_amd.data import DevicePrefetcher, ResidentLoader, SyntheticImages
    from marlclassification_amd.train import ShardedBatchSampler

    ds = SyntheticImages(37, 3, 8, 5, seed=3)
    part = th.randperm(37, generator=th.Generator().manual_seed(1))[:31].tolist()
    bs = ShardedBatchSampler(part, 8, 0, 1, shuffle=True, seed=2)
    rl = ResidentLoader(ds, part, bs, "cpu", workers=0, chunk=4)
    assert rl.augment is None and rl.generator is None
    for e in range(2):
        bs.set_epoch(e)
        got, want = list(rl), list(bs)
        assert len(got) == len(want) == len(rl)
        for (x, y), idx in zip(got, want):
            assert th.equal(x, ds.x[idx]) and th.equal(y, ds.y[idx])
    # (a DevicePrefetcher iterates on a GPU only - tests/test_gpu_augment.py; here: it takes and keeps the arguments)
    pf = DevicePrefetcher([1, 2, 3], "cpu")
    assert pf.augment is None and pf.generator is None and len(pf) == 3
    g = th.Generator().manual_seed(1)
    pol = augment.parse("hflip")
    assert DevicePrefetcher([], "cpu", augment=pol, generator=g).generator is g
    assert ResidentLoader(ds, part, bs, "cpu", augment=pol, generator=g).augment is pol
