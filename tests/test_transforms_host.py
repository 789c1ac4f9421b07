"""CPU: the definition of the per-image input normalisation (``transforms.reference_stats`` / ``reference_coef`` /
``reference_apply``), its command-line spelling, the reference's six transform classes, the ``dataset`` mean / std and
the ``normalize`` key of ``marl.json``.  The yardstick of every numeric check is the direct float64 expression
``(x / 255 - mean) / std`` or ``(x / 255 - min) / (max - min)`` of the module docstring's table (fp32 sources: without
the 255), computed here with torch's own float64 ``mean`` / ``std`` / ``amin`` / ``amax``."""
import json

import pytest
import torch as th

from marlclassification_amd import transforms
from marlclassification_amd.__main__ import build_parser
from marlclassification_amd.config import EvalConfig, InferConfig, ModelConfig

STAT_MODES = ("normal", "channel-normal", "minmax", "channel-minmax")
# float64 against float64: both sides round O(N) additions of N <= 3 * 33 * 31 terms (2^-53 each, cancellation of the
# one-pass variance included: |mean| <= 3 std on these inputs), far below this relative bound
REL64 = 1e-10


def _images(dtype, shape, n=4, seed=0):
    g = th.Generator().manual_seed(seed + 13 * shape[0] + shape[1])
    if dtype == th.uint8:
        return th.randint(0, 256, (n,) + tuple(shape), dtype=th.uint8, generator=g)
    return th.randn((n,) + tuple(shape), generator=g) * 0.75 + 1.5


def _direct(x, spec):
    """the float64 yardstick: (scale64, offset64) [B, C] in units of the stored pixel, and the normalised batch"""
    spec = transforms.parse(spec)
    k = 255.0 if x.dtype == th.uint8 else 1.0
    xd = x.double() / k
    nb, c = x.shape[:2]
    flat = xd.reshape(nb, 1, -1).expand(nb, c, -1) if spec.whole_image else xd.reshape(nb, c, -1)
    if spec.mode in ("normal", "channel-normal"):
        a, b = flat.mean(-1), flat.std(-1)
    elif spec.mode in ("minmax", "channel-minmax"):
        a, b = flat.amin(-1), flat.amax(-1) - flat.amin(-1)
    elif spec.mode == "user-normal":
        a, b = (th.tensor(v, dtype=th.float64).expand(nb, c) for v in (spec.first, spec.second))
    else:
        lo, hi = (th.tensor(v, dtype=th.float64) for v in (spec.first, spec.second))
        a, b = lo.expand(nb, c), (hi - lo).expand(nb, c)
    return 1.0 / (k * b), -a / b, (xd - a[:, :, None, None]) / b[:, :, None, None]


USER = {1: ("user-normal:0.4:0.25", "user-minmax:0.1:0.9"),
        3: ("user-normal:0.485,0.456,0.406:0.229,0.224,0.225", "user-minmax:0.0,0.1,-0.5:1.0,0.8,2.0")}


# ---- the spelling ---------------------------------------------------------------------------------------------------
def test_parse_round_trips():
    for text in STAT_MODES + USER[1] + USER[3] + ("dataset",):
        spec = transforms.parse(text)
        assert transforms.parse(spec.spelling) == spec and transforms.parse(spec) is spec
    spec = transforms.parse("user-normal:0.1,0.2:0.3,0.7")
    assert spec.mode == "user-normal" and spec.first == (0.1, 0.2) and spec.second == (0.3, 0.7) and spec.is_user
    third = transforms.Spec("user-normal", (1.0 / 3.0,), (2.0 / 3.0,))
    assert transforms.parse(third.spelling) == third  # (repr of a float reads back to the same float)
    assert transforms.parse("normal").whole_image and not transforms.parse("channel-minmax").whole_image
    assert transforms.resolve(None) is None and transforms.resolve("none") is None
    assert transforms.resolve("minmax") == transforms.Spec("minmax")


@pytest.mark.parametrize("bad", ["", "norm", "normal:1", "user-normal", "user-normal:0.5", "user-normal:0.5:0.2:1",
                                 "user-normal:0.5,0.5:0.2", "user-normal:0.5:0", "user-minmax:0.3:0.3",
                                 "user-normal:a:b", "user-normal:nan:1", "user-minmax:0:inf", "dataset:1", "none",
                                 "user-normal:" + ",".join(["0"] * 17) + ":" + ",".join(["1"] * 17)])
def test_parse_rejections(bad):
    with pytest.raises(ValueError, match="normalize"):
        transforms.parse(bad)


def test_parse_rejects_what_is_no_string_and_resolve_refuses_dataset():
    with pytest.raises(ValueError):
        transforms.parse(3)
    with pytest.raises(ValueError, match="dataset"):
        transforms.resolve("dataset")
    with pytest.raises(ValueError, match="channels"):
        transforms.reference_apply(_images(th.uint8, (3, 4, 4)), None, USER[1][0])


# ---- the definition against the float64 yardstick -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 8, 8), (3, 33, 31)], ids=lambda s: "x".join(map(str, s)))
def test_reference_coef_against_the_direct_float64_statistics(dtype, shape):
    x = _images(dtype, shape)
    rec = transforms.reference_stats(x)
    assert rec.dtype == (th.int64 if dtype == th.uint8 else th.float64) and rec.shape == (4, shape[0], 4)
    flat = x.reshape(4, shape[0], -1)
    assert th.equal(rec[:, :, 2].to(flat.dtype), flat.amin(-1)) and th.equal(rec[:, :, 3].to(flat.dtype), flat.amax(-1))
    for spec in STAT_MODES + USER[shape[0]]:
        coef = transforms.reference_coef(rec, spec, shape, dtype == th.uint8)
        scale, offset, _ = _direct(x, spec)
        assert coef.dtype == th.float64 and coef.shape == (4, shape[0], 2)
        assert ((coef[:, :, 0] - scale).abs() <= REL64 * scale.abs()).all(), spec
        assert ((coef[:, :, 1] - offset).abs() <= REL64 * (offset.abs() + 1.0)).all(), spec


@pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 8, 8), (3, 33, 31)], ids=lambda s: "x".join(map(str, s)))
def test_reference_apply_against_the_float64_formula(dtype, shape):
    """bound per image: 4 * 2^-24 * (max|x| scale + |offset|) - two fp32 roundings of the result plus the two rounded
    coefficients (max|x| = 255 for uint8)"""
    x = _images(dtype, shape)
    rows = th.tensor([3, 0, 0, 2, -5, 99])  # repeated, and clamped to [0, 4)
    picked = x[rows.clamp(0, 3)]
    for spec in STAT_MODES + USER[shape[0]]:
        got = transforms.reference_apply(x, rows, spec)
        assert got.dtype == th.float32 and got.shape == (6,) + shape
        scale, offset, want = _direct(picked, spec)
        top = 255.0 if dtype == th.uint8 else picked.abs().amax(dim=(1, 2, 3)).double()[:, None]
        bound = (4.0 * 2.0 ** -24 * (top * scale.abs() + offset.abs())).amax(dim=1)  # per image
        err = (got.double() - want).abs().amax(dim=(1, 2, 3))
        assert (err <= bound).all(), (spec, err.tolist(), bound.tolist())
    assert th.equal(transforms.reference_apply(x, None, "normal"), transforms.reference_apply(x, th.arange(4), "normal"))


def test_reference_apply_multiplies_and_adds_in_two_rounded_steps():
    x = _images(th.uint8, (3, 8, 8))
    coef = transforms.reference_coef(transforms.reference_stats(x), "channel-normal", (3, 8, 8), True).float()
    prod = x.float() * coef[:, :, 0, None, None]
    assert th.equal(transforms.reference_apply(x, None, "channel-normal"), prod + coef[:, :, 1, None, None])


# ---- the reference's classes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3])
def test_the_six_classes_are_reference_apply_of_one_image(c):
    x = _images(th.float32, (c, 9, 11), n=1)[0]
    um, us = ([0.4], [0.25]) if c == 1 else ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    lo, hi = ([0.1], [0.9]) if c == 1 else ([0.0, 0.1, -0.5], [1.0, 0.8, 2.0])
    cases = [(transforms.NormalNorm(), "normal"), (transforms.ChannelNormalNorm(), "channel-normal"),
             (transforms.MinMaxNorm(), "minmax"), (transforms.ChannelMinMaxNorm(), "channel-minmax"),
             (transforms.UserNormalNorm(um, us), USER[c][0]), (transforms.UserMinMaxNorm(lo, hi), USER[c][1])]
    for tf, spec in cases:
        assert isinstance(tf, transforms.ImgTransform) and type(tf).__name__ in repr(tf)
        got = tf(x)
        assert got.shape == x.shape and got.dtype == th.float32
        assert th.equal(got, transforms.reference_apply(x.unsqueeze(0), None, spec)[0]), spec
    # ... which is what the reference's expressions compute, up to fp32 rounding
    xm, xs = x.reshape(c, -1).mean(-1).view(c, 1, 1), x.reshape(c, -1).std(-1).view(c, 1, 1)
    assert th.allclose(transforms.ChannelNormalNorm()(x), (x - xm) / xs, atol=1e-5, rtol=0)
    assert th.allclose(transforms.NormalNorm()(x), (x - x.mean()) / x.std(), atol=1e-5, rtol=0)
    assert th.allclose(transforms.MinMaxNorm()(x), (x - x.min()) / (x.max() - x.min()), atol=1e-6, rtol=0)
    assert th.allclose(transforms.UserNormalNorm(um, us)(x),
                       (x - th.tensor(um).view(c, 1, 1)) / th.tensor(us).view(c, 1, 1), atol=1e-5, rtol=0)
    with pytest.raises(TypeError):
        transforms.ImgTransform()
    with pytest.raises(ValueError):
        transforms.UserNormalNorm([0.5], [0.0])


def test_constant_planes_and_images_give_zeros():
    x = _images(th.uint8, (3, 6, 6), n=3)
    x[0] = 77          # a constant image
    x[1, 1] = 255      # one constant plane
    for mode in STAT_MODES:
        got = transforms.reference_apply(x, None, mode)
        assert bool(th.isfinite(got).all()), mode
        assert not got[0].any(), mode
        if mode.startswith("channel"):
            assert not got[1, 1].any() and got[1, 0].any() and got[1, 2].any(), mode
        else:
            assert got[1, 1].any(), mode  # (the image is not constant)
        assert got[2].any(), mode
    one = th.full((1, 1, 1, 1), 9, dtype=th.uint8)  # N == 1
    for mode in STAT_MODES:
        assert not transforms.reference_apply(one, None, mode).any()
    assert not transforms.reference_apply(th.full((1, 2, 3, 3), 0.25), None, "channel-normal").any()


# ---- the dataset mean / std -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [th.uint8, th.float32], ids=["u8", "f32"])
def test_dataset_spec_is_the_mean_and_std_of_the_set(dtype):
    x = _images(dtype, (3, 9, 7), n=13, seed=5)
    spec = transforms.dataset_spec(x, chunk=4)  # (13 = 4 + 4 + 4 + 1 images)
    assert spec.mode == "user-normal" and transforms.parse(spec.spelling) == spec
    xd = (x.double() / 255.0 if dtype == th.uint8 else x.double()).transpose(0, 1).reshape(3, -1)
    mean, std = xd.mean(-1), xd.std(-1)
    assert ((th.tensor(spec.first, dtype=th.float64) - mean).abs() <= REL64 * mean.abs()).all()
    assert ((th.tensor(spec.second, dtype=th.float64) - std).abs() <= REL64 * std).all()
    assert transforms.dataset_spec(x, chunk=100) == spec or dtype == th.float32  # (integers: any chunking)
    # the spec standardises the set: per-channel mean 0 and std 1 over the whole of it
    out = transforms.reference_apply(x, None, spec).double().transpose(0, 1).reshape(3, -1)
    assert out.mean(-1).abs().max().item() <= 1e-5 and (out.std(-1) - 1.0).abs().max().item() <= 1e-5
    flat = x.clone()
    flat[:, 1] = 3
    with pytest.raises(ValueError, match="constant"):
        transforms.dataset_spec(flat)


# ---- marl.json and the command line ---------------------------------------------------------------------------------
def _model_config(**kw):
    return ModelConfig(ft_extr_str="mnist", window_size=6, hidden_size_belief=32, hidden_size_action=32,
                       hidden_size_msg=8, hidden_size_msg_output=12, hidden_size_state=8, state_dim=2,
                       actions=[[1, 0], [-1, 0], [0, 1], [0, -1]], nb_class=10, hidden_size_linear_belief=48,
                       hidden_size_linear_action=48, **kw)


def test_marl_json_has_the_key_only_when_given(tmp_path):
    path = str(tmp_path / "marl.json")
    _model_config().save_marl_config(path)
    assert "normalize" not in json.load(open(path)) and ModelConfig.load_marl_config(path).normalize is None
    spelling = transforms.parse(USER[3][0]).spelling
    for text in ("channel-normal", spelling):
        _model_config(normalize=text).save_marl_config(path)
        assert json.load(open(path))["normalize"] == text
        back = ModelConfig.load_marl_config(path)
        assert back.normalize == text and transforms.resolve(back.normalize) == transforms.parse(text)


TEST_MODE = ["test", "--dataset-path", "d", "--json-path", "j", "--state-dict-path", "s", "-o", "o"]
INFER_MODE = ["infer", "--images", "i", "--json-path", "j", "--state-dict-path", "s", "--class2idx", "c", "-o", "o"]


def _parse(*mode):
    return build_parser().parse_args(["--run-id", "x", *mode])


def test_parser_flags():
    assert _parse("train", "-o", "out").normalize is None
    assert _parse(*TEST_MODE).normalize is None and _parse(*INFER_MODE).normalize is None
    assert _parse("train", "-o", "out", "--normalize", "channel-normal").normalize == "channel-normal"
    assert _parse("train", "-o", "out", "--normalize", "dataset").normalize == "dataset"
    given = _parse("train", "-o", "out", "--normalize", "user-normal:0.5:0.25").normalize
    assert transforms.parse(given) == transforms.Spec("user-normal", (0.5,), (0.25,))
    for mode in (TEST_MODE, INFER_MODE):
        assert _parse(*mode, "--normalize", "none").normalize == "none"
        assert _parse(*mode, "--normalize", "minmax").normalize == "minmax"
        with pytest.raises(SystemExit):
            _parse(*mode, "--normalize", "dataset")  # (nothing to resolve it against)
    for bad in ("none", "norm", "user-normal:1:0", ""):
        with pytest.raises(SystemExit):
            _parse("train", "-o", "out", "--normalize", bad)


def test_the_flag_reaches_the_configs(tmp_path, monkeypatch):
    from marlclassification_amd import __main__ as cli
    from marlclassification_amd import eval as eval_mod
    from marlclassification_amd import infer as infer_mod
    from marlclassification_amd import train as train_mod

    seen = {}
    monkeypatch.setattr(train_mod, "train_main", lambda m, mc, tc, **kw: seen.update(model=mc))
    monkeypatch.setattr(eval_mod, "eval_main", lambda m, ec: seen.update(eval=ec))
    monkeypatch.setattr(infer_mod, "infer_main", lambda m, ic: seen.update(infer=ic))
    cli.main(["--run-id", "x", "train", "-o", str(tmp_path), "--normalize", "channel-minmax"])
    cli.main(["--run-id", "x", *TEST_MODE, "--normalize", "none"])
    cli.main(["--run-id", "x", *INFER_MODE[:-1], str(tmp_path / "frames"), "--normalize", "normal"])
    assert seen["model"].normalize == "channel-minmax"
    assert seen["eval"].normalize == "none" and seen["infer"].normalize == "normal"
    cli.main(["--run-id", "x", "train", "-o", str(tmp_path)])
    cli.main(["--run-id", "x", *TEST_MODE])
    assert seen["model"].normalize is None and seen["eval"].normalize is None
    assert EvalConfig(img_size=28, state_dict_path="s", batch_size=2, json_path="j", dataset_path="d",
                      output_dir="o").normalize is None
    assert InferConfig(state_dict_path="s", json_path="j", images_path=["i"], output_dir="o",
                       class_to_idx="c").normalize is None


def test_the_entries_are_bound_beside_the_versioned_abi():
    from marlclassification_amd import _lib

    assert _lib.NORMALIZE_ENTRIES == ("marl_batch_stats", "marl_batch_stats_scratch_bytes", "marl_batch_normalize",
                                      "marl_batch_normalize_plan")
    assert all(name in _lib._HOOKS for name in _lib.NORMALIZE_ENTRIES)
    assert not any(name in _lib.EXPORTS for name in _lib.NORMALIZE_ENTRIES)
    assert _lib.MARL_ABI_VERSION == 5 and len(_lib.EXPORTS) == 57
    assert transforms.MODES == {"normal": 0, "channel-normal": 1, "minmax": 2, "channel-minmax": 3, "user-normal": 4,
                                "user-minmax": 5}


def test_the_plan_and_the_guards_are_host_arithmetic():
    """No GPU: the plan query and every refusal of the two launchers answer before anything is enqueued (made-up
    pointers, never dereferenced)."""
    import ctypes as C

    from marlclassification_amd import _lib

    lib = _lib.load()
    info = transforms.NormalizePlan()
    SRC, DST, REC = 0x10000000, 0x20000000, 0x30000000
    assert lib.marl_batch_normalize_plan(3, 256, 256, 1, SRC, DST, C.byref(info)) == 0
    p = info.as_dict()
    assert p["load_bytes"] == 16 and p["store_bytes"] == 16 and p["chunk_elems"] > 0
    assert p["partials_per_plane"] == -(-256 * 256 // p["chunk_elems"])
    assert p["apply_blocks_per_plane"] == -(-256 * 256 // p["apply_chunk_elems"])
    assert lib.marl_batch_stats_scratch_bytes(5, 3, 256, 256, 1) == 5 * 3 * p["partials_per_plane"] * 32
    assert lib.marl_batch_normalize_plan(3, 256, 256, 4, SRC, DST, C.byref(info)) == 0
    assert info.chunk_elems * 4 == p["chunk_elems"]  # (a chunk is a byte count)
    for (h, w, off), store in (((33, 31, 0), 4), ((8, 8, 8), 8), ((8, 8, 4), 4), ((5, 6, 0), 8), ((1, 1, 0), 4)):
        assert lib.marl_batch_normalize_plan(3, h, w, 1, SRC, DST + off, C.byref(info)) == 0
        assert info.store_bytes == store, (h, w, off)
    assert lib.marl_batch_normalize_plan(3, 8, 8, 1, SRC, DST, None) == -1
    assert lib.marl_batch_normalize_plan(3, 8, 8, 2, SRC, DST, C.byref(info)) == -1
    assert lib.marl_batch_normalize_plan(0, 8, 8, 1, SRC, DST, C.byref(info)) == -1
    assert lib.marl_batch_stats_scratch_bytes(0, 3, 8, 8, 1) == 0 and lib.marl_batch_stats_scratch_bytes(1, 3, 8, 8, 3) == 0
    user = (C.c_double * 6)(0.5, 0.25, 0.5, 0.25, 0.5, 0.25)

    def norm(src=SRC, n_src=4, rows=None, rec=REC, mode=1, usr=None, batch=4, c=3, h=8, w=8, elt=1, dst=DST, coef=None):
        rc = lib.marl_batch_normalize(src, n_src, rows, rec, mode, usr, batch, c, h, w, elt, dst, coef, None)
        return rc, lib.marl_last_error().decode()

    def stat(src=SRC, n_src=4, rows=None, batch=4, c=3, h=8, w=8, elt=1, scratch=DST, rec=REC):
        rc = lib.marl_batch_stats(src, n_src, rows, batch, c, h, w, elt, scratch, rec, None)
        return rc, lib.marl_last_error().decode()

    zero_s = (C.c_double * 6)(0.5, 0.25, 0.5, 0.0, 0.5, 0.25)
    same = (C.c_double * 6)(0.5, 0.9, 0.3, 0.3, 0.5, 0.9)
    many = (C.c_double * 34)(*([0.5, 0.25] * 17))
    for kw, word in ((dict(src=None), "null"), (dict(dst=None), "null"), (dict(rec=None), "records"),
                     (dict(mode=4, usr=None), "user"), (dict(mode=6), "mode"), (dict(mode=-1), "mode"),
                     (dict(elt=2), "elt_bytes"), (dict(batch=0), "positive"), (dict(n_src=0), "positive"),
                     (dict(c=0), "positive"), (dict(h=-1), "positive"), (dict(w=0), "positive"),
                     (dict(n_src=3), "n_src"), (dict(mode=4, usr=many, c=17), "16"),
                     (dict(mode=4, usr=zero_s), "s must"), (dict(mode=5, usr=same), "hi - lo"),
                     (dict(dst=SRC), "overlaps"), (dict(dst=SRC + 4 * 3 * 64 - 4), "overlaps"),
                     (dict(src=SRC + 2, elt=4), "aligned"), (dict(dst=DST + 2), "aligned"),
                     (dict(rec=REC + 4), "records"), (dict(coef=REC + 2), "coef")):
        rc, msg = norm(**kw)
        assert rc == -1 and msg.startswith("marl_batch_normalize:") and word in msg, (kw, rc, msg)
    for kw, word in ((dict(c=2, h=32768, w=32768), "2^31"), (dict(c=3, h=2048, w=2048), "2^23"),
                     (dict(mode=4, usr=user, c=3, h=16384, w=16384), "2^31")):
        rc, msg = norm(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)
    for kw, word in ((dict(src=None), "null"), (dict(scratch=None), "null"), (dict(rec=None), "null"),
                     (dict(elt=3), "elt_bytes"), (dict(batch=-1), "positive"), (dict(n_src=0), "positive"),
                     (dict(c=0), "positive"), (dict(h=0), "positive"), (dict(w=-2), "positive"),
                     (dict(n_src=2), "n_src"), (dict(src=SRC + 1, elt=4), "aligned"),
                     (dict(scratch=DST + 4), "8-byte"), (dict(rec=REC + 1), "8-byte")):
        rc, msg = stat(**kw)
        assert rc == -1 and msg.startswith("marl_batch_stats:") and word in msg, (kw, rc, msg)
    for kw, word in ((dict(c=2, h=32768, w=32768), "2^31"), (dict(c=3, h=2048, w=2048), "2^23"),
                     (dict(batch=2 ** 31 - 1, n_src=2 ** 31, c=1, h=128, w=256, rows=REC), "workgroups")):
        rc, msg = stat(**kw)
        assert rc == -2 and word in msg, (kw, rc, msg)
