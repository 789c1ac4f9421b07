"""Host side of the loss options (no GPU): the definition in torch (``marlclassification_amd/class_loss.py``) against
``F.cross_entropy(weight=, label_smoothing=)`` and the closed-form gradient the kernel implements, balanced weights, the
step schedules, the guards of ``ClassLoss`` / ``Trainer`` / the library, the entry point's place beside the versioned
ABI and the command line."""
import math
import os
import re

import pytest
import torch as th
import torch.nn.functional as F

from marlclassification_amd import _lib
from marlclassification_amd import class_loss as cl
from marlclassification_amd.__main__ import build_parser

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS, NA, NB, NC = 3, 2, 5, 7


def _inputs(seed=3, scale=4.0):
    g = th.Generator().manual_seed(seed)
    preds = scale * th.randn(NS, NA, NB, NC, generator=g, dtype=th.float64)
    y = th.randint(NC, (NB,), generator=g)
    w = th.rand(NC, generator=g, dtype=th.float64) + 0.25
    w[1] = 0.0  # (a class nobody is asked to get right)
    y[0] = 1
    s = th.tensor([0.0, 0.5, 2.0], dtype=th.float64)
    return preds, y, w, s


def _torch_ce(preds, y, w, eps):
    z = preds.mean(dim=1)
    return th.stack([F.cross_entropy(z[t], y, weight=w, label_smoothing=eps, reduction="none") for t in range(NS)])


# ---- the definition -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_w,eps", [(True, 0.0), (False, 0.1), (True, 0.1), (True, 0.9), (False, 0.0)])
def test_vote_error_is_torchs_cross_entropy_times_the_step_weight(use_w, eps):
    preds, y, w, s = _inputs()
    w = w if use_w else None
    ref = _torch_ce(preds, y, w, eps)
    got = cl.vote_error(preds, y, w, eps)
    assert got.shape == (NS, NB) and got.dtype == th.float64
    assert (got - ref).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item())
    got = cl.vote_error(preds, y, w, eps, s)
    assert (got - ref * s.view(NS, 1)).abs().max().item() <= 1e-13 * max(1.0, ref.abs().max().item())
    assert bool((got[0] == 0).all())


def closed_form_g_preds(preds, y, w, eps, s):
    """g_preds[t,a,b,c] = s_t / R * (softmax(z)_c * sum_c' q_c' - q_c) for the loss sum_t mean_b err."""
    ns, na, nb, nc = preds.shape
    z = preds.mean(dim=1)
    onehot = F.one_hot(y, nc).to(preds.dtype)  # [Nb, nC]
    q = (1.0 - eps) * w[y].unsqueeze(-1) * onehot + (eps / nc) * w.unsqueeze(0)  # [Nb, nC]
    g = s.view(ns, 1, 1) / (na * nb) * (th.softmax(z, -1) * q.sum(-1, keepdim=True) - q)
    return g.unsqueeze(1).expand(ns, na, nb, nc)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_autograd_through_vote_error_is_the_closed_form(eps):
    preds, y, w, s = _inputs()
    leaf = preds.clone().requires_grad_()
    cl.vote_error(leaf, y, w, eps, s).sum(0).mean().backward()
    ref = closed_form_g_preds(preds, y, w, eps, s)
    assert (leaf.grad - ref).abs().max().item() <= 1e-13 * ref.abs().max().item()
    assert bool((leaf.grad[0] == 0).all()), "a step of weight 0 gets no gradient"


def test_a_logit_gap_of_200_stays_finite():
    preds, y, w, s = _inputs()
    preds = preds.float()
    preds[..., 0] += 200.0
    leaf = preds.clone().requires_grad_()
    err = cl.vote_error(leaf, y, w.float(), 0.1, s.float())
    err.sum().backward()
    assert bool(th.isfinite(err).all()) and bool(th.isfinite(leaf.grad).all())
    assert err.max().item() > 10.0


def test_rewards_are_the_references_times_the_label_weight():
    from oracle import marl_oracle as mo

    preds, y, w, _ = _inputs()
    ref = mo.classification_rewards(preds, y)
    assert (cl.rewards(preds, y) - ref).abs().max().item() <= 1e-13
    assert (cl.rewards(preds, y, w) - ref * w[y]).abs().max().item() <= 1e-13
    assert bool((cl.rewards(preds, y, w)[:, :, 0] == 0).all())


# ---- balanced weights and schedules ---------------------------------------------------------------------------------
def test_balanced_weights():
    w = cl.balanced_weights([0, 0, 0, 1, 3, 3], 4)  # N = 6, nC = 4, counts 3, 1, 0, 2
    assert w.dtype == th.float32
    assert th.allclose(w.double(), th.tensor([0.5, 1.5, 0.0, 0.75], dtype=th.float64))
    assert th.equal(cl.balanced_weights(th.tensor([1, 0, 2]), 3), th.ones(3))
    for bad in ([], [0, 4], [-1, 0]):
        with pytest.raises(ValueError):
            cl.balanced_weights(bad, 4)


def test_step_schedule():
    assert cl.step_schedule("all", 4) == (1.0, 1.0, 1.0, 1.0)
    assert cl.step_schedule("last", 4) == (0.0, 0.0, 0.0, 1.0) == cl.step_schedule("last:1", 4)
    assert cl.step_schedule("last:3", 4) == (0.0, 1.0, 1.0, 1.0)
    assert cl.step_schedule("last:4", 4) == cl.step_schedule("all", 4)
    assert cl.step_schedule("linear", 4) == (0.25, 0.5, 0.75, 1.0)
    assert cl.step_schedule([0, 0.5, 2], 3) == (0.0, 0.5, 2.0)
    for bad in ("last:5", "last:0", "first", "", "last:", "linear:2", [1.0, 2.0], [0.0, 0.0, 0.0, 0.0],
                [1.0, -1.0, 1.0, 1.0], [1.0, math.nan, 1.0, 1.0]):
        with pytest.raises(ValueError):
            cl.step_schedule(bad, 4)


# ---- the setting --------------------------------------------------------------------------------------------------
def test_class_loss_holds_the_fp32_values_and_is_hashable():
    c = cl.ClassLoss(3, 2, [0.1, 0.0, 2.0], 0.1, th.tensor([0.0, 1.0]), True)
    assert c.class_weights == tuple(th.tensor([0.1, 0.0, 2.0]).tolist()) and c.step_weights == (0.0, 1.0)
    assert c.label_smoothing == 0.1 and c.weight_rewards is True and not c.is_default
    assert c == cl.ClassLoss(3, 2, (0.1, 0.0, 2.0), 0.1, [0, 1], 1) and hash(c) == hash(cl.ClassLoss(3, 2, (0.1, 0.0, 2.0), 0.1, [0, 1], 1))
    assert cl.ClassLoss(3, 2).is_default
    assert not cl.ClassLoss(3, 2, [1.0, 1.0, 1.0]).is_default, "neutral values given explicitly are a setting"
    with pytest.raises(Exception):
        c.label_smoothing = 0.2
    assert cl.from_options(3, 2) is None
    assert cl.from_options(3, 2, error_step_weights="last") == cl.ClassLoss(3, 2, step_weights=(0.0, 1.0))


@pytest.mark.parametrize("kw", [
    {"class_weights": [1.0, 1.0]}, {"class_weights": [1.0, 1.0, 1.0, 1.0]}, {"class_weights": [0.0, 0.0, 0.0]},
    {"class_weights": [1.0, -0.5, 1.0]}, {"class_weights": [1.0, math.nan, 1.0]},
    {"class_weights": [1.0, math.inf, 1.0]}, {"class_weights": [[1.0, 1.0, 1.0]]}, {"class_weights": "abc"},
    {"step_weights": [1.0]}, {"step_weights": [0.0, 0.0]}, {"step_weights": [1.0, -1.0]},
    {"step_weights": [math.nan, 1.0]}, {"label_smoothing": 1.0}, {"label_smoothing": -0.1},
    {"label_smoothing": math.nan}, {"label_smoothing": "0.1"}, {"label_smoothing": True}, {"weight_rewards": 2},
    {"nb_class": 0}, {"nb_steps": 1.5}])
def test_class_loss_refuses(kw):
    args = {"nb_class": 3, "nb_steps": 2}
    args.update(kw)
    with pytest.raises(ValueError):
        cl.ClassLoss(**args)


def _model():
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import MnistCnn

    return ModelsWrapper(MnistCnn(6), 8, 8, 4, 4, 4, 2, 4, 10, 8, 8)


def test_trainer_and_fused_take_the_keywords_and_check_them():
    import inspect

    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FusedA2C
    from marlclassification_amd.training.trainer import Trainer

    m = _model()
    keys = list(m.state_dict().keys())
    Trainer(m, 10, 1e-3, 0.9)
    Trainer(m, 10, 1e-3, 0.9, class_weights=[1.0] * 10, label_smoothing=0.1, error_step_weights="last:2",
            weight_rewards=True)
    Trainer(m, 10, 1e-3, 0.9, error_step_weights=[0.0, 1.0, 1.0])
    assert list(m.state_dict().keys()) == keys
    for kw in ({"class_weights": [1.0] * 9}, {"class_weights": [0.0] * 10}, {"class_weights": [-1.0] + [1.0] * 9},
               {"label_smoothing": 1.0}, {"error_step_weights": "first"}):
        with pytest.raises(ValueError):
            Trainer(m, 10, 1e-3, 0.9, **kw)
    for fn in (Trainer.__init__, FusedA2C.__init__):
        p = inspect.signature(fn).parameters
        assert p["class_weights"].default is None and p["label_smoothing"].default == 0.0
        assert p["error_step_weights"].default is None and p["weight_rewards"].default is False
    assert inspect.signature(HipEngine.set_class_loss).parameters["class_loss"].default is None


# ---- the library: a header of its own, the versioned ABI untouched, guards without a device -----------------------
def _declared(header):
    with open(os.path.join(ROOT, "include", header), "r", encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(marl_[a-z0-9_]+)\s*\(", text))


def test_entry_point_lives_beside_the_versioned_abi():
    assert _declared("marl_hip_classloss.h") == {"marl_class_loss"} == set(_lib.CLASSLOSS_ENTRIES)
    assert "marl_class_loss" not in _declared("marl_hip.h")
    assert len(_lib.EXPORTS) == 57 and "marl_class_loss" not in _lib.EXPORTS
    assert _lib.MARL_ABI_VERSION == 5


def test_library_guards_answer_without_a_device():
    import ctypes as C

    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "marl_hip.h"), "r", encoding="utf-8") as f:
        einval = int(re.search(r"#define MARL_EINVAL \((-?\d+)\)", f.read()).group(1))
    fake = C.c_void_p(4096)  # (never read: the setting only keeps the pointer)

    try:
        for eps in (1.0, 1.5, -0.01, math.nan, math.inf):
            assert lib.marl_class_loss(None, 0, eps, None, 0, 0) == einval, eps
            assert b"class_loss" in lib.marl_last_error()
        assert lib.marl_class_loss(fake, 0, 0.0, None, 0, 0) == einval
        assert lib.marl_class_loss(None, 0, 0.0, fake, 0, 0) == einval
        assert lib.marl_class_loss(None, -1, 0.0, None, 0, 0) == einval
        assert lib.marl_class_loss(fake, 10, 0.1, fake, 4, 1) == 0
        assert lib.marl_class_loss(None, 0, 0.999, None, 0, 0) == 0
    finally:
        assert lib.marl_class_loss(None, 0, 0.0, None, 0, 0) == 0


# ---- the command line -------------------------------------------------------------------------------------------
def _parse(*mode):
    return build_parser().parse_args(["--run-id", "x", *mode])


def test_parser_train_flags_and_config():
    from marlclassification_amd.config import TrainConfig

    a = _parse("train", "-o", "out")
    assert a.class_weights is None and a.label_smoothing == 0.0 and a.error_steps is None and a.weight_rewards is False
    a = _parse("train", "-o", "out", "--class-weights", "balanced", "--label-smoothing", "0.1", "--error-steps",
               "last:2", "--weight-rewards")
    assert a.class_weights == "balanced" and a.label_smoothing == 0.1 and a.error_steps == "last:2" and a.weight_rewards
    assert _parse("train", "-o", "out", "--class-weights", "1,0,2.5").class_weights == (1.0, 0.0, 2.5)
    assert _parse("train", "-o", "out", "--class-weights", "w.npy").class_weights == "w.npy"
    for spec in ("all", "last", "linear"):
        assert _parse("train", "-o", "out", "--error-steps", spec).error_steps == spec
    for bad in (["--class-weights", "1,x"], ["--class-weights", "0,0"], ["--class-weights", "1,-1"],
                ["--label-smoothing", "1"], ["--label-smoothing", "-0.1"], ["--label-smoothing", "x"],
                ["--error-steps", "last:0"], ["--error-steps", "first"], ["--weight-rewards", "1"]):
        with pytest.raises(SystemExit):
            _parse("train", "-o", "out", *bad)
    test = ["test", "--dataset-path", "d", "--json-path", "j", "--state-dict-path", "s", "-o", "o"]
    infer = ["infer", "--images", "i", "--json-path", "j", "--state-dict-path", "s", "--class2idx", "c", "-o", "o"]
    for mode in (test, infer):
        for flag in (["--class-weights", "balanced"], ["--label-smoothing", "0.1"], ["--error-steps", "last"],
                     ["--weight-rewards"]):
            with pytest.raises(SystemExit):
                _parse(*mode, *flag)
    t = TrainConfig(img_size=28, nb_epoch=2, learning_rate=1e-3, batch_size=2, resources_dir="r", output_dir="o",
                    gamma=0.9)
    assert t.class_weights is None and t.label_smoothing == 0.0 and t.error_steps is None and not t.weight_rewards
    t = TrainConfig(img_size=28, nb_epoch=2, learning_rate=1e-3, batch_size=2, resources_dir="r", output_dir="o",
                    gamma=0.9, class_weights=(1.0, 2.0), label_smoothing=0.1, error_steps="linear", weight_rewards=True)
    assert t.class_weights == (1.0, 2.0) and t.error_steps == "linear"


def test_resolve_class_weights(tmp_path):
    import numpy as np

    assert cl.resolve_class_weights(None, 3) is None
    assert cl.resolve_class_weights("balanced", 3, [0, 0, 1, 1, 2, 2]) == (1.0, 1.0, 1.0)
    assert cl.resolve_class_weights((1.0, 2.0, 0.0), 3) == (1.0, 2.0, 0.0)
    path = str(tmp_path / "w.npy")
    np.save(path, np.array([0.5, 1.5, 1.0]))
    assert cl.resolve_class_weights(path, 3) == (0.5, 1.5, 1.0)
    for spec, n in (((1.0, 2.0), 3), (path, 4), ("balanced", 3)):
        with pytest.raises(ValueError):
            cl.resolve_class_weights(spec, n)
    # the model's configuration file never learns of a run-time option
    from marlclassification_amd.config import ModelConfig

    assert not any(k in ModelConfig.model_fields for k in ("class_weights", "label_smoothing", "error_steps"))
