"""CPU: the three entries that carry the fused episode's action distributions are exported by the built library,
declared in the header behind the image-gradient entry (same ABI version, old signatures unchanged) and required
by the loader; ``train`` takes ``--entropy-coef`` (default 0); the reference's four-field construction of
``EpisodeDetailedOutput`` still works; the masked entropy the GPU tests use as their reference is sound."""
import os
import re

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("marl_episode_forward_probs", "marl_episode_backward_probs", "marl_a2c_loss_entropy_fwd_bwd")


def _args(header, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m, f"{name} is not declared"
    return m


def test_library_exports_the_three_entries():
    from marlclassification_amd import _lib

    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTS, name
    assert lib.marl_abi_version() == 5 == _lib.MARL_ABI_VERSION


def test_header_declares_them_after_the_image_gradient_entry():
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    assert re.search(r"#define\s+MARL_ABI_VERSION\s+5\b", header)
    img_end = _args(header, "marl_episode_backward_img").end()
    for name in NEW:
        assert _args(header, name).start() > img_end, name
    fwd = _args(header, "marl_episode_forward_probs").group(1)
    assert "float* step_probs" in fwd and "forced_actions" in fwd and fwd.rstrip().endswith("void* stream")
    bwd = _args(header, "marl_episode_backward_probs").group(1)
    assert "float* d_img" in bwd and "const float* g_probs" in bwd and bwd.rstrip().endswith("void* stream")
    loss = _args(header, "marl_a2c_loss_entropy_fwd_bwd").group(1)
    for piece in ("const float* step_probs", "float entropy_coef", "float* g_probs", "float* scalars_out", "int phase"):
        assert piece in loss, piece
    # the existing entries keep their signatures
    for name in ("marl_episode_forward", "marl_episode_backward", "marl_episode_backward_img",
                 "marl_a2c_loss_fwd_bwd"):
        assert "probs" not in _args(header, name).group(1), name
    assert "entropy" not in _args(header, "marl_a2c_loss_fwd_bwd").group(1)


def test_train_parser_takes_entropy_coef_and_defaults_it_to_zero():
    from marlclassification_amd.__main__ import build_parser
    from marlclassification_amd.config import TrainConfig

    p = build_parser()
    base = "--run-id r train -o out"
    assert p.parse_args(base.split()).entropy_coef == 0.0
    assert p.parse_args((base + " --entropy-coef 0.02").split()).entropy_coef == 0.02
    cfg = TrainConfig(img_size=28, nb_epoch=1, learning_rate=1e-3, batch_size=2, resources_dir="r", output_dir="o",
                      gamma=0.99)
    assert cfg.entropy_coef == 0.0


def test_episode_output_keeps_the_reference_construction():
    from marlclassification_amd.core import EpisodeDetailedOutput, Trajectory  # noqa: F401

    a, b, c, d = (th.zeros(1) for _ in range(4))
    out = EpisodeDetailedOutput(a, b, c, d)
    assert out.step_pos is d and out.step_probs is None and out.step_actions is None


def test_engine_signatures_default_to_the_plain_entries():
    import inspect

    from marlclassification_amd.engine import EpisodeTensors, HipEngine
    from marlclassification_amd.fused import FusedA2C
    from marlclassification_amd.training import Trainer

    assert inspect.signature(HipEngine.episode_forward).parameters["probs"].default is False
    assert inspect.signature(HipEngine.episode_backward).parameters["g_probs"].default is None
    assert inspect.signature(HipEngine.a2c_loss).parameters["entropy_coef"].default == 0.0
    assert inspect.signature(Trainer.__init__).parameters["entropy_coef"].default == 0.0
    assert inspect.signature(FusedA2C.__init__).parameters["entropy_coef"].default == 0.0
    t = th.zeros(1)
    assert EpisodeTensors(t, t, t, t, t).step_probs is None


def test_masked_entropy_reference():
    from tests.loss_ref import masked_entropy

    g = th.Generator().manual_seed(5)
    p = th.softmax(th.randn(64, 6, generator=g, dtype=th.float64), -1)
    assert th.allclose(masked_entropy(p), -(p * p.log()).sum(-1), rtol=1e-14, atol=0)
    # fp32 softmax([200, 0, -1, 3]) is exactly [1, 0, 0, 0]: the naive form is NaN, the masked one 0 with a finite
    # gradient (0 at the zeros, -(log 1 + 1) = -1 at the one)
    logits = th.tensor([200.0, 0.0, -1.0, 3.0])
    q = th.softmax(logits, -1).requires_grad_()
    assert q.tolist() == [1.0, 0.0, 0.0, 0.0]
    assert bool(th.isnan(-(q * q.log()).sum()))
    h = masked_entropy(q)
    h.backward()
    assert h.item() == 0.0 and q.grad.tolist() == [-1.0, 0.0, 0.0, 0.0]
    # float64: tiny but positive, finite gradient through the softmax
    z = logits.double().requires_grad_()
    h64 = masked_entropy(th.softmax(z, -1))
    h64.backward()
    assert 0.0 < h64.item() < 1e-80 and bool(th.isfinite(z.grad).all())
