"""CPU: the three PPO entries (marl_advantages, marl_ppo_loss_fwd_bwd, marl_grad_clip) are exported by the built
library, declared behind marl_a2c_loss_entropy_fwd_bwd (same ABI version, old signatures unchanged) and required by the
loader; ``train`` takes ``--ppo-epochs`` / ``--ppo-clip`` / ``--gae-lambda`` / ``--max-grad-norm``; ``Trainer``,
``FusedA2C`` and ``run_episode_raw`` carry the new keywords with their defaults and guard them; the GAE recursion and
the ratio grid of tests/loss_ref.py, the GPU tests' reference, are sound."""
import inspect
import os
import re

import pytest
import torch as th

from oracle import marl_oracle as mo
from tests.loss_ref import gae, ratio_deltas

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("marl_advantages", "marl_ppo_loss_fwd_bwd", "marl_grad_clip")


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


def test_header_declares_them_after_the_entropy_loss():
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    assert re.search(r"#define\s+MARL_ABI_VERSION\s+5\b", header)
    ent_end = _args(header, "marl_a2c_loss_entropy_fwd_bwd").end()
    for name in NEW:
        assert _args(header, name).start() > ent_end, name
    adv = _args(header, "marl_advantages").group(1)
    for piece in ("float gamma", "float lam", "float* advn", "float* ret", "double* adv_stats", "int phase"):
        assert piece in adv, piece
    ppo = _args(header, "marl_ppo_loss_fwd_bwd").group(1)
    for piece in ("const float* old_logp", "const float* advn", "const float* ret", "float clip_eps",
                  "const float* step_probs", "float entropy_coef", "float* g_probs", "float* scalars_out"):
        assert piece in ppo, piece
    clip = _args(header, "marl_grad_clip").group(1)
    for piece in ("float* grads", "int64_t n", "float max_norm", "float* norm_out"):
        assert piece in clip, piece
    for name in NEW:
        assert _args(header, name).group(1).rstrip().endswith("void* stream"), name
    # the existing loss / episode / optimiser entries keep their signatures
    for name in ("marl_a2c_loss_fwd_bwd", "marl_a2c_loss_entropy_fwd_bwd", "marl_episode_forward",
                 "marl_episode_forward_probs", "marl_episode_backward", "marl_episode_backward_img",
                 "marl_episode_backward_probs", "marl_adam_step"):
        sig = _args(header, name).group(1)
        for word in ("clip", "lam", "old_logp"):
            assert word not in sig, (name, word)


def test_train_parser_and_config_defaults():
    from marlclassification_amd.__main__ import build_parser
    from marlclassification_amd.config import TrainConfig

    p = build_parser()
    base = "--run-id r train -o out"
    a = p.parse_args(base.split())
    assert (a.ppo_epochs, a.ppo_clip, a.gae_lambda, a.max_grad_norm) == (1, 0.2, 1.0, None)
    a = p.parse_args((base + " --ppo-epochs 4 --ppo-clip 0.1 --gae-lambda 0.95 --max-grad-norm 0.5").split())
    assert (a.ppo_epochs, a.ppo_clip, a.gae_lambda, a.max_grad_norm) == (4, 0.1, 0.95, 0.5)
    cfg = TrainConfig(img_size=28, nb_epoch=1, learning_rate=1e-3, batch_size=2, resources_dir="r", output_dir="o",
                      gamma=0.99)
    assert (cfg.ppo_epochs, cfg.ppo_clip, cfg.gae_lambda, cfg.max_grad_norm) == (1, 0.2, 1.0, None)
    cfg = TrainConfig(img_size=28, nb_epoch=1, learning_rate=1e-3, batch_size=2, resources_dir="r", output_dir="o",
                      gamma=0.99, ppo_epochs=3, max_grad_norm=2.0)
    assert cfg.ppo_epochs == 3 and cfg.max_grad_norm == 2.0


def test_keyword_defaults():
    from marlclassification_amd.core import EpisodeSampler
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FusedA2C
    from marlclassification_amd.training import Trainer

    want = {"ppo_epochs": 1, "ppo_clip": 0.2, "gae_lambda": 1.0, "max_grad_norm": None}
    for cls in (Trainer, FusedA2C):
        par = inspect.signature(cls.__init__).parameters
        for k, v in want.items():
            assert par[k].default == v, (cls.__name__, k)
        assert par["entropy_coef"].default == 0.0
    raw = inspect.signature(EpisodeSampler.run_episode_raw).parameters
    assert list(raw)[1:] == ["img_batch", "train", "draws", "probs", "forced"]
    assert raw["forced"].default is None and raw["draws"].default is None and raw["probs"].default is False
    assert list(inspect.signature(HipEngine.advantages).parameters)[1:] == ["out", "y", "gamma", "lam", "phase",
                                                                             "bufs"]
    assert inspect.signature(HipEngine.advantages).parameters["phase"].default == 0
    ppo = inspect.signature(HipEngine.ppo_loss).parameters
    assert list(ppo)[1:] == ["out", "y", "old_logp", "advn", "ret", "clip_eps", "bufs", "entropy_coef"]
    assert ppo["entropy_coef"].default == 0.0 and ppo["bufs"].default is None
    assert list(inspect.signature(HipEngine.grad_clip).parameters)[1:3] == ["grads", "max_norm"]
    assert list(inspect.signature(HipEngine.new_ppo_bufs).parameters)[1:] == ["out", "entropy"]


BAD = ({"ppo_epochs": 0}, {"ppo_epochs": -2}, {"ppo_epochs": 1.5}, {"ppo_clip": 0.0}, {"ppo_clip": -0.1},
       {"gae_lambda": -0.01}, {"gae_lambda": 1.01}, {"max_grad_norm": 0.0}, {"max_grad_norm": -1.0},
       {"ppo_clip": float("nan")}, {"gae_lambda": float("nan")}, {"max_grad_norm": float("nan")})


@pytest.mark.parametrize("kwargs", BAD, ids=[f"{k}={v}" for d in BAD for k, v in d.items()])
def test_constructor_guards(kwargs):
    from marlclassification_amd.fused import FusedA2C
    from marlclassification_amd.training import Trainer

    key = next(iter(kwargs))
    # (the guards come first: neither constructor reaches its model / engine argument)
    with pytest.raises(ValueError, match=key):
        Trainer(None, 10, 1e-3, 0.99, **kwargs)
    with pytest.raises(ValueError, match=key):
        FusedA2C(None, None, 1e-3, 0.99, **kwargs)


def discounted_returns64(rewards, gamma):
    """training/functions.py:35-51 (flip-cumsum-flip) with float64 discount factors.  ``mo.discounted_returns`` keeps
    the reference's float32 ``gamma ** t`` whatever the dtype of the rewards, so on float64 rewards it carries the
    rounding of those factors (~1e-7 relative): the 1e-12 identity below is checked against this form, and this form
    against the oracle's within that rounding.  (rtol 1e-12 against ``mo.discounted_returns`` itself, as first
    planned for this check, cannot be met by ANY exact GAE: the oracle as written rounds gamma ** t to float32.)"""
    shape = [rewards.size(0)] + [1] * (rewards.dim() - 1)
    disc = gamma ** th.arange(rewards.size(0), dtype=th.float64).view(*shape)
    return (rewards * disc).flip(dims=(0,)).cumsum(0).flip(dims=(0,)) / disc


def test_gae_reference_at_both_ends_of_lambda():
    g = th.Generator().manual_seed(5)
    rew = th.rand(7, 3, 4, generator=g, dtype=th.float64) * 2 - 1
    val = th.randn(7, 3, 4, generator=g, dtype=th.float64)
    gamma = 0.93
    adv1, ret1 = gae(rew, val, gamma, 1.0)
    returns = discounted_returns64(rew, gamma)
    assert th.allclose(returns, mo.discounted_returns(rew, gamma).double(), rtol=1e-6, atol=1e-6)
    assert th.allclose(adv1, returns - val, rtol=1e-12, atol=1e-12)
    assert th.allclose(ret1, returns, rtol=1e-12, atol=1e-12)
    adv0, _ = gae(rew, val, gamma, 0.0)
    nxt = th.cat([val[1:], th.zeros_like(val[:1])])
    assert th.allclose(adv0, rew + gamma * nxt - val, rtol=1e-12, atol=0)


@pytest.mark.parametrize("n", [3 * 5 * 19, 3 * 2 * 5, 3, 256, 260])
@pytest.mark.parametrize("eps", [0.1, 0.3])
def test_ratio_grid_stays_clear_of_the_clip_bounds(n, eps):
    """The grids of the two GPU cases (g1: Ns * Na * Nb = 285, wide: 30) and of the partial-placement sizes (3, 256,
    260; 257, 258 and 513 come within 1e-4 of a bound and are not used), in float64 and after the fp32 subtraction
    the test performs on the device: no ratio within 1e-4 of 1 +- eps, and ratios on all three sides."""
    delta = ratio_deltas((n,))
    assert delta.min().item() == -0.5 and delta.max().item() == 0.5 and delta.unique().numel() == n
    for d in (delta, delta.float().double()):
        rho = d.exp()
        for bound in (1 - eps, 1 + eps):
            assert (rho - bound).abs().min().item() >= 1e-4
        assert bool((rho > 1 + eps).any()) and bool((rho < 1 - eps).any())
        assert bool(((rho > 1 - eps) & (rho < 1 + eps)).any())
