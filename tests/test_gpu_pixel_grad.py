"""GPU: gradient with respect to the image through the fused episode (marl_episode_backward_img).  The reference's
crop is a masked_select of the image batch (core/environment.py:95-126), so ``img.requires_grad_()`` ->
``run_episode`` -> ``loss.backward()`` fills ``img.grad`` there; here the image is a differentiable input of the
episode's autograd node.  Checked against float64 autograd through the oracle (cases, seeds and NS of
tests/cases.py, the gradient tolerance of tests/parity.py), on overlapping windows, for its support, with a
frozen model, for bit-reproducibility, at the benchmark shape (full batch against two half batches) and through
``visualization.saliency_maps``.  Achieved errors per case go through ``parity.Recorder`` (copied into
profiles/pixel_grad_errors.json after the box run)."""
import pytest
import torch as th

from oracle import marl_oracle as mo
from tests.cases import CASES, NS, Case, _a2c_like_loss, _loss_terms
from tests.parity import GRAD_TOL, Recorder
from tests.parity import close as _close
from tests.parity import param_grads_match as _param_grads_match
from tests.util import uniform_params

pytestmark = pytest.mark.gpu

REC = Recorder("pixel_grad_errors", "pixel grad")


def _record_margin(tag, got, ref):
    """(this record keeps the bound itself and the margin to it)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    bound = GRAD_TOL * scale + 1e-7
    print(f"[pixel grad] {tag}: max err {err:.3e}, ref max {scale:.3e}, bound {bound:.3e}")
    REC.put(tag, {"max_err": err, "ref_max": scale, "bound": bound, "margin": bound / err if err > 0 else None})


class _Custom(Case):
    """A case of its own: (config, Na, Nb, image [C, H, W], seed), built like the named ones."""

    def __init__(self, spec):
        self.cfg, self.na, self.nb, shape, seed = spec
        self.params = uniform_params(self.cfg, seed)
        self.img = th.rand(self.nb, *shape, generator=th.Generator().manual_seed(seed))
        self.inp = mo.draw_episode_inputs(self.cfg, self.na, self.nb, NS, list(shape[1:]), seed)
        self.gen = th.Generator().manual_seed(seed + 1000)
        self.sizes = list(self.img.shape[2:])


def _sampler(k, model, device):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.fused import EpisodeDraws

    i = k.inp
    sampler = EpisodeSampler(MultiAgent(k.na, model), Environment(k.cfg.actions, k.cfg.window), NS)
    sampler.fixed_draws = EpisodeDraws(*(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0, i.q[:NS])))
    return sampler


def _oracle_loop(k, p64, img64):
    """tests/test_gpu_step_autograd.py::_oracle_act_loop with the crops taken from ``img64`` (float64, may require
    grad); also returns the positions after every move."""
    c, i = k.cfg, k.inp
    table = th.tensor(c.actions)
    pos = i.pos0
    h, cst, hc, cc = (t.double() for t in (i.h0, i.c0, i.hc0, i.cc0))
    msg = th.zeros(k.na, k.nb, c.n_m, dtype=th.float64)
    acc = {"preds": [], "logp": [], "values": [], "pos": []}
    for t in range(NS):
        so = mo.step_forward(p64, c, mo.crop_patches(img64, pos, c.window), msg,
                             mo.normalized_positions(pos, k.sizes).double(), h, cst, hc, cc)
        h, cst, hc, cc, msg = so.h, so.c, so.hc, so.cc, so.msg
        a = mo.sample_actions(so.probs, i.q[t].double())
        logp = th.gather(so.probs, -1, a.unsqueeze(-1)).squeeze(-1).log()
        pos = mo.transition(pos, a, table, c.window, k.sizes)
        for key, v in zip(acc, (so.preds, logp, so.values, pos)):
            acc[key].append(v)
    return {key: th.stack(v) for key, v in acc.items()}


def _check_against_oracle(k, device, tag, frozen=False):
    """One episode + backward with the image requiring grad, on the GPU and in float64; returns
    (d_img, float64 d_img, positions after every move)."""
    model = k.model(device)
    if frozen:
        model.requires_grad_(False)
    terms = _loss_terms(k)
    img = k.img.to(device).requires_grad_()
    ep = _sampler(k, model, device).run_episode(img)
    assert ep.step_preds.grad_fn is not None and ep.step_log_probas.grad_fn is not None
    _a2c_like_loss(ep.step_preds, ep.step_log_probas, ep.step_values, terms).backward()
    assert img.grad is not None, "no gradient reached the image"

    p64 = {n: v.double() for n, v in k.params.items()} if frozen else k.params64()
    img64 = k.img.double().requires_grad_()
    tr = _oracle_loop(k, p64, img64)
    assert th.equal(ep.step_pos.cpu(), tr["pos"]), "the episode moved otherwise than the oracle"
    _a2c_like_loss(tr["preds"], tr["logp"], tr["values"], terms).backward()
    _record_margin(tag, img.grad, img64.grad)
    _close(img.grad, img64.grad, GRAD_TOL, "d_img")
    if frozen:
        assert all(p.grad is None for p in model.parameters())
    else:
        _param_grads_match(model, p64)
    return img.grad.detach().cpu(), img64.grad, tr["pos"]


def _visited(k, step_pos):
    """[Nb, H, W] bool: union of the windows cropped at pos0 and after the moves 0 .. NS - 2."""
    f = k.cfg.window
    mask = th.zeros(k.nb, *k.sizes, dtype=th.bool)
    for pos in [k.inp.pos0] + [step_pos[t] for t in range(NS - 1)]:
        for a in range(k.na):
            for b in range(k.nb):
                r0, c0 = int(pos[a, b, 0]), int(pos[a, b, 1])
                mask[b, r0:r0 + f, c0:c0 + f] = True
    return mask


# ---- 1: float64 oracle parity --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_image_gradient_matches_float64_oracle(device, name):
    _check_against_oracle(Case(name), device, name)


# ---- 2: windows that collide from step 0 ----------------------------------------------------------------------
def test_overlapping_windows(device):
    k = _Custom((mo.OracleConfig("resisc45", 12, 32, 32, 8, 12, 8, 10, 48, 48), 3, 4, (3, 40, 40), 22))
    p = k.inp.pos0
    p[0, :, 1].clamp_(max=40 - 12 - 2)  # room for the shifted agent inside [0, W - f)
    p[1] = p[0]                         # exact overlap
    p[2] = p[0]
    p[2, :, 1] += 1                     # partial overlap, one pixel to the right
    _check_against_oracle(k, device, "collisions")


# ---- 3: support -----------------------------------------------------------------------------------------------
def test_support_is_the_union_of_the_cropped_windows(device):
    k = _Custom((mo.OracleConfig("mnist", 12, 23, 22, 21, 20, 19, 10, 24, 25), 2, 3, (3, 28, 28), 23))
    got, ref, step_pos = _check_against_oracle(k, device, "mnist_3ch")
    mask = _visited(k, step_pos)
    for what, g in (("float64 oracle", ref), ("d_img", got)):
        assert bool((g[:, 1:] == 0).all()), f"{what}: MnistCnn reads channel 0 only"
        assert bool((g[:, 0][~mask] == 0).all()), f"{what}: gradient outside the visited windows"
        assert bool((g[:, 0][mask] != 0).any()), what


# ---- 4: frozen model ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1", "resisc3"])
def test_frozen_model(device, name):
    _check_against_oracle(Case(name), device, name + "_frozen", frozen=True)


# ---- 5: the forward does not move ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1", "resisc3"])
def test_forward_is_unchanged_by_an_image_that_requires_grad(device, name):
    k = Case(name)
    model = k.model(device)
    sampler = _sampler(k, model, device)
    ref = sampler.run_episode(k.img.to(device))
    got = sampler.run_episode(k.img.to(device).requires_grad_())
    with th.no_grad():
        plain = sampler.run_episode(k.img.to(device))
    for key in ("step_preds", "step_log_probas", "step_values", "step_pos"):
        assert th.equal(getattr(got, key).detach(), getattr(ref, key).detach()), key
        assert th.equal(getattr(got, key).detach(), getattr(plain, key)), key


# ---- 6: reproducible --------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(device):
    k = Case("resisc3")
    model = k.model(device)
    sampler = _sampler(k, model, device)
    terms = _loss_terms(k)
    grads = []
    for _ in range(2):
        img = k.img.to(device).requires_grad_()
        ep = sampler.run_episode(img)
        _a2c_like_loss(ep.step_preds, ep.step_log_probas, ep.step_values, terms).backward()
        grads.append(img.grad.clone())
    assert th.equal(grads[0], grads[1])


# ---- 7: the benchmark shape: whole batch against two half batches ----------------------------------------------
def test_full_batch_equals_two_half_batches_at_the_bench_shape(device):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.fused import EpisodeDraws
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import Resisc45Cnn

    c = mo.OracleConfig("resisc45", 12, 256, 256, 64, 96, 16, 45, 384, 384)
    na, ns, nb, hw = 16, 16, 64, 256
    model = ModelsWrapper(Resisc45Cnn(c.window), c.n_b, c.n_a, c.n_m, c.n_m_o, c.n_d, 2, c.nb_action, c.nb_class,
                          c.nlb, c.nla)
    model.load_state_dict(uniform_params(c, 31))
    model.to(device)
    gen = th.Generator().manual_seed(32)
    img = th.rand(nb, 3, hw, hw, generator=gen)  # distinct images
    i = mo.draw_episode_inputs(c, na, nb, ns, [hw, hw], 33)
    terms = (th.randn(ns, na, nb, generator=gen), th.randint(c.nb_class, (ns, na, nb), generator=gen),
             th.randn(ns, na, nb, generator=gen))
    sampler = EpisodeSampler(MultiAgent(na, model), Environment(c.actions, c.window), ns)

    def run(sl):
        sampler.fixed_draws = EpisodeDraws(*(t[:, sl].contiguous().to(device) for t in (i.pos0, i.h0, i.c0, i.hc0,
                                                                                         i.cc0)),
                                           i.q[:, :, sl].contiguous().to(device))
        x = img[sl].to(device).requires_grad_()
        ep = sampler.run_episode(x)
        # sums over everything: a per-image sum, no batch-wide statistic
        _a2c_like_loss(ep.step_preds, ep.step_log_probas, ep.step_values, tuple(t[:, :, sl] for t in terms)).backward()
        model.zero_grad(set_to_none=True)
        return x.grad.cpu(), ep.step_pos.cpu()

    full, pos_full = run(slice(0, nb))
    lo, pos_lo = run(slice(0, nb // 2))
    hi, pos_hi = run(slice(nb // 2, nb))
    assert th.equal(pos_full, th.cat([pos_lo, pos_hi], dim=2)), "the half batches moved otherwise than the full batch"
    halves = th.cat([lo, hi], dim=0)
    _record_margin("bench_shape_b64_full_vs_halves", full, halves)
    _close(full, halves, GRAD_TOL, "d_img, full batch against two half batches")
    assert bool((full != 0).any(dim=3).any(dim=2).all()), "an image / channel without any gradient"


# ---- 8: the helper ---------------------------------------------------------------------------------------------
def test_saliency_maps(device):
    from marlclassification_amd.visualization import saliency_maps

    k = Case("resisc3")
    model = k.model(device)
    sampler = _sampler(k, model, device)
    sal = saliency_maps(sampler, k.img)
    assert sal.shape == (k.nb, *k.sizes) and sal.dtype == th.float32
    assert bool(th.isfinite(sal).all()) and bool((sal >= 0).all())
    with th.no_grad():
        step_pos = sampler.run_episode(k.img.to(device)).step_pos.cpu()
    mask = _visited(k, step_pos)
    sal = sal.cpu()
    assert bool((sal[~mask] == 0).all())
    assert bool((sal.flatten(1) != 0).any(dim=1).all()), "an image without any attribution"
    assert all(p.grad is None for p in model.parameters()), "saliency_maps touched the parameter gradients"
    # an explicit class: same support, another map
    other = saliency_maps(sampler, k.img, class_idx=3).cpu()
    assert other.shape == sal.shape and bool((other[~mask] == 0).all())
