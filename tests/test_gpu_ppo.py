"""GPU: PPO on the fused path - GAE(lambda) advantages (marl_advantages), the clipped surrogate and its gradients
(marl_ppo_loss_fwd_bwd), global-norm gradient clipping (marl_grad_clip), and ``Trainer`` / ``FusedA2C`` running K update
epochs per rollout with epochs 1 .. K-1 replaying the stored trajectory.  Cases and NS are those of tests/cases.py, the
tolerances those of tests/parity.py; the reference is the float64 torch of tests/loss_ref.py with no options: the
oracle's rewards / standardise, the plain GAE recursion (held to the oracle's returns by tests/test_ppo_host.py),
``torch.minimum`` / ``clamp`` and ``smooth_l1_loss``.  Achieved errors go through ``parity.Recorder`` (copied into
profiles/ppo_errors.json after the box run)."""
import pytest
import torch as th

from oracle import marl_oracle as mo
from tests import loss_ref as ref64
from tests.cases import (NS, POL_BIAS, TWO_EPOCH, TWO_EPOCH_EPS, Case, _engine_episode, _golden_sampler, _sampler, _y,
                         masked_entropy, two_epoch_reference)
from tests.dp import run_ranks
from tests.loss_ref import assert_clear_of_bounds, ratio_deltas
from tests.parity import FWD_TOL, Recorder
from tests.util import model_spec

pytestmark = pytest.mark.gpu

REC = Recorder("ppo_errors", "ppo")
SCALARS = ("loss", "surrogate", "error", "critic", "entropy", "approx_kl", "clip_frac")


# ---- 1: advantages -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.9, 1.0])
@pytest.mark.parametrize("name", ["g1", "wide"])
def test_advantages_match_float64(device, name, lam):
    k = Case(name)
    gamma = 0.97
    y = _y(k)
    eng, out = _engine_episode(k, device)
    bufs = [t.clone() for t in eng.advantages(out, y.to(device), gamma, lam)]
    advn, ret, _ = ref64.advantages(out.step_preds.double().cpu(), out.step_values.double().cpu(), y, gamma, lam)
    tag = f"{name}/lam{lam}"
    REC.fwd(f"{tag}/advn", bufs[5], advn)
    REC.fwd(f"{tag}/ret", bufs[6], ret)
    if lam == 1.0:
        # the oracle's own form too (its float32 discount factors are inside FWD_TOL) ...
        returns = mo.discounted_returns(mo.classification_rewards(out.step_preds.double().cpu(), y), gamma)
        REC.fwd(f"{tag}/ret_vs_discounted_returns", bufs[6], returns)
        REC.fwd(f"{tag}/advn_vs_a2c", bufs[5], mo.standardize(returns - out.step_values.double().cpu()))
        # ... and with rho = 1 the PPO gradients ARE the A2C gradients, bit for bit
        ppo = eng.ppo_loss(out, y.to(device), out.step_log_probas, bufs[5], bufs[6], 0.2)
        a2c = eng.a2c_loss(out, y.to(device), gamma)
        for j, what in enumerate(("g_preds", "g_logp", "g_values")):
            assert th.equal(ppo[j], a2c[j]), f"{what} differs from a2c_loss's"
        assert ppo[3][6].item() == 0.0 and ppo[3][5].item() == 0.0
    # two phases with the statistics untouched in between = phase 0, bit for bit; and a second run too
    two = eng.new_ppo_bufs(out, True)
    eng.advantages(out, y.to(device), gamma, lam, 1, two)
    eng.advantages(out, y.to(device), gamma, lam, 2, two)
    again = eng.advantages(out, y.to(device), gamma, lam)
    for j in (4, 5, 6):
        assert th.equal(bufs[j], two[j]), "phases 1 + 2 differ from phase 0"
        assert th.equal(bufs[j], again[j]), "two runs differ"


# ---- 2: the loss ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, 0.05])
@pytest.mark.parametrize("eps", [0.1, 0.3])
@pytest.mark.parametrize("name", ["g1", "wide"])
def test_ppo_loss_matches_float64_autograd(device, name, eps, beta):
    k = Case(name)
    y = _y(k)
    eng, out = _engine_episode(k, device)
    adv = eng.advantages(out, y.to(device), 0.97, 0.9)
    advn, ret = adv[5].clone(), adv[6].clone()
    old_logp = out.step_log_probas - ratio_deltas(out.step_log_probas.shape).float().to(device)
    bufs = [t.clone() for t in eng.ppo_loss(out, y.to(device), old_logp, advn, ret, eps, entropy_coef=beta)]
    assert len(bufs) == (8 if beta > 0 else 7) and bufs[3].numel() == 7

    leaves = [t.detach().double().cpu().requires_grad_()
              for t in (out.step_preds, out.step_log_probas, out.step_values, out.step_probs)]
    loss, ref_scalars, rho, clipped = ref64.ppo(*leaves, y, old_logp.double().cpu(), advn.double().cpu(),
                                              ret.double().cpu(), eps, beta)
    # fp32 and float64 must agree on the side of 1 +- eps of every ratio: asserted on the reference alone, and
    # both branches must be exercised, the clipped one with either sign of the advantage
    assert_clear_of_bounds(rho, eps)
    a64 = advn.double().cpu()
    assert bool(clipped.any()) and bool((~clipped).any())
    assert bool((clipped & (a64 > 0)).any()) and bool((clipped & (a64 < 0)).any())
    loss.backward()
    tag = f"{name}/eps{eps}/beta{beta}"
    for j, what in enumerate(SCALARS):
        REC.fwd(f"{tag}/scalar_{what}", bufs[3][j], ref_scalars[j])
    assert bufs[3][6].item() == ref_scalars[6].float().item(), "clip_frac is a count: it must be exact"
    grads = [(bufs[0], "g_preds"), (bufs[1], "g_logp"), (bufs[2], "g_values")] + ([(bufs[7], "g_probs")] if beta else [])
    for (got, what), leaf in zip(grads, leaves):
        REC.grad(f"{tag}/{what}", got, leaf.grad)
    assert bool((bufs[1][clipped.to(device)] == 0).all()), "a clipped entry must get a zero g_logp"
    again = eng.ppo_loss(out, y.to(device), old_logp, advn, ret, eps, entropy_coef=beta)
    for j in (0, 1, 2, 3) + ((7,) if beta else ()):  # (what ppo_loss writes: the gradients and the scalars)
        assert th.equal(bufs[j], again[j]), "two runs differ"


# ---- 2b: where the extra per-block partials live ------------------------------------------------------------------
# (Ns, Na, Nb): one block with an odd error count in front of the 8-byte alignment of the spare floats; exactly one
# full block; a second block with four rows (the partials move to the place of the rewards)
PARTIAL_SIZES = [(3, 1, 1), (1, 2, 128), (1, 2, 130)]


def _synthetic_outputs(k, ns, na, nb, seed):
    from marlclassification_amd.engine import EpisodeTensors

    gen = th.Generator().manual_seed(seed)
    c = k.cfg
    preds = th.randn(ns, na, nb, c.nb_class, generator=gen)
    values = th.randn(ns, na, nb, generator=gen)
    probs = th.randn(ns, na, nb, c.nb_action, generator=gen).softmax(-1)
    act = th.randint(c.nb_action, (ns, na, nb), generator=gen)
    logp = probs.gather(-1, act.unsqueeze(-1)).squeeze(-1).log()
    y = th.randint(c.nb_class, (nb,), generator=gen)
    return EpisodeTensors(preds, logp, values, th.zeros(ns, na, nb, 2, dtype=th.int64), act, probs), y


@pytest.mark.parametrize("size", PARTIAL_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", ["g1", "wide"])
def test_losses_match_float64_at_the_partial_placement_sizes(device, name, size):
    """a2c_loss with the bonus, advantages and ppo_loss on synthetic episode outputs at the sizes where the extra
    per-block partials change place (one block: the spare floats behind the vote error; more: the rewards' place),
    with four actions (float4 rows) and six (scalar rows), against the float64 references above."""
    from marlclassification_amd.engine import EpisodeTensors, HipEngine

    k = Case(name)
    ns, na, nb = size
    gamma, lam, beta = 0.97, 0.9, 0.05
    eng = HipEngine(model_spec(k.cfg), device)
    eng.configure(na, nb, ns, k.img.shape[1:])
    host, y = _synthetic_outputs(k, ns, na, nb, 1000 + ns * na * nb)
    out = EpisodeTensors(*(t.to(device) for t in (host.step_preds, host.step_log_probas, host.step_values,
                                                  host.step_pos, host.step_actions, host.step_probs)))
    yd = y.to(device)
    tag = f"partials/{name}/{ns}x{na}x{nb}"

    def leaves():
        return [t.double().requires_grad_() for t in (host.step_preds, host.step_log_probas, host.step_values,
                                                      host.step_probs)]

    # the A2C entry with the bonus: its entropy partial is the one the unified placement moved
    a2c = [t.clone() for t in eng.a2c_loss(out, yd, gamma, entropy_coef=beta)]
    lv = leaves()
    lo = mo.a2c_loss(lv[0], lv[1], lv[2], y, gamma)
    ent = masked_entropy(lv[3])
    loss = lo.loss - beta * ent.sum(0).mean()
    loss.backward()
    ref_scalars = th.stack([loss, lo.path, lo.error, lo.critic, ent.mean()]).detach()
    for j, what in enumerate(("loss", "path", "error", "critic", "entropy")):
        REC.fwd(f"{tag}/a2c/scalar_{what}", a2c[3][j], ref_scalars[j])
    for got, leaf, what in zip((a2c[0], a2c[1], a2c[2], a2c[5]), lv, ("g_preds", "g_logp", "g_values", "g_probs")):
        REC.grad(f"{tag}/a2c/{what}", got, leaf.grad)
    for a, b in zip(a2c, eng.a2c_loss(out, yd, gamma, entropy_coef=beta)):
        assert th.equal(a, b), "two a2c_loss runs differ"

    adv = [t.clone() for t in eng.advantages(out, yd, gamma, lam)]
    advn64, ret64, _ = ref64.advantages(host.step_preds.double(), host.step_values.double(), y, gamma, lam)
    REC.fwd(f"{tag}/advn", adv[5], advn64)
    REC.fwd(f"{tag}/ret", adv[6], ret64)
    again = eng.advantages(out, yd, gamma, lam)
    for j in (4, 5, 6):
        assert th.equal(adv[j], again[j]), "two advantages runs differ"

    advn, ret = adv[5], adv[6]
    old_logp = out.step_log_probas - ratio_deltas(out.step_log_probas.shape).float().to(device)
    for eps in (0.1, 0.3):
        bufs = [t.clone() for t in eng.ppo_loss(out, yd, old_logp, advn, ret, eps, entropy_coef=beta)]
        lv = leaves()
        loss, ref_scalars, rho, _ = ref64.ppo(*lv, y, old_logp.double().cpu(), advn.double().cpu(), ret.double().cpu(),
                                            eps, beta)
        assert_clear_of_bounds(rho, eps)
        loss.backward()
        for j, what in enumerate(SCALARS):
            REC.fwd(f"{tag}/eps{eps}/scalar_{what}", bufs[3][j], ref_scalars[j])
        assert bufs[3][6].item() == ref_scalars[6].float().item(), "clip_frac is a count: it must be exact"
        for got, leaf, what in zip((bufs[0], bufs[1], bufs[2], bufs[7]), lv, ("g_preds", "g_logp", "g_values",
                                                                               "g_probs")):
            REC.grad(f"{tag}/eps{eps}/{what}", got, leaf.grad)
        again = eng.ppo_loss(out, yd, old_logp, advn, ret, eps, entropy_coef=beta)
        for j in (0, 1, 2, 3, 7):
            assert th.equal(bufs[j], again[j]), "two ppo_loss runs differ"


# ---- 3: exactly zero probabilities ----------------------------------------------------------------------------------
def test_zero_probabilities_give_finite_scalars_and_gradients(device):
    k = Case("g1")
    k.params = dict(k.params)
    k.params[POL_BIAS] = th.tensor([200.0, 0.0, 0.0, 0.0])
    model = k.model(device)
    eng, out = _engine_episode(k, device)
    one_hot = th.tensor([1.0, 0.0, 0.0, 0.0], device=device).expand_as(out.step_probs)
    assert th.equal(out.step_probs, one_hot), "precondition: the distributions are exactly [1, 0, 0, 0]"
    y = _y(k).to(device)
    adv = eng.advantages(out, y, 0.99, 0.9)
    bufs = eng.ppo_loss(out, y, out.step_log_probas, adv[5], adv[6], 0.2, adv, entropy_coef=0.5)
    sc, gpr = bufs[3], bufs[7]
    assert bool(th.isfinite(sc).all()) and sc[4].item() == 0.0 and sc[5].item() == 0.0 and sc[6].item() == 0.0
    for t in bufs[:3] + (gpr,):
        assert bool(th.isfinite(t).all())
    assert bool((gpr[..., 1:] == 0).all())
    grads = {n: th.empty_like(p) for n, p in model.named_parameters()}
    eng.episode_backward(bufs[0], bufs[1], bufs[2], grads, g_probs=gpr)
    assert all(bool(th.isfinite(v).all()) for v in grads.values())


# ---- 4: gradient clipping -------------------------------------------------------------------------------------------
def test_grad_clip_matches_clip_grad_norm(device):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams

    k = Case("resisc3")
    eng = HipEngine(model_spec(k.cfg), device)
    flat = FlatParams(mo.param_shapes(k.cfg), device)
    gen = th.Generator().manual_seed(123)
    for v in flat.grad_views().values():  # (the padding gaps of the flat buffer stay zero)
        v.copy_(th.randn(v.shape, generator=gen))
    g0 = flat.grads.clone()
    ref = th.nn.Parameter(th.zeros(flat.numel, dtype=th.float64))
    ref.grad = g0.double().cpu()
    max_norm = 3.0
    ref_norm = th.nn.utils.clip_grad_norm_([ref], max_norm).item()
    assert ref_norm > 10 * max_norm
    norm = eng.grad_clip(flat.grads, max_norm).clone()
    rel = abs(norm.item() - ref_norm) / ref_norm
    err = (flat.grads.double().cpu() - ref.grad).abs().max().item()
    entries = err / ref.grad.abs().max().item()
    print(f"[ppo] grad_clip: norm rel err {rel:.3e}, entries {entries:.3e}")
    REC.put("grad_clip", {"norm_rel_err": rel, "max_err_over_max_g": entries, "tol": 1e-6})
    assert rel <= 1e-6
    assert err <= 1e-6 * ref.grad.abs().max().item()
    clipped = flat.grads.clone()
    # two runs give the same bits
    flat.grads.copy_(g0)
    norm2 = eng.grad_clip(flat.grads, max_norm).clone()
    assert th.equal(flat.grads, clipped) and th.equal(norm, norm2)
    # a bound above the norm leaves every bit
    flat.grads.copy_(g0)
    norm3 = eng.grad_clip(flat.grads, 2.0 * ref_norm).clone()
    assert th.equal(flat.grads, g0) and th.equal(norm3, norm)
    # an unaligned view with a length that is no multiple of four: the scalar instance
    odd = g0[1:1 + 1001].clone()
    view = th.zeros(1004, device=device)[1:1002]
    view.copy_(odd)
    n_odd = eng.grad_clip(view, 0.5).item()
    ref_odd = odd.double().norm().item()
    assert abs(n_odd - ref_odd) <= 1e-6 * ref_odd
    assert (view.double() - odd.double() * (0.5 / (ref_odd + 1e-6))).abs().max().item() <= 1e-6 * odd.abs().max().item()


# ---- 5: the trainer with the options at / next to their defaults ----------------------------------------------------
def _one_epoch(k, device, y, **kwargs):
    from marlclassification_amd.training import Trainer

    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    trainer = Trainer(model, k.cfg.nb_class, 1e-3, 0.99, **kwargs)
    trainer.train_epoch([(k.img, y)], 0, sampler)
    return trainer, {n: v.clone() for n, v in model.state_dict().items()}


def test_trainer_at_the_defaults_and_through_the_new_entries_is_the_plain_trainer(device):
    k = Case("g1")
    y = _y(k)
    plain_tr, plain = _one_epoch(k, device, y)
    same_tr, same = _one_epoch(k, device, y, ppo_epochs=1)
    assert set(same_tr.metrics()) == set(plain_tr.metrics())
    # rho = 1, lambda = 1 and a bound nothing reaches: the new entries, the same bits
    ppo_tr, ppo = _one_epoch(k, device, y, ppo_epochs=1, ppo_clip=0.2, gae_lambda=1.0, max_grad_norm=1e9)
    m = ppo_tr.metrics()
    assert {"approx_kl", "clip_frac", "grad_norm"} <= set(m) and "entropy" not in m
    assert m["approx_kl"] == 0.0 and m["clip_frac"] == 0.0 and 0.0 < m["grad_norm"] < 1e9
    for n in plain:
        assert th.equal(plain[n], same[n]), n
        assert th.equal(plain[n], ppo[n]), n
    assert any(not th.equal(plain[n], k.params[n].to(device)) for n in plain), "the step must move the weights"


def test_fused_a2c_runs_the_trainers_epochs(device):
    """``FusedA2C.iteration`` and ``Trainer.train_step`` share one epoch loop: same draws, same bits."""
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    y = _y(k)
    kw = dict(ppo_epochs=2, ppo_clip=0.1, gae_lambda=0.9, max_grad_norm=0.5, entropy_coef=0.05)
    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    trainer = Trainer(model, k.cfg.nb_class, 1e-3, 0.99, **kw)
    out_t, sc_t = trainer.train_step(k.img, y, sampler)

    eng = HipEngine(model_spec(k.cfg), device)
    eng.configure(k.na, k.nb, NS, k.img.shape[1:])
    flat = FlatParams(mo.param_shapes(k.cfg), device)
    flat.load(k.params)
    fa = FusedA2C(eng, flat, 1e-3, 0.99, **kw)
    out_f, sc_f = fa.iteration(k.img.to(device), y.to(device), sampler.fixed_draws)
    assert flat.step == 2 == model.flat_state().step
    assert th.equal(sc_t, sc_f) and 0.0 < sc_f[6].item() < 1.0, "the second epoch must clip some ratios"
    assert th.equal(out_t.step_log_probas, out_f.step_log_probas)
    assert fa.last_grad_norm.item() > 0.5, "the bound must bite"
    sd = model.state_dict()
    for n, v in flat.param_views().items():
        assert th.equal(v, sd[n]), n


# ---- 6: two epochs against the float64 oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1", "resisc3"])
def test_two_epochs_match_the_float64_oracle(device, name):
    from marlclassification_amd.training import Trainer

    k = Case(name)
    eps, lr = TWO_EPOCH_EPS[name], TWO_EPOCH["lr"]
    y = _y(k)
    ref = two_epoch_reference(k, y, eps)
    frac_ref = ref["clipped"].double().mean().item()
    assert 0.0 < frac_ref < 1.0, "the reference must clip some entries in the second epoch, not all"
    assert_clear_of_bounds(ref["rho"], eps)

    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    trainer = Trainer(model, k.cfg.nb_class, lr, TWO_EPOCH["gamma"], ppo_epochs=2, ppo_clip=eps,
                      gae_lambda=TWO_EPOCH["lam"], entropy_coef=TWO_EPOCH["beta"])
    trainer.train_epoch([(k.img, y)], 0, sampler)
    assert trainer.curr_step == 1 and model.flat_state().step == 2
    m = trainer.metrics()
    print(f"[ppo] {name}: clip_frac {m['clip_frac']:.6f} (ref {frac_ref:.6f}), approx_kl {m['approx_kl']:.3e}")
    assert m["clip_frac"] == th.tensor(frac_ref, dtype=th.float64).float().item()
    REC.fwd(f"{name}/two_epochs/approx_kl", th.tensor(m["approx_kl"]), ref["scalars2"][5])
    for key, j in (("loss", 0), ("entropy", 4)):  # (the last epoch's, recorded only)
        REC.rec(f"{name}/two_epochs/{key}", th.tensor(m[key]), ref["scalars2"][j], FWD_TOL)
    REC.check_update(f"{name}/two_epochs", k, model, ref["after"], [ref["g1"], ref["g2"]], lr)


# ---- 7: a replay leaves the generator alone -------------------------------------------------------------------------
def test_replay_does_not_advance_the_episode_counter(device):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    y = _y(k)
    fourth = []
    for epochs in (3, 1):
        th.manual_seed(4242)
        model = k.model(device)
        sampler = EpisodeSampler(MultiAgent(k.na, model), Environment(k.cfg.actions, k.cfg.window), NS)
        assert sampler.device_rng
        trainer = Trainer(model, k.cfg.nb_class, 0.0, 0.99, ppo_epochs=epochs)  # lr = 0: the weights agree
        pos = [trainer.train_step(k.img, y, sampler)[0].step_pos.clone() for _ in range(3)]
        _, out = sampler.run_episode_raw(k.img, train=False)
        fourth.append((pos, out.step_pos.clone()))
        assert model.flat_state().step == 3 * epochs
    (pos3, last3), (pos1, last1) = fourth
    for a, b in zip(pos3, pos1):
        assert th.equal(a, b)
    assert not th.equal(pos3[0], pos3[1]), "every rollout draws anew"
    assert th.equal(last3, last1), "the replays moved the generator sequence of later rollouts"


# ---- 8: two ranks ---------------------------------------------------------------------------------------------------
def _dp_ppo_worker(rank, world, port, bucketed, out_q):
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from marlclassification_amd.fused import EpisodeDraws
    from marlclassification_amd.parallel import BucketedGradAllReduce, GradAllReduce, broadcast_parameters, shard_bounds
    from marlclassification_amd.training import Trainer
    from tests.util import Golden

    device = th.device("cuda:0")  # both ranks share the one GPU of the test box
    g = Golden("g2_mnist_c1")
    model, sampler = _golden_sampler(g, device)
    flat = model.flat_state()
    broadcast_parameters(flat.params)
    lo, hi = shard_bounds(g.nb, rank, world)
    i = g.inp
    sampler.fixed_draws = EpisodeDraws(*(t.to(device) for t in (
        i.pos0[:, lo:hi].contiguous(), i.h0[:, lo:hi].contiguous(), i.c0[:, lo:hi].contiguous(),
        i.hc0[:, lo:hi].contiguous(), i.cc0[:, lo:hi].contiguous(), i.q[:, :, lo:hi].contiguous())))
    hook = BucketedGradAllReduce(world, None, flat.offsets, flat.numel, device) if bucketed else GradAllReduce(world)
    if bucketed:
        assert hook.split is not None and 0 < hook.split < flat.numel
    trainer = Trainer(model, g.cfg.nb_class, g.lr, g.gamma, allreduce=hook, ppo_epochs=2, ppo_clip=0.01,
                      gae_lambda=0.9, max_grad_norm=0.05)
    norms = []
    for _ in range(2):
        trainer.train_epoch([(g.img[lo:hi], g.y[lo:hi])], 0, sampler)
        norms.append(trainer.metrics()["grad_norm"])
    th.cuda.synchronize()
    if rank == 0:
        out_q.put((model.flat_state().params.cpu().numpy(), model.flat_state().grads.cpu().numpy(), norms,
                   model.flat_state().step))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_ppo_gives_the_same_bits_with_one_and_two_buckets(device):
    import numpy as np

    res = {bucketed: run_ranks(_dp_ppo_worker, 2, bucketed)[0] for bucketed in (False, True)}
    assert res[False][3] == res[True][3] == 4
    assert np.array_equal(res[False][0], res[True][0]), "parameters differ"
    assert np.array_equal(res[False][1], res[True][1]), "clipped gradients differ"
    assert res[False][2] == res[True][2] and all(n > 0.05 for n in res[False][2]), "the bound must bite"
    # (clipped to the bound: the norm of what Adam read is max_grad_norm, up to the 1e-6 of the coefficient)
    assert abs(float(np.sqrt((res[False][1].astype(np.float64) ** 2).sum())) - 0.05) <= 1e-5


# ---- 9: guards ------------------------------------------------------------------------------------------------------
def test_guards(device):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C

    k = Case("g1")
    model = k.model(device)
    eng, out = _engine_episode(k, device)
    y = _y(k).to(device)
    flat = FlatParams(mo.param_shapes(k.cfg), device)
    for kwargs in ({"ppo_epochs": 2}, {"ppo_clip": 0.1}, {"gae_lambda": 0.95}, {"max_grad_norm": 1.0}):
        with pytest.raises(ValueError, match="use_graph"):
            FusedA2C(eng, flat, 1e-3, 0.99, use_graph=True, **kwargs)
        with pytest.raises(ValueError, match="iteration_graph"):
            FusedA2C(eng, flat, 1e-3, 0.99, **kwargs).iteration_graph(k.img.to(device), y, 1, 0)
    FusedA2C(eng, flat, 1e-3, 0.99, use_graph=True, ppo_epochs=1, ppo_clip=0.2, gae_lambda=1.0, max_grad_norm=None)

    sampler = _sampler(k, model, device)
    from marlclassification_amd.core import Trajectory

    _, first = sampler.run_episode_raw(k.img, train=True)
    traj = Trajectory(sampler.fixed_draws, first.step_actions)
    _, again = sampler.run_episode_raw(k.img, train=True, draws=traj.draws, forced=traj.actions)
    for key in ("step_preds", "step_log_probas", "step_values", "step_pos", "step_actions"):
        assert th.equal(getattr(first, key), getattr(again, key)), key
    for bad in (traj.actions[:-1], traj.actions[:, :, :-1], traj.actions[:, :-1]):
        with pytest.raises(ValueError, match="replay"):
            sampler.run_episode_raw(k.img, train=True, draws=traj.draws, forced=bad.contiguous())
    with pytest.raises(ValueError, match="replay"):
        sampler.run_episode_raw(k.img, train=True, forced=traj.actions)

    adv = eng.advantages(out, y, 0.99, 0.9)
    advn, ret = adv[5], adv[6]
    plain = eng.episode_forward(k.img.to(device), *(t.to(device) for t in (k.inp.pos0, k.inp.h0, k.inp.c0, k.inp.hc0,
                                                                           k.inp.cc0, k.inp.q[:NS])), None, True)
    with pytest.raises(ValueError, match="step_probs"):
        eng.ppo_loss(plain, y, plain.step_log_probas, advn, ret, 0.2, entropy_coef=0.1)
    with pytest.raises(ValueError, match="old_logp"):
        eng.ppo_loss(out, y, out.step_log_probas[:-1], advn, ret, 0.2)
    with pytest.raises(ValueError, match="ppo_clip"):
        eng.ppo_loss(out, y, out.step_log_probas, advn, ret, 0.0)
    with pytest.raises(ValueError, match="gae_lambda"):
        eng.advantages(out, y, 0.99, 1.5)
    with pytest.raises(ValueError, match="max_grad_norm"):
        eng.grad_clip(flat.grads, 0.0)

    # a2c_loss and its buffers are untouched by a PPO call sequence on the same engine
    eng.advantages(out, y, 0.99, 0.9, 0, adv)
    eng.ppo_loss(out, y, out.step_log_probas - 0.3, advn, ret, 0.1, adv, entropy_coef=0.2)
    after_ppo = [t.clone() for t in eng.a2c_loss(out, y, 0.99, entropy_coef=0.1)]
    after_ppo_plain = [t.clone() for t in eng.a2c_loss(out, y, 0.99)]
    fresh, out2 = _engine_episode(k, device)
    for a, b in zip(after_ppo, fresh.a2c_loss(out2, y, 0.99, entropy_coef=0.1)):
        assert th.equal(a, b)
    for a, b in zip(after_ppo_plain, fresh.a2c_loss(out2, y, 0.99)):
        assert th.equal(a, b)
