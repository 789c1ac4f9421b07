"""GPU: the action distributions of the fused episode - ``EpisodeSampler.return_probs`` / ``step_probs``
(marl_episode_forward_probs), gradients through them (marl_episode_backward_probs), the entropy bonus of the fused
loss (marl_a2c_loss_entropy_fwd_bwd) in ``Trainer`` / ``FusedA2C``, and trajectory replay.  Cases, seeds and NS are
those of tests/cases.py, the tolerances those of tests/parity.py; the reference is float64 autograd through the oracle
(``cases._oracle_loop``).  Achieved errors go through ``parity.Recorder`` (copied into profiles/policy_dist_errors.json
after the box run)."""
import math

import pytest
import torch as th

from oracle import marl_oracle as mo
from tests.cases import (CASES, NS, POL_BIAS, Case, _a2c_like_loss, _dist_loss, _engine_episode, _loss_terms,
                         _oracle_loop, _sampler, masked_entropy)
from tests.parity import FWD_TOL, GRAD_TOL, Recorder
from tests.parity import close as _close
from tests.util import model_spec

pytestmark = pytest.mark.gpu

REC = Recorder("policy_dist_errors", "policy dist")


# ---- 1: forward -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_step_probs_match_float64_oracle(device, name):
    k = Case(name)
    model = k.model(device)
    sampler = _sampler(k, model, device)
    img = k.img.to(device)
    tr = _oracle_loop(k, {n: v.double() for n, v in k.params.items()}, k.img.double())
    R = k.na * k.nb
    with th.no_grad():
        plain = sampler.run_episode(img)
        eng = model.hip_engine(k.cfg.actions)
        rollout_ws = th.stack([eng.debug_buffer("PROBS", t, train=False).clone() for t in range(NS)])
    ep = sampler.run_episode(img)
    assert ep.step_probs.grad_fn is not None and plain.step_probs.grad_fn is None
    assert not ep.step_actions.requires_grad and ep.step_actions.dtype == th.int64
    for tag, o in (("grad", ep), ("no_grad", plain)):
        assert o.step_probs.shape == (NS, k.na, k.nb, k.cfg.nb_action)
        assert th.equal(o.step_pos.cpu(), tr["pos"]), "the episode moved otherwise than the oracle"
        assert th.equal(o.step_actions.cpu(), tr["act"])
        REC.fwd(f"{name}/{tag}/step_probs", o.step_probs, tr["probs"])
        REC.fwd(f"{name}/{tag}/row_sums", o.step_probs.sum(-1), th.ones(NS, k.na, k.nb))
        REC.fwd(f"{name}/{tag}/exp_logp_vs_gather", o.step_log_probas.exp(),
                o.step_probs.gather(-1, o.step_actions.unsqueeze(-1)).squeeze(-1))
    assert th.equal(plain.step_probs.view(NS, R, -1), rollout_ws), "step_probs is not the rollout layout's PROBS"
    assert th.equal(plain.step_probs, ep.step_probs.detach())
    # the training layout of the engine's own workspace (the fused trainer's path)
    eng, out = sampler.run_episode_raw(img, train=True, probs=True)
    train_ws = th.stack([eng.debug_buffer("PROBS", t, train=True) for t in range(NS)])
    assert th.equal(out.step_probs.view(NS, R, -1), train_ws), "step_probs is not the training layout's PROBS"
    assert th.equal(out.step_probs, ep.step_probs.detach())


# ---- 2: nothing moves when the feature is off --------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_outputs_and_gradients_are_bit_equal_with_return_probs_on_and_off(device, name):
    k = Case(name)
    model = k.model(device)
    terms = _loss_terms(k)
    res = []
    for probs in (False, True):
        sampler = _sampler(k, model, device, probs=probs)
        ep = sampler.run_episode(k.img.to(device))
        assert (ep.step_probs is not None) == probs and ep.step_actions is not None
        _a2c_like_loss(ep.step_preds, ep.step_log_probas, ep.step_values, terms).backward()
        res.append((ep, {n: p.grad.clone() for n, p in model.named_parameters()}))
        model.zero_grad(set_to_none=True)
    (off, g_off), (on, g_on) = res
    for key in ("step_preds", "step_log_probas", "step_values", "step_pos", "step_actions"):
        assert th.equal(getattr(off, key), getattr(on, key)), key
    for n in g_off:
        assert th.equal(g_off[n], g_on[n]), n


def test_trainer_with_a_zero_coefficient_is_the_plain_trainer(device):
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    res = []
    for kwargs in ({}, {"entropy_coef": 0.0}):
        model = k.model(device)
        sampler = _sampler(k, model, device, probs=False)
        trainer = Trainer(model, k.cfg.nb_class, 1e-3, 0.99, **kwargs)
        scalars = [trainer.train_step(k.img, y, sampler)[1].clone() for _ in range(2)]
        assert scalars[0].numel() == 4
        res.append((th.stack(scalars), {n: v.clone() for n, v in model.state_dict().items()}))
    assert th.equal(res[0][0], res[1][0])
    for n in res[0][1]:
        assert th.equal(res[0][1][n], res[1][1][n]), n


# ---- 3: gradient through the distributions ----------------------------------------------------------------------
def _check_gradients(k, device, tag, only_probs=False, with_img=False, frozen=False):
    model = k.model(device)
    if frozen:
        model.requires_grad_(False)
    terms = _loss_terms(k)
    w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    img = k.img.to(device)
    if with_img:
        img.requires_grad_()
    ep = _sampler(k, model, device).run_episode(img)
    assert ep.step_probs.grad_fn is not None
    _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, terms, w, only_probs).backward()

    p64 = {n: v.double() for n, v in k.params.items()} if frozen else k.params64()
    img64 = k.img.double()
    if with_img:
        img64.requires_grad_()
    tr = _oracle_loop(k, p64, img64)
    assert th.equal(ep.step_pos.cpu(), tr["pos"]), "the episode moved otherwise than the oracle"
    _dist_loss(tr["preds"], tr["logp"], tr["values"], tr["probs"], terms, w, only_probs).backward()
    if with_img:
        assert img.grad is not None, "no gradient reached the image"
        REC.grad(f"{tag}/d_img", img.grad, img64.grad)
    if frozen:
        assert all(p.grad is None for p in model.parameters())
    else:
        REC.param_grads(f"{tag}/params", model, p64)


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_through_step_probs_match_float64_oracle(device, name):
    _check_gradients(Case(name), device, name)


@pytest.mark.parametrize("name", list(CASES))
def test_loss_on_step_probs_only(device, name):
    _check_gradients(Case(name), device, name + "/probs_only", only_probs=True)


@pytest.mark.parametrize("name", ["g1", "resisc3"])
def test_gradients_with_an_image_that_requires_grad(device, name):
    _check_gradients(Case(name), device, name + "/img", with_img=True)
    _check_gradients(Case(name), device, name + "/img_probs_only", only_probs=True, with_img=True)


@pytest.mark.parametrize("name", ["g1", "resisc3"])
def test_frozen_model_gives_the_image_gradient_only(device, name):
    _check_gradients(Case(name), device, name + "/frozen", with_img=True, frozen=True)


# ---- 4: the fused node equals the step loop ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_step_loop_gradients_equal_the_fused_episode(device, name):
    from marlclassification_amd.core import Environment
    from marlclassification_amd.networks.models import RecurrentOutput

    k = Case(name)
    model = k.model(device)
    terms = _loss_terms(k)
    w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    ep = _sampler(k, model, device).run_episode(k.img.to(device))
    _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, terms, w).backward()
    g_ep = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)

    i = k.inp
    env = Environment(k.cfg.actions, k.cfg.window)
    env.place(k.img.to(device), k.na, positions=i.pos0.to(device))
    obs = env.observe()
    rec = RecurrentOutput(*(t.to(device) for t in (i.h0, i.c0, i.hc0, i.cc0)))
    msg = th.zeros(k.na, k.nb, k.cfg.n_m, device=device)
    acc = {"preds": [], "logp": [], "values": [], "probs": []}
    for t in range(NS):
        out, rec = model(obs, msg, env.normalized_positions, rec)
        msg = out.messages
        a = ep.step_actions[t]
        logp = out.actions_probabilities.gather(-1, a.unsqueeze(-1)).squeeze(-1).log()
        obs = env.step(a)
        assert th.equal(env.positions, ep.step_pos[t])
        for key, v in zip(acc, (out.predictions, logp, out.values, out.actions_probabilities)):
            acc[key].append(v)
    o = {key: th.stack(v) for key, v in acc.items()}
    REC.fwd(f"{name}/loop_probs_vs_fused", o["probs"], ep.step_probs)
    _dist_loss(o["preds"], o["logp"], o["values"], o["probs"], terms, w).backward()
    for n, p in model.named_parameters():
        _close(p.grad, g_ep[n], GRAD_TOL, n)


# ---- 5: the fused loss ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.01, 0.5])
@pytest.mark.parametrize("name", ["g1", "wide"])
def test_fused_entropy_loss_matches_autograd(device, name, beta):
    k = Case(name)
    gamma = 0.97
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    eng, out = _engine_episode(k, device)
    bufs = [t.clone() for t in eng.a2c_loss(out, y.to(device), gamma, entropy_coef=beta)]
    assert len(bufs) == 6 and bufs[3].numel() == 5

    leaves = [t.detach().double().cpu().requires_grad_()
              for t in (out.step_preds, out.step_log_probas, out.step_values, out.step_probs)]
    lo = mo.a2c_loss(leaves[0], leaves[1], leaves[2], y, gamma)
    ent = masked_entropy(leaves[3])
    loss = lo.loss - beta * ent.sum(0).mean()
    loss.backward()
    ref_scalars = th.stack([loss, lo.path, lo.error, lo.critic, ent.mean()]).detach()
    tag = f"{name}/beta{beta}"
    for j, what in enumerate(("loss", "path", "error", "critic", "entropy")):
        REC.fwd(f"{tag}/scalar_{what}", bufs[3][j], ref_scalars[j])
    for got, leaf, what in zip((bufs[0], bufs[1], bufs[2], bufs[5]), leaves, ("g_preds", "g_logp", "g_values",
                                                                               "g_probs")):
        REC.grad(f"{tag}/{what}", got, leaf.grad)

    # two phases with the statistics untouched in between = phase 0, bit for bit; and a second run too
    two = eng.new_loss_bufs(out, True)
    eng.a2c_loss(out, y.to(device), gamma, 1, two, entropy_coef=beta)
    eng.a2c_loss(out, y.to(device), gamma, 2, two, entropy_coef=beta)
    again = eng.a2c_loss(out, y.to(device), gamma, entropy_coef=beta)
    for a, b, c in zip(bufs, two, again):
        assert th.equal(a, b), "phases 1 + 2 differ from phase 0"
        assert th.equal(a, c), "two runs differ"


# ---- 6: trainer ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1", "resisc3"])
def test_trainer_step_with_entropy_bonus_matches_oracle_update(device, name):
    from marlclassification_amd.training import Trainer

    k = Case(name)
    beta, lr, gamma = 0.05, 1e-3, 0.99
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    trainer = Trainer(model, k.cfg.nb_class, lr, gamma, entropy_coef=beta)
    trainer.train_epoch([(k.img, y)], 0, sampler)
    m = trainer.metrics()
    assert 0.0 < m["entropy"] <= math.log(k.cfg.nb_action) + 1e-6

    p64 = k.params64()
    tr = _oracle_loop(k, p64, k.img.double())
    lo = mo.a2c_loss(tr["preds"], tr["logp"], tr["values"], y, gamma)
    ent = masked_entropy(tr["probs"])
    loss = lo.loss - beta * ent.sum(0).mean()
    loss.backward()
    assert abs(m["loss"] - loss.item()) <= 2e-5 * abs(loss.item())
    assert abs(m["entropy"] - ent.mean().item()) <= FWD_TOL
    grads = {n: (v.grad if v.grad is not None else th.zeros_like(v)) for n, v in p64.items()}
    after = {n: v.detach().clone() for n, v in p64.items()}
    mo.adam_step(after, grads, {n: th.zeros_like(v) for n, v in after.items()},
                 {n: th.zeros_like(v) for n, v in after.items()}, 1, lr)
    sd = model.state_dict()
    for n in k.params:
        ref_upd = after[n] - k.params[n].double()
        upd = sd[n].double().cpu() - k.params[n].double()
        big = grads[n].abs() > 1e-6
        if big.any():
            assert (upd[big] - ref_upd[big]).abs().max().item() <= 1e-3 * lr, n


def test_graph_replay_with_entropy_bonus_equals_eager_iterations(device):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C, draw_episode_device
    from tests.util import Golden

    g = Golden("g2_mnist_c1")
    img, y = g.img.to(device), g.y.to(device)
    finals = []
    for use_graph in (False, True):
        eng = HipEngine(model_spec(g.cfg), device)
        eng.configure(g.na, g.nb, g.ns, g.img.shape[1:])
        eng.pack({n: v.to(device) for n, v in g.params.items()})
        flat = FlatParams(mo.param_shapes(g.cfg), device)
        flat.load(g.params)
        fa = FusedA2C(eng, flat, 1e-3, g.gamma, use_graph=use_graph, entropy_coef=0.01)
        losses, keys = [], []
        for it in range(7):  # graph: one eager + three replays, then a new coefficient: one eager + two replays
            if it == 4:
                fa.entropy_coef = 0.2
            if use_graph:
                out, sc = fa.iteration_graph(img, y, 77, it)
                keys.append(fa._graph[0])
            else:
                out, sc = fa.iteration(img, y, draw_episode_device(eng, 77, it))
            assert sc.numel() == 5
            losses.append(sc.clone())
        th.cuda.synchronize()
        finals.append((flat.params.clone(), th.stack(losses), out.step_pos.clone(), flat.step, keys))
    (p0, l0, pos0, s0, _), (p1, l1, pos1, s1, keys) = finals
    assert s0 == s1 == 7
    assert keys[0] == keys[3] and keys[4] == keys[6] and keys[3] != keys[4], "a new coefficient must re-capture"
    assert th.equal(pos0, pos1), "replayed episodes must draw the same positions / actions"
    assert th.allclose(l0, l1, rtol=1e-6, atol=1e-7), (l0, l1)
    assert bool((l0[:, 4] > 0).all()) and not th.equal(l0[3], l0[4])
    # the only difference allowed: Adam's bias correction computed on the device (1 ulp)
    assert (p0 - p1).abs().max().item() <= 1e-6 * p0.abs().max().item()


# ---- 7: exactly zero probabilities -----------------------------------------------------------------------------
def test_zero_probabilities_give_zero_entropy_and_finite_gradients(device):
    k = Case("g1")
    assert k.cfg.nb_action == 4
    k.params = dict(k.params)
    k.params[POL_BIAS] = th.tensor([200.0, 0.0, 0.0, 0.0])
    model = k.model(device)
    terms = _loss_terms(k)
    ep = _sampler(k, model, device).run_episode(k.img.to(device))
    one_hot = th.tensor([1.0, 0.0, 0.0, 0.0], device=device).expand_as(ep.step_probs)
    assert th.equal(ep.step_probs.detach(), one_hot), "precondition: the distributions are exactly [1, 0, 0, 0]"
    loss = (_a2c_like_loss(ep.step_preds, ep.step_log_probas, ep.step_values, terms) -
            0.37 * masked_entropy(ep.step_probs).sum(0).mean())
    assert bool(th.isfinite(loss))
    loss.backward()
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(th.isfinite(p.grad).all()), n

    p64 = k.params64()
    tr = _oracle_loop(k, p64, k.img.double())
    assert th.equal(ep.step_pos.cpu(), tr["pos"])
    assert 0 < tr["probs"][..., 1:].max().item() < 1e-80 and 0 < masked_entropy(tr["probs"]).max().item() < 1e-75
    (_a2c_like_loss(tr["preds"], tr["logp"], tr["values"], terms) -
     0.37 * masked_entropy(tr["probs"]).sum(0).mean()).backward()
    REC.param_grads("zero_prob/params", model, p64)  # every parameter, the policy head's included

    # the fused loss on the same distributions: entropy exactly 0, nothing NaN / Inf, and its backward too
    eng, out = _engine_episode(k, device)
    assert th.equal(out.step_probs, one_hot)
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen).to(device)
    gp, gl, gv, sc, _, gpr = eng.a2c_loss(out, y, 0.99, entropy_coef=0.5)
    assert sc[4].item() == 0.0 and bool(th.isfinite(sc).all())
    assert bool(th.isfinite(gpr).all()) and bool((gpr[..., 1:] == 0).all())
    ref = eng.a2c_loss(out, y, 0.99)
    assert th.equal(sc[:4], ref[3]), "a zero entropy leaves the plain loss"
    grads = {n: th.empty_like(p) for n, p in model.named_parameters()}
    eng.episode_backward(gp, gl, gv, grads, g_probs=gpr)
    assert all(bool(th.isfinite(v).all()) for v in grads.values())


# ---- 8: trajectory replay --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g1", "aid4"])
def test_replay_reproduces_and_follows_new_weights(device, name):
    k = Case(name)
    model = k.model(device)
    terms = _loss_terms(k)
    sampler = _sampler(k, model, device)
    img = k.img.to(device)
    first = sampler.run_episode(img)
    traj = sampler.last_trajectory
    assert th.equal(traj.actions, first.step_actions) and traj.actions.shape == (NS, k.na, k.nb)
    again = sampler.run_episode(img, replay=traj)
    with th.no_grad():
        plain = sampler.run_episode(img, replay=traj)
    for key in ("step_preds", "step_log_probas", "step_values", "step_pos", "step_actions", "step_probs"):
        assert th.equal(getattr(first, key).detach(), getattr(again, key).detach()), key
        assert th.equal(getattr(first, key).detach(), getattr(plain, key)), key

    # one optimiser step, then the stored trajectory under the new weights
    _a2c_like_loss(first.step_preds, first.step_log_probas, first.step_values, terms).backward()
    th.optim.SGD(model.parameters(), lr=0.05).step()
    model.zero_grad(set_to_none=True)
    new = sampler.run_episode(img, replay=traj)
    assert th.equal(new.step_pos, first.step_pos) and th.equal(new.step_actions, traj.actions)
    assert not th.equal(new.step_log_probas.detach(), first.step_log_probas.detach())
    ratio_loss = (new.step_log_probas - first.step_log_probas.detach()).exp().sum() + \
        _a2c_like_loss(new.step_preds, new.step_log_probas, new.step_values, terms)
    ratio_loss.backward()

    k.params = {n: v.detach().cpu().clone() for n, v in model.state_dict().items()}
    p64 = k.params64()
    tr = _oracle_loop(k, p64, k.img.double(), forced=traj.actions.cpu())
    assert th.equal(new.step_pos.cpu(), tr["pos"])
    REC.fwd(f"{name}/replay_logp", new.step_log_probas, tr["logp"])
    REC.fwd(f"{name}/replay_probs", new.step_probs, tr["probs"])
    old_logp = first.step_log_probas.detach().double().cpu()
    ((tr["logp"] - old_logp).exp().sum() + _a2c_like_loss(tr["preds"], tr["logp"], tr["values"], terms)).backward()
    REC.param_grads(f"{name}/replay_params", model, p64)


# ---- 9: guards -----------------------------------------------------------------------------------------------------
def test_guards(device):
    from marlclassification_amd.fused import FlatParams, FusedA2C
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    model = k.model(device)
    eng, out = _engine_episode(k, device)
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen).to(device)
    gp, gl, gv, _, _, gpr = eng.a2c_loss(out, y, 0.99, entropy_coef=0.1)
    grads = {n: th.empty_like(p) for n, p in model.named_parameters()}
    with pytest.raises(RuntimeError, match="g_probs"):
        eng.episode_backward(gp, gl, gv, grads, g_probs=gpr[:, :, :-1].contiguous())
    with pytest.raises(RuntimeError, match="g_probs"):
        eng.episode_backward(gp, gl, gv, grads, g_probs=gpr[..., :-1].contiguous())
    with pytest.raises(RuntimeError, match="g_probs"):
        eng.episode_backward(gp, gl, gv, grads, g_probs=gpr.cpu())
    with pytest.raises(ValueError, match="entropy_coef"):
        eng.a2c_loss(out, y, 0.99, entropy_coef=-0.1)
    plain = eng.episode_forward(k.img.to(device), *(t.to(device) for t in (k.inp.pos0, k.inp.h0, k.inp.c0, k.inp.hc0,
                                                                           k.inp.cc0, k.inp.q[:NS])), None, True)
    with pytest.raises(ValueError, match="step_probs"):
        eng.a2c_loss(plain, y, 0.99, entropy_coef=0.1)
    eng.episode_backward(gp, gl, gv, grads, generation=eng.fwd_generation, g_probs=gpr)  # the live episode still works
    assert all(bool(th.isfinite(v).all()) for v in grads.values())

    with pytest.raises(ValueError, match="entropy_coef"):
        Trainer(model, k.cfg.nb_class, 1e-3, 0.99, entropy_coef=-1e-3)
    with pytest.raises(ValueError, match="entropy_coef"):
        FusedA2C(eng, FlatParams(mo.param_shapes(k.cfg), device), 1e-3, 0.99, entropy_coef=-1.0)

    sampler = _sampler(k, model, device)
    with th.no_grad():
        sampler.run_episode(k.img.to(device))
    traj = sampler.last_trajectory
    with pytest.raises(ValueError, match="replay"):
        sampler.run_episode(k.img[:-1].to(device), replay=traj)
    from marlclassification_amd.core import Trajectory

    with pytest.raises(ValueError, match="replay"):
        sampler.run_episode(k.img.to(device), replay=Trajectory(traj.draws, traj.actions[:-1]))
