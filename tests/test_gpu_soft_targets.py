"""GPU: a target distribution per image in the fused loss (marl_soft_targets; the soft instances of loss_error_kernel /
loss_rewards_kernel) - through the three loss entries and marl_advantages, the trainer, hipGraph replay, two ranks and
``train --mix``.  The reference is float64 torch: ``class_loss.vote_error(targets=)`` / ``class_loss.rewards(targets=)``
(themselves held to ``F.cross_entropy`` with probabilities by tests/test_mix_host.py) fed into the restatement of the
remaining loss in tests/loss_ref.py, with the targets ``q`` given.  Bounds are those of tests/parity.py: FWD_TOL 1e-5
(x max(1, |ref|)) for forward quantities and scalars, GRAD_TOL 1e-4 of the tensor's scale for gradients, UPDATE_TOL
2e-3 lr for an Adam update.  Achieved errors go through its ``Recorder`` (profiles/mix_errors.json).

Shapes are those of tests/loss_cases.py: nC = 3 (less than a wave), 45, 70 (a second lane-stride pass with a ragged
tail); Na = 1, 3 with Nb = 5, Ns = 3; and Na = 16, Nb = 6 (Ns R = 288 > 256)."""
import dataclasses

import pytest
import torch as th
import torch.nn.functional as F

from marlclassification_amd import class_loss as cl
from oracle import marl_oracle as mo
from tests import loss_ref as ref64
from tests.cases import (NS, TWO_EPOCH, Case, _engine_episode, _golden_sampler, _grads_of, _oracle_loop, _sampler)
from tests.dp import run_ranks
from tests.loss_cases import (BETA, GAMMA, SHAPES, STEP_W, _engine, _entries, _setting, _trainer_options, all_on,
                              check_entries, synthetic, weights)
from tests.loss_ref import assert_clear_of_bounds, soft, under
from tests.parity import GRAD_TOL, UPDATE_TOL, Recorder
from tests.parity import close as _close
from tests.util import model_spec

pytestmark = pytest.mark.gpu

REC = Recorder("mix_errors", "soft_targets")


# ---- targets ------------------------------------------------------------------------------------------------------
def dense_targets(nb, nc, seed=0):
    """fp32 [nb, nc], rows summing to 1 (up to rounding): dense, but with exact zeros in row 1 and row 0 one-hot"""
    q = th.rand(nb, nc, generator=th.Generator().manual_seed(300 + seed + nb * nc)) + 0.05
    q[1, ::2] = 0.0
    q[0] = 0.0
    q[0, nc - 1] = 1.0
    return (q / q.sum(dim=1, keepdim=True)).float()


def entries(eng, out, y, device, c=None, q=None):
    """The outputs of every entry (cloned) with the options ``c`` and the targets ``q`` installed (None: not)."""
    with under(eng, c), soft(eng, q):
        return _entries(eng, out, y, device)


def check_all_entries(eng, out, y, c, q, tag, device):
    """a2c_loss (plain and entropy entry), advantages (lambda 1 and 0.9), ppo_loss (without and with the bonus) under
    the options ``c`` and the targets ``q`` (host fp32) against float64; phases 1 + 2 against phase 0 and a second run,
    bit for bit.  ``y`` is passed and must not be read."""
    with under(eng, c), soft(eng, q.to(device)):
        return check_entries(REC, eng, out, y, c, q, tag, device)


# ---- 1: float64 parity under dense targets ------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["plain", "all"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "nC{}_Na{}_Nb{}".format(*s))
def test_dense_targets_match_float64_through_every_entry(device, shape, setting):
    nc, na, nb = shape
    n_act = 6 if na == 3 else 4  # (scalar and float4 rows of the entropy pass)
    eng = _engine(nc, na, nb, NS, device, n_act)
    _, out, y = synthetic(nc, na, nb, NS, device, n_act)
    c = all_on(nc, y) if setting == "all" else None
    q = dense_targets(nb, nc)
    wrong_y = th.zeros_like(y)  # (the labels are passed and not read)
    kept = check_all_entries(eng, out, wrong_y, c, q, "{}/nC{}_Na{}_Nb{}".format(setting, *shape), device)
    assert eng.plan_query("soft_targets") == 0, "the engine clears the targets behind every call"
    if setting == "all":
        assert bool((kept["a2c0.0"][0][0] == 0).all()), "a step of weight 0 must get an exactly zero g_preds"
    label = entries(eng, out, y, device, c)
    assert not th.equal(label[0], kept["a2c0.0"][0]), "the targets must reach the vote error"
    assert not th.equal(label[12], kept["adv1.0"][5]), "... and the rewards"


@pytest.mark.parametrize("name", ["weights", "weights+rewards", "smoothing", "steps", "rewards_without_weights"])
def test_each_option_alone_under_dense_targets(device, name):
    nc, na, nb = 45, 3, 5
    eng = _engine(nc, na, nb, NS, device, 6)
    _, out, y = synthetic(nc, na, nb, NS, device, 6)
    w = weights(nc, 7, zero=int(y[1]))
    c = {"weights": cl.ClassLoss(nc, NS, w), "weights+rewards": cl.ClassLoss(nc, NS, w, weight_rewards=True),
         "smoothing": cl.ClassLoss(nc, NS, label_smoothing=0.1), "steps": cl.ClassLoss(nc, NS, step_weights=STEP_W),
         "rewards_without_weights": cl.ClassLoss(nc, NS, weight_rewards=True)}[name]
    check_all_entries(eng, out, y, c, dense_targets(nb, nc, 1), f"alone/{name}", device)


# ---- 2: a one-hot Q gives the bits of the integer-label call --------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 1, 5), (70, 3, 5), (45, 16, 6)], ids=lambda s: "nC{}_Na{}_Nb{}".format(*s))
def test_one_hot_targets_give_the_label_bits(device, shape):
    nc, na, nb = shape
    eng = _engine(nc, na, nb, NS, device)
    _, out, y = synthetic(nc, na, nb, NS, device, gap=200.0 if nc == 70 else None)
    hot = F.one_hot(y, nc).float().to(device)
    wrong_y = (y + 1) % nc
    settings = [None, all_on(nc, y), cl.ClassLoss(nc, NS, weights(nc, 9)), cl.ClassLoss(nc, NS, label_smoothing=0.1),
                cl.ClassLoss(nc, NS, weights(nc, 9), 0.1, STEP_W, True)]
    for k, c in enumerate(settings):
        label = entries(eng, out, y, device, c)
        got = entries(eng, out, wrong_y, device, c, hot)
        assert len(label) == len(got)
        for j, (a, b) in enumerate(zip(got, label)):
            assert th.equal(a, b), f"setting {k}: output {j} differs from the label call's"


def test_one_hot_targets_on_a_rollout_give_the_label_bits(device):
    k = Case("g1")
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    eng, out = _engine_episode(k, device)
    nc = k.cfg.nb_class
    hot = F.one_hot(y, nc).float().to(device)
    for c in (None, all_on(nc, y)):
        for j, (a, b) in enumerate(zip(entries(eng, out, y, device, c, hot), entries(eng, out, y, device, c))):
            assert th.equal(a, b), f"output {j} differs from the label call's"


# ---- 3: zeros are skipped, a logit gap of 200 stays finite --------------------------------------------------------
@pytest.mark.parametrize("nc", [3, 70])
def test_zero_targets_beside_a_logit_of_minus_infinity_stay_finite(device, nc):
    """Class j has weight 0, no target mass in image 1, and every agent's logit for it there is -inf: nll_j = +inf must
    stay out of every sum (0 * inf would be NaN), in the error, the rewards and the gradient."""
    na, nb, j = 3, 5, 0  # (dense_targets leaves image 1 no mass on the even classes)
    eng = _engine(nc, na, nb, NS, device)
    host, out, y = synthetic(nc, na, nb, NS, device, gap=200.0)
    preds = host.step_preds.clone()
    preds[:, :, 1, j] = -float("inf")
    out = dataclasses.replace(out, step_preds=preds.to(device))
    q = dense_targets(nb, nc, 2)
    assert q[1, j] == 0.0 and q[1].sum() > 0.99
    c = cl.ClassLoss(nc, NS, weights(nc, 9, zero=j), 0.0, STEP_W, True)
    def all_finite(kept):
        """what each entry wrote (advantages leaves the gradient buffers of its tuple alone, ppo_loss the statistics)"""
        for name, bufs in kept.items():
            wrote = range(len(bufs)) if name.startswith("a2c") else (4, 5, 6) if name.startswith("adv") else \
                (0, 1, 2, 3) + ((7,) if name == f"ppo{BETA}" else ())
            assert all(bool(th.isfinite(bufs[i]).all()) for i in wrote), name

    kept = check_all_entries(eng, out, y, c, q, f"minus_inf/nC{nc}", device)
    all_finite(kept)
    assert bool((kept["a2c0.0"][0][:, :, 1, j] == 0).all())
    # ... and without options
    all_finite(check_all_entries(eng, out, y, None, q, f"minus_inf_plain/nC{nc}", device))


# ---- 4: through the trainer ---------------------------------------------------------------------------------------
def _mixed_targets(y, nc, seed=0):
    """What a CutMix / Mixup loader yields for the labels ``y``: (primary labels, Q) from a drawn mix"""
    from marlclassification_amd import mix

    m = mix.parse("cutmix:1.0:0.5,mixup:0.4:0.5").draw(y.shape[0], th.Generator().manual_seed(40 + seed), (28, 28))
    return mix.primary_labels(y, m, 28, 28), mix.soft_targets(y, m, 28, 28, nc)


def test_train_step_under_targets_matches_the_float64_oracle_update(device):
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    lr, gamma, beta = 1e-3, 0.99, 0.05
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    yp, q = _mixed_targets(y, k.cfg.nb_class)
    assert int(((q > 0).sum(dim=1) == 2).sum()) > 0, "some image must carry two labels"
    opts = _trainer_options(k, y)
    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    trainer = Trainer(model, k.cfg.nb_class, lr, gamma, entropy_coef=beta, **opts)
    trainer.train_epoch([(k.img, yp, q.to(device))], 0, sampler)  # (the loaders' three-element batches)
    m = trainer.metrics()
    eng, _ = sampler.run_episode_raw(k.img, train=False)
    assert eng.soft_targets is None and eng.plan_query("soft_targets") == 0

    p64 = k.params64()
    tr = _oracle_loop(k, p64, k.img.double())
    loss, scalars = ref64.a2c(tr["preds"], tr["logp"], tr["values"], tr["probs"], y, gamma, beta, _setting(k, opts), q)
    loss.backward()
    REC.fwd("trainer/a2c/loss", th.tensor(m["loss"]), scalars[0])
    REC.fwd("trainer/a2c/error", th.tensor(m["error"]), scalars[2])
    grads = _grads_of(p64)
    after = {n: v.detach().clone() for n, v in p64.items()}
    mo.adam_step(after, grads, {n: th.zeros_like(v) for n, v in after.items()},
                 {n: th.zeros_like(v) for n, v in after.items()}, 1, lr)
    REC.check_update("trainer/a2c", k, model, after, [grads], lr)

    # the label trainer moves the weights elsewhere: the targets reached the update
    plain = k.model(device)
    Trainer(plain, k.cfg.nb_class, lr, gamma, entropy_coef=beta, **opts).train_epoch(
        [(k.img, y)], 0, _sampler(k, plain, device, probs=False))
    assert any(not th.equal(v, plain.state_dict()[n]) for n, v in model.state_dict().items())


def test_two_ppo_epochs_under_targets_match_the_float64_oracle_update(device):
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    lr, gamma, lam, beta = (TWO_EPOCH[n] for n in ("lr", "gamma", "lam", "beta"))
    eps = 0.1
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    # (draw 7: the float64 reference's second-epoch ratios stay 7.7e-4 / 1.2e-3 clear of the clip bounds, so fp32 clips
    # the entries the reference clips - assert_clear_of_bounds below; draw 1 puts one ratio 3e-5 from 1.1)
    yp, q = _mixed_targets(y, k.cfg.nb_class, 7)

    p = k.params64()
    img64 = k.img.double()
    tr = _oracle_loop(k, p, img64)
    advn, ret, _ = ref64.advantages(tr["preds"], tr["values"], y, gamma, lam, None, q)
    old_logp = tr["logp"].detach()
    loss = ref64.ppo(tr["preds"], tr["logp"], tr["values"], tr["probs"], y, old_logp, advn, ret, eps, beta, None, q)[0]
    loss.backward()
    g1 = _grads_of(p)
    after = {n: v.detach().clone() for n, v in p.items()}
    m1 = {n: th.zeros_like(v) for n, v in after.items()}
    v1 = {n: th.zeros_like(v) for n, v in after.items()}
    mo.adam_step(after, g1, m1, v1, 1, lr)
    p2 = {n: v.clone().requires_grad_() for n, v in after.items()}
    tr2 = _oracle_loop(k, p2, img64, forced=tr["act"])
    loss2, _, rho, _ = ref64.ppo(tr2["preds"], tr2["logp"], tr2["values"], tr2["probs"], y, old_logp, advn, ret, eps,
                                 beta, None, q)
    assert_clear_of_bounds(rho, eps)
    loss2.backward()
    g2 = _grads_of(p2)
    mo.adam_step(after, g2, m1, v1, 2, lr)

    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    trainer = Trainer(model, k.cfg.nb_class, lr, gamma, ppo_epochs=2, ppo_clip=eps, gae_lambda=lam, entropy_coef=beta)
    trainer.train_step(k.img, yp, sampler, targets=q.to(device))  # (same batch, same Q in both epochs)
    assert model.flat_state().step == 2
    REC.check_update("trainer/ppo", k, model, after, [g1, g2], lr)


def test_fused_iteration_is_the_trainers_step(device):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    _, q = _mixed_targets(y, k.cfg.nb_class, 2)
    qd = q.to(device)
    for kw in ({}, dict(ppo_epochs=2, ppo_clip=0.1, gae_lambda=0.9, entropy_coef=0.05)):
        model = k.model(device)
        sampler = _sampler(k, model, device, probs=False)
        _, sc_t = Trainer(model, k.cfg.nb_class, 1e-3, 0.99, **kw).train_step(k.img, y, sampler, targets=qd)
        eng = HipEngine(model_spec(k.cfg), device)
        eng.configure(k.na, k.nb, NS, k.img.shape[1:])
        flat = FlatParams(mo.param_shapes(k.cfg), device)
        flat.load(k.params)
        _, sc_f = FusedA2C(eng, flat, 1e-3, 0.99, **kw).iteration(k.img.to(device), y.to(device), sampler.fixed_draws,
                                                                targets=qd)
        assert th.equal(sc_t, sc_f)
        assert eng.soft_targets is None and eng.plan_query("soft_targets") == 0
        sd = model.state_dict()
        for n, v in flat.param_views().items():
            assert th.equal(v, sd[n]), n


def test_graph_replay_equals_eager_iterations(device):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C, draw_episode_device
    from tests.util import Golden

    g = Golden("g2_mnist_c1")
    img, y = g.img.to(device), g.y.to(device)
    _, q = _mixed_targets(g.y, g.cfg.nb_class, 3)
    qd = q.to(device)
    finals = []
    for use_graph, tgt in ((False, qd), (True, qd), (False, None)):
        eng = HipEngine(model_spec(g.cfg), device)
        eng.configure(g.na, g.nb, g.ns, g.img.shape[1:])
        eng.pack({n: v.to(device) for n, v in g.params.items()})
        flat = FlatParams(mo.param_shapes(g.cfg), device)
        flat.load(g.params)
        fa = FusedA2C(eng, flat, 1e-3, g.gamma, use_graph=use_graph)
        losses, keys = [], []
        for it in range(3):  # graph: one eager iteration (the capture), then two replays
            if use_graph:
                out, sc = fa.iteration_graph(img, y, 77, it, targets=tgt)
                keys.append(fa._graph[0])
            else:
                out, sc = fa.iteration(img, y, draw_episode_device(eng, 77, it), targets=tgt)
            losses.append(sc.clone())
        th.cuda.synchronize()
        assert eng.plan_query("soft_targets") == 0
        finals.append((flat.params.clone(), th.stack(losses), out.step_pos.clone(), flat.step, keys))
    (p0, l0, pos0, s0, _), (p1, l1, pos1, s1, keys), (_, lplain, _, _, _) = finals
    assert s0 == s1 == 3 and keys[0] == keys[2], "the replays must reuse the capture"
    assert qd.data_ptr() in keys[0], "the graph is keyed by the targets' storage"
    assert th.equal(pos0, pos1), "replayed episodes must draw the same positions / actions"
    assert th.allclose(l0, l1, rtol=1e-6, atol=1e-7), (l0, l1)
    assert not th.allclose(l0[:, 2], lplain[:, 2], rtol=1e-3), "the targets must reach the captured loss"
    # the only difference allowed: Adam's bias correction computed on the device (1 ulp)
    assert (p0 - p1).abs().max().item() <= 1e-6 * p0.abs().max().item()


def test_command_line_trains_with_mix_and_augment(device, tmp_path, capsys):
    import json

    from marlclassification_amd.__main__ import main

    out = tmp_path / "run"
    main((f"-a 3 --step 3 --cuda --run-id mix train --ft-extr mnist --f 6 --img-size 28 --nb-class 10 --nb 16 --na 16 "
          f"--nm 8 --nmo 12 --nd 4 --nlb 24 --nla 24 --batch-size 16 --nb-epoch 1 --lr 1e-3 --res-folder synthetic "
          f"--mix cutmix:1.0,mixup:0.4:0.3 --augment hflip -o {out}").split())
    printed = capsys.readouterr().out
    assert "mix cutmix:1.0,mixup:0.4:0.3" in printed and "augment hflip" in printed and "epoch 0:" in printed
    cfg = json.loads((out / "marl.json").read_text())
    assert "mix" not in cfg and "augment" not in cfg
    sd = th.load(out / "models" / "nn_models_epoch_0.pt", map_location="cpu")
    assert all(bool(th.isfinite(v).all()) for v in sd.values())


# ---- 5: two ranks ---------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_q):
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from marlclassification_amd.fused import EpisodeDraws
    from marlclassification_amd.parallel import GradAllReduce, broadcast_parameters, shard_bounds
    from marlclassification_amd.training import Trainer
    from tests.util import Golden

    device = th.device("cuda:0")  # both ranks share the one GPU of the test box
    g = Golden("g2_mnist_c1")
    model, sampler = _golden_sampler(g, device)
    broadcast_parameters(model.flat_state().params)
    lo, hi = shard_bounds(g.nb, rank, world)
    i = g.inp
    sampler.fixed_draws = EpisodeDraws(*(t.to(device) for t in (
        i.pos0[:, lo:hi].contiguous(), i.h0[:, lo:hi].contiguous(), i.c0[:, lo:hi].contiguous(),
        i.hc0[:, lo:hi].contiguous(), i.cc0[:, lo:hi].contiguous(), i.q[:, :, lo:hi].contiguous())))
    _, q = _mixed_targets(g.y, g.cfg.nb_class, 4)
    trainer = Trainer(model, g.cfg.nb_class, g.lr, g.gamma, allreduce=GradAllReduce(world),
                      exact_standardize_group=dist.group.WORLD, label_smoothing=0.1)
    for _ in range(2):
        trainer.train_step(g.img[lo:hi], g.y[lo:hi], sampler, targets=q[lo:hi].contiguous().to(device))
    th.cuda.synchronize()
    sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}  # numpy: plain pickles
    if rank == 0:
        out_q.put((sd, model.flat_state().grads.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_take_the_big_batch_update(device):
    """Two processes, each on half of the G2 batch and its half of Q, with the flat-gradient all-reduce and the
    exact-standardize exchange (phases 1 and 2 under the targets), two steps; the reference is the single-process
    trainer on the whole batch under the whole Q - itself held to float64 by the trainer tests above."""
    from marlclassification_amd.training import Trainer
    from tests.util import Golden

    (sd, flat_grads), = run_ranks(_dp_worker, 2)
    sd = {n: th.from_numpy(v) for n, v in sd.items()}
    flat_grads = th.from_numpy(flat_grads)

    g = Golden("g2_mnist_c1")
    _, q = _mixed_targets(g.y, g.cfg.nb_class, 4)
    model, sampler = _golden_sampler(g, device)
    trainer = Trainer(model, g.cfg.nb_class, g.lr, g.gamma, label_smoothing=0.1)
    for _ in range(2):
        trainer.train_step(g.img, g.y, sampler, targets=q.to(device))
    ref_grads = model.flat_state().grads.cpu()
    # the ranks' flat gradient buffer holds the SUM over the ranks (the 1 / world scale is Adam's)
    _close(flat_grads / 2, ref_grads, GRAD_TOL, "flat gradient of the second step")
    ref_sd = model.state_dict()
    worst, moved = 0.0, False
    for n in g.params:
        ref_upd = ref_sd[n].double().cpu() - g.params[n].double()
        upd = sd[n].double() - g.params[n].double()
        err = (upd - ref_upd).abs().max().item()
        worst = max(worst, err)
        moved = moved or bool((upd != 0).any())
        assert err <= UPDATE_TOL * g.lr, f"{n}: {err:.3e}"
    assert moved
    REC.put("two_ranks/update", {"max_err": worst, "tol": UPDATE_TOL * g.lr})


# ---- 6: guards, and nothing stays installed -------------------------------------------------------------------------
def test_guards_refuse_before_anything_is_enqueued_and_nothing_stays_installed(device):
    import ctypes as C
    import re

    from marlclassification_amd._lib import check
    from marlclassification_amd.engine import _nbytes, _stream
    from tests.util import ROOT

    nc, na, nb = 45, 3, 5
    eng = _engine(nc, na, nb, NS, device)
    _, out, y = synthetic(nc, na, nb, NS, device)
    yd = y.to(device)
    assert eng.plan_query("soft_targets") == 0
    before = entries(eng, out, y, device)
    poisoned = eng.new_loss_bufs(out)
    for t in poisoned:
        t.fill_(7.0)

    def untouched():
        th.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in poisoned), "a refused call wrote its outputs"

    good = dense_targets(nb, nc).to(device)
    nan, neg, zero_row = good.clone(), good.clone(), good.clone()
    nan[2, 3], neg[2, 3], zero_row[3] = float("nan"), -0.1, 0.0
    for bad, err in ((good.cpu(), RuntimeError), (good.double(), TypeError), (good[:, :-1].contiguous(), ValueError),
                     (good[:-1].contiguous(), ValueError), (good.t().contiguous().t(), ValueError),
                     (good.view(-1), ValueError), (nan, ValueError), (neg, ValueError), (zero_row, ValueError),
                     (good.tolist(), TypeError)):
        with pytest.raises(err):
            eng.set_soft_targets(bad)
        assert eng.soft_targets is None
    wrong = dense_targets(nb + 1, nc).to(device)
    eng.soft_targets = wrong  # (set before the engine was configured for these sizes: refused at the call)
    try:
        with pytest.raises(ValueError, match="configured"):
            eng.a2c_loss(out, yd, GAMMA, 0, poisoned)
        with pytest.raises(ValueError, match="configured"):
            eng.advantages(out, yd, GAMMA, 0.9)
    finally:
        eng.set_soft_targets(None)
    untouched()

    # the library itself: MARL_EINVAL for a setting whose sizes disagree with cfg, before anything is enqueued
    with open(f"{ROOT}/include/marl_hip.h", "r", encoding="utf-8") as f:
        einval = int(re.search(r"#define MARL_EINVAL \((-?\d+)\)", f.read()).group(1))
    lib, cfg, ews = eng.lib, eng.cfg, eng.episode_ws(True)
    gp, gl, gv, sc, st = poisoned

    def a2c_direct():
        return lib.marl_a2c_loss_fwd_bwd(C.byref(cfg), ews.data_ptr(), _nbytes(ews), out.step_preds.data_ptr(),
                                         out.step_log_probas.data_ptr(), out.step_values.data_ptr(), yd.data_ptr(),
                                         C.c_float(GAMMA), gp.data_ptr(), gl.data_ptr(), gv.data_ptr(), sc.data_ptr(),
                                         st.data_ptr(), 0, _stream(device))

    assert lib.marl_soft_targets(good.data_ptr(), -1, nc) == einval
    assert lib.marl_soft_targets(good.data_ptr(), 0, nc) == einval
    assert eng.plan_query("soft_targets") == 0, "a refused setting must not be installed"
    try:
        for sizes in ((nb + 1, nc), (nb, nc - 1)):
            check(lib.marl_soft_targets(wrong.data_ptr(), *sizes))
            assert eng.plan_query("soft_targets") == 1
            assert a2c_direct() == einval
            assert b"soft targets" in lib.marl_last_error()
            untouched()
    finally:
        check(lib.marl_soft_targets(None, 0, 0))
    assert eng.plan_query("soft_targets") == 0

    # under targets, then cleared: the next plain call gives the bits of one made before
    under_q = entries(eng, out, y, device, None, good)
    assert not th.equal(under_q[0], before[0])
    assert eng.soft_targets is None and eng.plan_query("soft_targets") == 0
    for a, b in zip(entries(eng, out, y, device), before):
        assert th.equal(a, b), "install, clear, call again: the plain bits once more"
