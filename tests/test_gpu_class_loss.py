"""GPU: class weights, label smoothing and step weights of the vote error, and cost-sensitive rewards, in the fused
loss (marl_class_loss; the option instances of loss_error_kernel / loss_rewards_kernel) - through the three loss
entries and marl_advantages, the trainer, hipGraph replay and two ranks.  The reference is float64 torch:
``class_loss.vote_error`` / ``class_loss.rewards`` fed into the restatement of the remaining loss in tests/loss_ref.py
(the oracle's returns / standardise, its GAE recursion, ``torch.minimum`` / ``clamp`` and ``smooth_l1_loss``), with the
options ``c`` given.  Bounds are those of tests/parity.py: FWD_TOL 1e-5 (x max(1, |ref|)) for forward quantities and
scalars, GRAD_TOL 1e-4 of the tensor's scale for gradients, UPDATE_TOL 2e-3 lr for an Adam update.  Achieved errors go
through its ``Recorder`` (copied into profiles/class_loss_errors.json after the box run).

Shapes (tests/loss_cases.py): nC = 3 (less than a wave), 45, 70 (a second lane-stride pass with a ragged tail); Na = 1, 3
with Nb = 5, Ns = 3 (Ns Nb = 15 and Ns R leave partial four-wave blocks); and Na = 16, Nb = 6 (Ns R = 288 > 256: the
extra partials of the entropy / PPO passes sit where the weighted rewards were)."""
import pytest
import torch as th

from marlclassification_amd import class_loss as cl
from oracle import marl_oracle as mo
from tests import loss_ref as ref64
from tests.cases import (NS, TWO_EPOCH, Case, _engine_episode, _golden_sampler, _grads_of, _oracle_loop, _sampler)
from tests.dp import run_ranks
from tests.loss_cases import (GAMMA, SHAPES, STEP_W, _engine, _entries, _setting, _trainer_options, all_on,
                              check_entries, synthetic, weights)
from tests.loss_ref import assert_clear_of_bounds, under
from tests.parity import GRAD_TOL, UPDATE_TOL, Recorder
from tests.parity import close as _close
from tests.util import model_spec

pytestmark = pytest.mark.gpu

REC = Recorder("class_loss_errors", "class_loss")


# ---- one setting through every entry ------------------------------------------------------------------------------
def check_all_entries(eng, out, y, c, tag, device):
    with under(eng, c):
        return check_entries(REC, eng, out, y, c, None, tag, device)


def plain_entries(eng, out, y, device, c=None):
    """The outputs of every entry (cloned) with ``c`` installed - None: nothing installed."""
    with under(eng, c):
        return _entries(eng, out, y, device)


@pytest.fixture(scope="module", autouse=True)
def pristine(device):
    """What the entries give before this module installs its first setting.  No loss entry has run under a setting in
    this process by then: the only other caller of marl_class_loss, the guard test of tests/test_class_loss_host.py,
    installs and clears without launching anything."""
    eng = _engine(45, 16, 6, NS, device)
    assert eng.plan_query("class_loss") == 0
    _, out, y = synthetic(45, 16, 6, NS, device)
    return plain_entries(eng, out, y, device)


# ---- 1: float64 parity at the shapes where the kernels can go wrong ---------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "nC{}_Na{}_Nb{}".format(*s))
def test_all_options_match_float64_through_every_entry(device, shape):
    nc, na, nb = shape
    n_act = 6 if na == 3 else 4  # (scalar and float4 rows of the entropy pass)
    eng = _engine(nc, na, nb, NS, device, n_act)
    _, out, y = synthetic(nc, na, nb, NS, device, n_act)
    c = all_on(nc, y)
    kept = check_all_entries(eng, out, y, c, "all/nC{}_Na{}_Nb{}".format(*shape), device)
    assert bool((kept["a2c0.0"][0][0] == 0).all()), "a step of weight 0 must get an exactly zero g_preds"
    assert bool((kept["a2c0.0"][0][:, :, 0] != 0).any()), "smoothing reaches an image whose class has weight 0"


# ---- 2: each option alone, on a real rollout ----------------------------------------------------------------------
def _alone(name, nc, y):
    w = weights(nc, 7, zero=int(y[1]))
    return {
        "weights": cl.ClassLoss(nc, NS, w),
        "weights+rewards": cl.ClassLoss(nc, NS, w, weight_rewards=True),
        "smoothing": cl.ClassLoss(nc, NS, label_smoothing=0.1),
        "last": cl.ClassLoss(nc, NS, step_weights=cl.step_schedule("last", NS)),
        "linear": cl.ClassLoss(nc, NS, step_weights=cl.step_schedule("linear", NS)),
        "rewards_without_weights": cl.ClassLoss(nc, NS, weight_rewards=True),
    }[name]


@pytest.mark.parametrize("name", ["weights", "weights+rewards", "smoothing", "last", "linear",
                                  "rewards_without_weights"])
def test_each_option_alone_on_a_rollout(device, name):
    k = Case("g1")
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    eng, out = _engine_episode(k, device)
    c = _alone(name, k.cfg.nb_class, y)
    plain = plain_entries(eng, out, y, device)
    kept = check_all_entries(eng, out, y, c, f"alone/{name}", device)
    gp = kept["a2c0.0"][0]
    if name == "last":
        assert bool((gp[:-1] == 0).all()) and bool((kept["ppo0.05"][0][:-1] == 0).all())
        assert th.equal(gp[-1], plain[0][-1]), "the last step's gradient is the plain one"
    if name.startswith("weights"):
        assert bool((gp[:, :, 1] == 0).all()), "an image whose class has weight 0 asks nothing of the vote"
    # the rewards change with weight_rewards and class weights only: otherwise the advantages are the plain bits
    adv_plain = plain[11:17]
    adv = [kept[f"adv{lam}"][j] for lam in (1.0, 0.9) for j in (4, 5, 6)]
    same = all(th.equal(a, b) for a, b in zip(adv, adv_plain))
    assert same == (name != "weights+rewards")
    if name == "rewards_without_weights":
        for a, b in zip(plain_entries(eng, out, y, device, c), plain):
            assert th.equal(a, b)


# ---- 3: a logit gap of 200 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [3, 70])
def test_a_logit_gap_of_200_stays_finite_and_accurate(device, nc):
    na, nb = 3, 5
    eng = _engine(nc, na, nb, NS, device)
    host, out, y = synthetic(nc, na, nb, NS, device, gap=200.0)
    z = host.step_preds.mean(dim=1)
    assert (z.max(-1).values - z.min(-1).values).max().item() >= 200.0
    c = cl.ClassLoss(nc, NS, weights(nc, 9), 0.1, STEP_W, True)
    kept = check_all_entries(eng, out, y, c, f"gap200/nC{nc}", device)
    err_mean = kept["a2c0.0"][3][2].item()
    assert err_mean > 10.0, "the confident wrong votes must show in the error"


# ---- 4: neutral options are exact ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 1, 5), (70, 3, 5), (45, 16, 6)], ids=lambda s: "nC{}_Na{}_Nb{}".format(*s))
def test_neutral_options_give_the_plain_bits(device, shape):
    nc, na, nb = shape
    eng = _engine(nc, na, nb, NS, device)
    _, out, y = synthetic(nc, na, nb, NS, device, gap=200.0 if nc == 70 else None)
    neutral = cl.ClassLoss(nc, NS, [1.0] * nc, 0.0, [1.0] * NS, True)
    assert not neutral.is_default
    plain = plain_entries(eng, out, y, device)
    got = plain_entries(eng, out, y, device, neutral)
    assert len(plain) == len(got)
    for j, (a, b) in enumerate(zip(got, plain)):
        assert th.equal(a, b), f"output {j} differs from the plain entry's"


def test_neutral_options_on_a_rollout_give_the_plain_bits(device):
    k = Case("g1")
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    eng, out = _engine_episode(k, device)
    nc = k.cfg.nb_class
    plain = plain_entries(eng, out, y, device)
    for c in (cl.ClassLoss(nc, NS, [1.0] * nc, 0.0, [1.0] * NS, True), cl.ClassLoss(nc, NS, [1.0] * nc),
              cl.ClassLoss(nc, NS, step_weights=[1.0] * NS)):
        for j, (a, b) in enumerate(zip(plain_entries(eng, out, y, device, c), plain)):
            assert th.equal(a, b), f"output {j} differs from the plain entry's"


# ---- 5: defaults ----------------------------------------------------------------------------------------------------
def test_defaults_launch_what_they_launched_before_any_setting(device, pristine):
    import ctypes as C

    eng = _engine(45, 16, 6, NS, device)
    _, out, y = synthetic(45, 16, 6, NS, device)
    c = all_on(45, y)
    assert eng.plan_query("class_loss") == 0
    for a, b in zip(plain_entries(eng, out, y, device), pristine):
        assert th.equal(a, b)
    with_options = plain_entries(eng, out, y, device, c)
    assert not th.equal(with_options[0], pristine[0])
    assert eng.plan_query("class_loss") == 0, "the engine clears the setting behind every call"
    w = th.ones(45, device=device)
    assert eng.lib.marl_class_loss(w.data_ptr(), 45, C.c_float(0.0), None, 0, 0) == 0
    try:
        assert eng.plan_query("class_loss") == 1
    finally:
        assert eng.lib.marl_class_loss(None, 0, C.c_float(0.0), None, 0, 0) == 0
    assert eng.plan_query("class_loss") == 0
    for a, b in zip(plain_entries(eng, out, y, device), pristine):
        assert th.equal(a, b), "install, clear, call again: the plain bits once more"
    # None and a ClassLoss with nothing given are the same plain call
    for a, b in zip(plain_entries(eng, out, y, device, cl.ClassLoss(45, NS)), pristine):
        assert th.equal(a, b)


# ---- 6: through the trainer ---------------------------------------------------------------------------------------
def test_train_step_matches_the_float64_oracle_update(device):
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    lr, gamma, beta = 1e-3, 0.99, 0.05
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    opts = _trainer_options(k, y)
    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    trainer = Trainer(model, k.cfg.nb_class, lr, gamma, entropy_coef=beta, **opts)
    trainer.train_epoch([(k.img, y)], 0, sampler)
    m = trainer.metrics()

    p64 = k.params64()
    tr = _oracle_loop(k, p64, k.img.double())
    loss, scalars = ref64.a2c(tr["preds"], tr["logp"], tr["values"], tr["probs"], y, gamma, beta, _setting(k, opts))
    loss.backward()
    REC.fwd("trainer/a2c/loss", th.tensor(m["loss"]), scalars[0])
    REC.fwd("trainer/a2c/error", th.tensor(m["error"]), scalars[2])
    grads = _grads_of(p64)
    after = {n: v.detach().clone() for n, v in p64.items()}
    mo.adam_step(after, grads, {n: th.zeros_like(v) for n, v in after.items()},
                 {n: th.zeros_like(v) for n, v in after.items()}, 1, lr)
    REC.check_update("trainer/a2c", k, model, after, [grads], lr)

    # the plain trainer moves the weights elsewhere: the options reached the update
    plain = k.model(device)
    Trainer(plain, k.cfg.nb_class, lr, gamma, entropy_coef=beta).train_epoch(
        [(k.img, y)], 0, _sampler(k, plain, device, probs=False))
    assert any(not th.equal(v, plain.state_dict()[n]) for n, v in model.state_dict().items())


def test_two_ppo_epochs_match_the_float64_oracle_update(device):
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    lr, gamma, lam, beta = (TWO_EPOCH[n] for n in ("lr", "gamma", "lam", "beta"))
    eps = 0.1
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    opts = _trainer_options(k, y)
    c = _setting(k, opts)

    p = k.params64()
    img64 = k.img.double()
    tr = _oracle_loop(k, p, img64)
    advn, ret, _ = ref64.advantages(tr["preds"], tr["values"], y, gamma, lam, c)
    old_logp = tr["logp"].detach()
    loss = ref64.ppo(tr["preds"], tr["logp"], tr["values"], tr["probs"], y, old_logp, advn, ret, eps, beta, c)[0]
    loss.backward()
    g1 = _grads_of(p)
    after = {n: v.detach().clone() for n, v in p.items()}
    m1 = {n: th.zeros_like(v) for n, v in after.items()}
    v1 = {n: th.zeros_like(v) for n, v in after.items()}
    mo.adam_step(after, g1, m1, v1, 1, lr)
    p2 = {n: v.clone().requires_grad_() for n, v in after.items()}
    tr2 = _oracle_loop(k, p2, img64, forced=tr["act"])
    loss2, sc2, rho, _ = ref64.ppo(tr2["preds"], tr2["logp"], tr2["values"], tr2["probs"], y, old_logp, advn, ret, eps,
                                   beta, c)
    assert_clear_of_bounds(rho, eps)
    frac_ref = sc2[6].item()
    assert 0.0 < frac_ref < 1.0, "the reference must clip some entries in the second epoch, not all"
    loss2.backward()
    g2 = _grads_of(p2)
    mo.adam_step(after, g2, m1, v1, 2, lr)

    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    trainer = Trainer(model, k.cfg.nb_class, lr, gamma, ppo_epochs=2, ppo_clip=eps, gae_lambda=lam, entropy_coef=beta,
                      **opts)
    trainer.train_epoch([(k.img, y)], 0, sampler)
    assert model.flat_state().step == 2
    m = trainer.metrics()
    assert m["clip_frac"] == th.tensor(frac_ref, dtype=th.float64).float().item()
    REC.fwd("trainer/ppo/error", th.tensor(m["error"]), sc2[2])
    REC.fwd("trainer/ppo/loss", th.tensor(m["loss"]), sc2[0])
    REC.check_update("trainer/ppo", k, model, after, [g1, g2], lr)


def test_fused_iteration_is_the_trainers_step(device):
    """``FusedA2C.iteration`` and ``Trainer.train_step`` with the same options: same draws, same bits (A2C and PPO)."""
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    opts = _trainer_options(k, y)
    for kw in ({}, dict(ppo_epochs=2, ppo_clip=0.1, gae_lambda=0.9, entropy_coef=0.05)):
        model = k.model(device)
        sampler = _sampler(k, model, device, probs=False)
        _, sc_t = Trainer(model, k.cfg.nb_class, 1e-3, 0.99, **kw, **opts).train_step(k.img, y, sampler)
        eng = HipEngine(model_spec(k.cfg), device)
        eng.configure(k.na, k.nb, NS, k.img.shape[1:])
        flat = FlatParams(mo.param_shapes(k.cfg), device)
        flat.load(k.params)
        own = cl.ClassLoss(k.cfg.nb_class, NS, label_smoothing=0.3)
        eng.set_class_loss(own)
        _, sc_f = FusedA2C(eng, flat, 1e-3, 0.99, **kw, **opts).iteration(k.img.to(device), y.to(device),
                                                                        sampler.fixed_draws)
        assert th.equal(sc_t, sc_f)
        assert eng.class_loss is own, "the engine's own setting must be back behind the iteration"
        model_eng, _ = sampler.run_episode_raw(k.img, train=False)
        assert model_eng.class_loss is None, "a later trainer on this model must not inherit the options"
        sd = model.state_dict()
        for n, v in flat.param_views().items():
            assert th.equal(v, sd[n]), n


def test_graph_replay_equals_eager_iterations(device):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C, draw_episode_device
    from tests.util import Golden

    g = Golden("g2_mnist_c1")
    img, y = g.img.to(device), g.y.to(device)
    opts = dict(class_weights=weights(g.cfg.nb_class, 22, zero=int(g.y[0])).tolist(), label_smoothing=0.1,
                error_step_weights="linear", weight_rewards=True)
    finals = []
    for use_graph, kw in ((False, opts), (True, opts), (False, {})):
        eng = HipEngine(model_spec(g.cfg), device)
        eng.configure(g.na, g.nb, g.ns, g.img.shape[1:])
        eng.pack({n: v.to(device) for n, v in g.params.items()})
        flat = FlatParams(mo.param_shapes(g.cfg), device)
        flat.load(g.params)
        fa = FusedA2C(eng, flat, 1e-3, g.gamma, use_graph=use_graph, **kw)
        losses, keys = [], []
        for it in range(3):  # graph: one eager iteration (the capture), then two replays
            if use_graph:
                out, sc = fa.iteration_graph(img, y, 77, it)
                keys.append(fa._graph[0])
            else:
                out, sc = fa.iteration(img, y, draw_episode_device(eng, 77, it))
            losses.append(sc.clone())
        th.cuda.synchronize()
        assert eng.plan_query("class_loss") == 0
        finals.append((flat.params.clone(), th.stack(losses), out.step_pos.clone(), flat.step, keys))
    (p0, l0, pos0, s0, _), (p1, l1, pos1, s1, keys), (_, lplain, _, _, _) = finals
    assert s0 == s1 == 3 and keys[0] == keys[2], "the replays must reuse the capture"
    assert th.equal(pos0, pos1), "replayed episodes must draw the same positions / actions"
    assert th.allclose(l0, l1, rtol=1e-6, atol=1e-7), (l0, l1)
    assert not th.allclose(l0[:, 2], lplain[:, 2], rtol=1e-3), "the options must reach the captured loss"
    # the only difference allowed: Adam's bias correction computed on the device (1 ulp)
    assert (p0 - p1).abs().max().item() <= 1e-6 * p0.abs().max().item()


def test_command_line_trains_with_the_four_options(device, tmp_path, capsys):
    import json

    from marlclassification_amd.__main__ import main

    out = tmp_path / "run"
    main((f"-a 3 --step 3 --cuda --run-id cl train --ft-extr mnist --f 6 --img-size 28 --nb-class 10 --nb 16 --na 16 "
          f"--nm 8 --nmo 12 --nd 4 --nlb 24 --nla 24 --batch-size 16 --nb-epoch 1 --lr 1e-3 --res-folder synthetic "
          f"--class-weights balanced --label-smoothing 0.1 --error-steps last:2 --weight-rewards -o {out}").split())
    printed = capsys.readouterr().out
    assert "class weights balanced" in printed and "label_smoothing 0.1" in printed
    assert "error steps last:2" in printed and "weighted rewards" in printed and "epoch 0:" in printed
    cfg = json.loads((out / "marl.json").read_text())
    assert not any(k in cfg for k in ("class_weights", "label_smoothing", "error_steps", "weight_rewards"))
    sd = th.load(out / "models" / "nn_models_epoch_0.pt", map_location="cpu")
    assert all(bool(th.isfinite(v).all()) for v in sd.values())
    assert not any("class" in k and "loss" in k for k in sd)
    with pytest.raises(ValueError, match="steps"):  # (last:K is checked against --step before anything trains)
        main((f"-a 3 --step 3 --cuda --run-id cl train --ft-extr mnist --f 6 --img-size 28 --res-folder synthetic "
              f"--error-steps last:4 -o {out}").split())


# ---- 7: two ranks ---------------------------------------------------------------------------------------------------
DP_OPTS = dict(label_smoothing=0.1, error_step_weights="last:3", weight_rewards=True)


def _dp_weights(nc, y):
    return weights(nc, 23, zero=int(y[0])).tolist()


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
    trainer = Trainer(model, g.cfg.nb_class, g.lr, g.gamma, allreduce=GradAllReduce(world),
                      exact_standardize_group=dist.group.WORLD,
                      class_weights=_dp_weights(g.cfg.nb_class, g.y), **DP_OPTS)
    for _ in range(2):
        trainer.train_step(g.img[lo:hi], g.y[lo:hi], sampler)
    th.cuda.synchronize()
    sd = {k: v.cpu().numpy() for k, v in model.state_dict().items()}  # numpy: plain pickles
    if rank == 0:
        out_q.put((sd, model.flat_state().grads.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_take_the_big_batch_update(device):
    """Two processes, each on half of the G2 batch with the flat-gradient all-reduce and the exact-standardize
    exchange (phases 1 and 2 under the options), two steps.  With global statistics the averaged gradient is the
    big-batch one, so the reference is the single-process trainer on the whole batch under the same options - itself
    held to float64 by the trainer tests above; the two differ by fp32 summation order only, far inside the gradient
    and update bounds."""
    from marlclassification_amd.training import Trainer
    from tests.util import Golden

    (sd, flat_grads), = run_ranks(_dp_worker, 2)
    sd = {n: th.from_numpy(v) for n, v in sd.items()}
    flat_grads = th.from_numpy(flat_grads)

    g = Golden("g2_mnist_c1")
    model, sampler = _golden_sampler(g, device)
    trainer = Trainer(model, g.cfg.nb_class, g.lr, g.gamma, class_weights=_dp_weights(g.cfg.nb_class, g.y), **DP_OPTS)
    for _ in range(2):
        trainer.train_step(g.img, g.y, sampler)
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


# ---- 8: guards ------------------------------------------------------------------------------------------------------
def test_guards_refuse_before_anything_is_enqueued(device):
    import ctypes as C
    import re

    from marlclassification_amd._lib import check
    from marlclassification_amd.engine import _nbytes, _stream
    from tests.util import ROOT

    nc, na, nb = 45, 3, 5
    eng = _engine(nc, na, nb, NS, device)
    _, out, y = synthetic(nc, na, nb, NS, device)
    yd = y.to(device)
    before = [t.clone() for t in eng.a2c_loss(out, yd, GAMMA)]
    poisoned = eng.new_loss_bufs(out)
    for t in poisoned:
        t.fill_(7.0)

    def untouched():
        th.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in poisoned), "a refused call wrote its outputs"

    for kw in ({"label_smoothing": 1.0}, {"class_weights": [1.0] * (nc - 1)}, {"class_weights": [float("nan")] * nc},
               {"step_weights": [1.0] * (NS + 1)}):
        with pytest.raises(ValueError):
            eng.set_class_loss(cl.ClassLoss(nc, NS, **kw))
    for wrong in (cl.ClassLoss(nc + 1, NS, label_smoothing=0.1), cl.ClassLoss(nc, NS + 1, label_smoothing=0.1)):
        with pytest.raises(ValueError, match="configured"):
            eng.set_class_loss(wrong)
        eng.class_loss = wrong  # (set before the engine was configured for these sizes: refused at the call)
        try:
            with pytest.raises(ValueError, match="configured"):
                eng.a2c_loss(out, yd, GAMMA, 0, poisoned)
            with pytest.raises(ValueError, match="configured"):
                eng.advantages(out, yd, GAMMA, 0.9)
        finally:
            eng.set_class_loss(None)
    with pytest.raises(ValueError, match="ClassLoss"):
        eng.set_class_loss({"label_smoothing": 0.1})
    assert eng.class_loss is None
    untouched()

    # the library itself: MARL_EINVAL for a smoothing of 1, and for a setting whose lengths disagree with cfg
    with open(f"{ROOT}/include/marl_hip.h", "r", encoding="utf-8") as f:
        einval = int(re.search(r"#define MARL_EINVAL \((-?\d+)\)", f.read()).group(1))
    lib, cfg, ews = eng.lib, eng.cfg, eng.episode_ws(True)
    w = th.ones(nc + 1, device=device)
    gp, gl, gv, sc, st = poisoned

    def a2c_direct():
        return lib.marl_a2c_loss_fwd_bwd(C.byref(cfg), ews.data_ptr(), _nbytes(ews), out.step_preds.data_ptr(),
                                         out.step_log_probas.data_ptr(), out.step_values.data_ptr(), yd.data_ptr(),
                                         C.c_float(GAMMA), gp.data_ptr(), gl.data_ptr(), gv.data_ptr(), sc.data_ptr(),
                                         st.data_ptr(), 0, _stream(device))

    assert lib.marl_class_loss(None, 0, C.c_float(1.0), None, 0, 0) == einval
    assert eng.plan_query("class_loss") == 0, "a refused setting must not be installed"
    try:
        for args in ((w.data_ptr(), nc + 1, C.c_float(0.0), None, 0, 0), (None, 0, C.c_float(0.1), w.data_ptr(), NS + 1, 0)):
            check(lib.marl_class_loss(*args))
            assert a2c_direct() == einval
            assert b"class-loss" in lib.marl_last_error()
            untouched()
    finally:
        check(lib.marl_class_loss(None, 0, C.c_float(0.0), None, 0, 0))
    for a, b in zip(eng.a2c_loss(out, yd, GAMMA), before):
        assert th.equal(a, b)
