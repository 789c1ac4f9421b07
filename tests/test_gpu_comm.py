"""GPU: communication graphs - a mixing matrix through the fused episode, the step API, the trainers and the
captured graph (``ModelsWrapper.set_comm``, ``marl_comm_matrix``, ``mix_msg_kernel``).

The float64 reference is the oracle's step loop (tests/cases.py::_oracle_loop) with
``marl_oracle.aggregate_messages`` replaced by ``einsum(M64, m)``: ``step_forward`` looks the function up at call
time.  Every comparison with it is teacher-forced (the oracle's actions are passed as ``forced``), so no case
depends on a sampled action.  Tolerances are the project's: outputs 1e-5 absolute (x max(1, |ref|)), gradients 1e-4
of the tensor's scale, Adam update 1e-3 * lr per update (tests/parity.py).  Achieved errors go through its ``Recorder``
(``comm_errors``)."""
import os
import subprocess
import sys

import pytest
import torch as th

from marlclassification_amd import comm
from oracle import marl_oracle as mo
from tests.cases import (NS, TWO_EPOCH, TWO_EPOCH_EPS, CommCase, _a2c_like_loss, _act_loop, _case_with_loss, _dist_loss,
                         _family, _force, _loss_terms, _oracle_loop, _replay, _run, _sampler, _unroll, _unroll_inputs,
                         _y, dense, graph, two_epoch_reference)
from tests.loss_ref import assert_clear_of_bounds
from tests.parity import GRAD_TOL, Recorder
from tests.parity import close as _close

pytestmark = pytest.mark.gpu

REC = Recorder("comm_errors", "comm", _family())  # (a child process of another kernel family keeps a record of its own)
SHAPES = ("g1", "g2", "resisc16")
GRAPHS = ("ring", "star", "none", "teams", "dense")


@pytest.fixture
def oracle_comm(monkeypatch):
    """aggregate_messages of the float64 oracle under a matrix: einsum over the sender index."""
    def use(m):
        m64 = m.double().cpu()
        monkeypatch.setattr(mo, "aggregate_messages", lambda msg: th.einsum("ac,cbk->abk", m64.to(msg.dtype), msg))
    return use


# ---- 1: parity with the float64 oracle ---------------------------------------------------------------------------
def _parity(k, m, device, oracle_comm, tag):
    oracle_comm(m)
    model = k.model(device)
    model.set_comm(m.to(device))
    terms = _loss_terms(k)
    w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    p64 = k.params64()
    img64 = k.img.double().requires_grad_()
    tr = _oracle_loop(k, p64, img64)
    _dist_loss(tr["preds"], tr["logp"], tr["values"], tr["probs"], terms, w).backward()

    sampler = _sampler(k, model, device)
    img = k.img.to(device).requires_grad_()
    ep = sampler.run_episode(img, replay=_replay(sampler, tr["act"], device))
    assert th.equal(ep.step_actions.cpu(), tr["act"]) and th.equal(ep.step_pos.cpu(), tr["pos"])
    for key, got in (("preds", ep.step_preds), ("logp", ep.step_log_probas), ("values", ep.step_values),
                     ("probs", ep.step_probs)):
        REC.fwd(f"{tag}/{key}", got, tr[key])
    _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, terms, w).backward()
    REC.param_grads(f"{tag}/params", model, p64)
    REC.grad(f"{tag}/d_img", img.grad, img64.grad)
    eng = model.hip_engine(k.cfg.actions)
    assert eng.plan_query("comm") == 1
    # (every shape of this file is inside the chained panel launch's range: mixed in the panel by default, by
    # mix_msg_kernel ahead of a plain panel launch with the chain off, ahead of the GEMM path with the panels off)
    assert eng.plan_query("comm_form") == {"panels0": 4, "chain0": 3, "default": 5}[_family()]


@pytest.mark.parametrize("gname", GRAPHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_with_float64_oracle(device, oracle_comm, shape, gname):
    k = CommCase(shape)
    _parity(k, graph(gname, k.na), device, oracle_comm, f"{_family()}/{shape}/{gname}")


@pytest.mark.parametrize("value", [0.0, 0.5])
def test_parity_one_agent(device, oracle_comm, value):
    k = CommCase("na1")
    _parity(k, th.tensor([[value]]), device, oracle_comm, f"{_family()}/na1/{value}")


@pytest.mark.parametrize("env", [{"MARL_PANEL_CHAIN": "0"}, {"MARL_PANELS": "0"}])
def test_parity_in_the_other_kernel_families(device, env):
    """The kernel family is chosen by variables read once per process (the chained panel launch off; the panel
    kernels off = the GEMM + row-kernel path): every parity case again in a child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_comm.py"), "-x", "-q",
                        "-m", "gpu", "-k", "test_parity_with_float64_oracle or test_parity_one_agent", "-s",
                        "-p", "no:cacheprovider"],
                       env=dict(os.environ, **env), cwd=root, capture_output=True, text=True, timeout=1500)
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("[comm]")))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


# ---- 2: the default path is untouched ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g1", "resisc16"])
def test_default_path_is_bit_equal_after_a_matrix_was_set_and_cleared(device, shape):
    k = _case_with_loss(shape)
    fresh = _run(k, k.model(device), device)
    model = k.model(device)
    model.set_comm(dense(k.na).to(device))
    mixed = _run(k, model, device, fresh["act"])
    assert not th.equal(mixed["preds"], fresh["preds"]), "the matrix changed nothing"
    model.set_comm(None)
    assert model.comm is None and model.hip_engine(k.cfg.actions).plan_query("comm") == 0
    again = _run(k, model, device)
    for key, v in fresh.items():
        assert th.equal(v, again[key]), key


# ---- 3: the complete graph through the new path ------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_full_graph_agrees_with_the_default_path(device, shape):
    k = _case_with_loss(shape)
    model = k.model(device)
    ref = _run(k, model, device)
    model.set_comm(comm.full(k.na).to(device))
    got = _run(k, model, device, ref["act"])
    for key in ("preds", "logp", "values", "probs"):
        REC.fwd(f"full/{shape}/{key}", got[key], ref[key])
    for key in ref:
        if key not in ("preds", "logp", "values", "probs", "act"):
            REC.grad(f"full/{shape}/{key}", got[key], ref[key])


# ---- 4: isolation, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g1", "resisc16"])
def test_teams_are_isolated_bit_for_bit(device, shape):
    """teams([k, Na - k]): whatever only team B sees (its initial state and message, its observations / the image
    pixels outside team A's patches) leaves every output row and every initial-state gradient of team A bit-identical."""
    k = _case_with_loss(shape)
    ka = 2
    model = k.model(device)
    model.set_comm(comm.teams([ka, k.na - ka]).to(device))
    # step API: observations, state and carried message of team B replaced
    obs, npos, st0, ws = _unroll_inputs(k)
    outs0, g0 = _unroll(k, model, device, obs, npos, st0, ws)
    model.zero_grad(set_to_none=True)
    obs1 = [o.clone() for o in obs]
    st1 = [s.clone() for s in st0]
    for o in obs1:
        o[ka:] = th.rand(o[ka:].shape, generator=k.gen)
    for s in st1:
        s[ka:] = th.randn(s[ka:].shape, generator=k.gen)
    outs1, g1 = _unroll(k, model, device, obs1, npos, st1, ws)
    model.zero_grad(set_to_none=True)
    changed = False
    for a, b in zip(outs0, outs1):
        for x, y in zip(a, b):
            assert th.equal(x[:ka], y[:ka]), "team A's outputs moved with team B's inputs"
            changed = changed or not th.equal(x[ka:], y[ka:])
    assert changed, "team B's outputs must move"
    for x, y in zip(g0, g1):
        assert th.equal(x[:ka], y[:ka]), "team A's initial-state gradients moved with team B's inputs"
    # fused episode (teacher-forced): the pixels no patch of team A ever covers, and team B's initial state
    base = _run(k, model, device)
    f, pos = k.cfg.window, th.cat([k.inp.pos0[None], base_pos(k, model, device, base["act"])[:-1]])
    seen = th.zeros(k.nb, *k.sizes, dtype=th.bool)
    for t in range(NS):
        for a in range(ka):
            for b in range(k.nb):
                p0, p1 = (int(v) for v in pos[t, a, b])
                seen[b, p0:p0 + f, p1:p1 + f] = True
    k2 = _case_with_loss(shape)
    noise = th.rand(k.img.shape, generator=k.gen)
    k2.img = th.where(seen[:, None].expand_as(k.img), k.img, noise)
    assert not th.equal(k2.img, k.img)
    k2.inp = mo.EpisodeInputs(*([k.inp.pos0] + [th.cat([t[:ka], th.randn(t[ka:].shape, generator=k.gen)])
                                                 for t in (k.inp.h0, k.inp.c0, k.inp.hc0, k.inp.cc0)] + [k.inp.q]))
    k2.terms, k2.w = k.terms, k.w
    moved = _run(k2, model, device, base["act"])
    for key in ("preds", "logp", "values", "probs"):
        assert th.equal(base[key][:, :ka], moved[key][:, :ka]), f"{key}: team A moved"
        assert not th.equal(base[key][:, ka:], moved[key][:, ka:]), f"{key}: team B did not move"


def base_pos(k, model, device, actions):
    sampler = _sampler(k, model, device)
    with th.no_grad():
        return sampler.run_episode(k.img.to(device), replay=_replay(sampler, actions, device)).step_pos.cpu()


def test_no_communication_keeps_a_nan_message_to_its_owner(device):
    from marlclassification_amd.networks.models import RecurrentOutput

    k = CommCase("g1")
    model = k.model(device)
    obs, npos, st0, _ = _unroll_inputs(k)
    st = [t.to(device) for t in st0]
    st[4][1] = float("nan")
    outs = {}
    for name, m in (("none", comm.none(k.na)), ("ring", comm.ring(k.na))):
        model.set_comm(m.to(device))
        with th.no_grad():
            out, rec = model(obs[0].to(device), st[4], npos[0].to(device), RecurrentOutput(*st[:4]))
        outs[name] = (out.actions_probabilities, out.values, out.predictions, out.messages, rec.h, rec.h_caret)
    for x in outs["none"]:
        assert bool(th.isfinite(x).all()), "a message nobody listens to leaked"
    for x in outs["ring"]:  # agents 0 and 2 hear agent 1, the others do not (skipped, not multiplied by 0)
        bad = ~th.isfinite(x).reshape(k.na, -1).all(1)
        assert bad.tolist() == [True, False, True, False, False], bad.tolist()


# ---- 5: the step path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g1", "resisc16"])
def test_act_loop_under_a_matrix_agrees_with_the_fused_node(device, shape):
    k = _case_with_loss(shape)
    model = k.model(device)
    model.set_comm(dense(k.na).to(device))
    sampler = _sampler(k, model, device)
    ep = sampler.run_episode(k.img.to(device))
    _a2c_like_loss(ep.step_preds, ep.step_log_probas, ep.step_values, k.terms).backward()
    g_ep = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    out = _act_loop(k, model, device)
    assert th.equal(out["pos"], ep.step_pos), "the act loop moved otherwise than the episode"
    for key, ref in (("preds", ep.step_preds), ("logp", ep.step_log_probas), ("values", ep.step_values)):
        REC.fwd(f"act_loop/{shape}/{key}", out[key], ref)
    _a2c_like_loss(out["preds"], out["logp"], out["values"], k.terms).backward()
    for n, p in model.named_parameters():
        _close(p.grad, g_ep[n], GRAD_TOL, n)


@pytest.mark.parametrize("shape", SHAPES)
def test_carried_message_gradient_goes_through_the_transpose(device, oracle_comm, shape):
    """ModelsWrapper.forward unrolled under the asymmetric matrix: the gradients of the carried message and the
    initial state against float64 autograd (M in place of M^T would miss by the size of M - M^T)."""
    k = CommCase(shape)
    m = dense(k.na)
    oracle_comm(m)
    model = k.model(device)
    model.set_comm(m.to(device))
    obs, npos, st0, ws = _unroll_inputs(k)
    outs, grads = _unroll(k, model, device, obs, npos, st0, ws)
    p64 = k.params64()
    leaves64 = [t.double().requires_grad_() for t in st0]
    h, cst, hc, cc, msg = leaves64
    loss64 = 0.0
    for t in range(NS):
        so = mo.step_forward(p64, k.cfg, obs[t].double(), msg, npos[t].double(), h, cst, hc, cc)
        h, cst, hc, cc, msg = so.h, so.c, so.hc, so.cc, so.msg
        o = (so.probs, so.values, so.preds, so.msg, so.h, so.c, so.hc, so.cc)
        for j, (g, r) in enumerate(zip(outs[t], o)):
            REC.fwd(f"unroll/{shape}/step{t}/out{j}", g, r)
        loss64 = loss64 + sum((w.double() * x).sum() for w, x in zip(ws[t], o))
    loss64.backward()
    REC.param_grads(f"unroll/{shape}/params", model, p64)
    for n, g, r in zip(("h0", "c0", "hc0", "cc0", "msg0"), grads, leaves64):
        REC.grad(f"unroll/{shape}/d_{n}", g, r.grad)
    # (the test can see a missing transpose: M and M^T differ by far more than the tolerance)
    assert (m - m.t()).abs().max().item() > 0.1


# ---- 6: trainers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g1", "resisc16"])
def test_train_step_with_a_ring_matches_the_float64_adam_update(device, oracle_comm, shape):
    from marlclassification_amd.training import Trainer

    k = CommCase(shape)
    m = comm.ring(k.na)
    oracle_comm(m)
    lr, gamma = 1e-3, 0.99
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    p64 = k.params64()
    tr = _oracle_loop(k, p64, k.img.double())
    lo = mo.a2c_loss(tr["preds"], tr["logp"], tr["values"], y, gamma)
    lo.loss.backward()
    g = {n: (v.grad if v.grad is not None else th.zeros_like(v)) for n, v in p64.items()}
    after = {n: v.detach().clone() for n, v in p64.items()}
    mo.adam_step(after, g, {n: th.zeros_like(v) for n, v in after.items()},
                 {n: th.zeros_like(v) for n, v in after.items()}, 1, lr)

    model = k.model(device)
    model.set_comm(m.to(device))
    sampler = _sampler(k, model, device, probs=False)
    _force(sampler, tr["act"], device)
    trainer = Trainer(model, k.cfg.nb_class, lr, gamma)
    out, scalars = trainer.train_step(k.img, y, sampler)
    assert th.equal(out.step_actions.cpu(), tr["act"])
    REC.fwd(f"train_step/{shape}/preds", out.step_preds, tr["preds"])
    REC.fwd(f"train_step/{shape}/loss", scalars[0], lo.loss)
    REC.updates_match(f"train_step/{shape}/update", k, model, after, [g], lr, 1)


def test_two_ppo_epochs_with_a_matrix_match_the_float64_oracle(device, oracle_comm):
    from marlclassification_amd.training import Trainer

    k = CommCase("g1")
    m = dense(k.na)
    oracle_comm(m)
    eps, lr = TWO_EPOCH_EPS["g1"], TWO_EPOCH["lr"]
    y = _y(k)
    ref = two_epoch_reference(k, y, eps)
    assert_clear_of_bounds(ref["rho"], eps)
    model = k.model(device)
    model.set_comm(m.to(device))
    sampler = _sampler(k, model, device, probs=False)
    _force(sampler, ref["tr"]["act"], device)
    trainer = Trainer(model, k.cfg.nb_class, lr, TWO_EPOCH["gamma"], ppo_epochs=2, ppo_clip=eps,
                      gae_lambda=TWO_EPOCH["lam"], entropy_coef=TWO_EPOCH["beta"])
    trainer.train_epoch([(k.img, y)], 0, sampler)
    assert trainer.curr_step == 1 and model.flat_state().step == 2
    mt = trainer.metrics()
    REC.fwd("ppo/g1/approx_kl", th.tensor(mt["approx_kl"]), ref["scalars2"][5])
    REC.updates_match("ppo/g1/update", k, model, ref["after"], [ref["g1"], ref["g2"]], lr, 2)


def test_graph_replay_equals_eager_under_a_matrix(device):
    """The captured iteration under a matrix: the rollout, the loss and the gradients of the replayed first iteration
    are the eager iteration's bits, and the matrix is part of the graph key."""
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C, draw_episode_device
    from tests.util import Golden, model_spec

    g = Golden("g2_mnist_c1")
    img, y = g.img.to(device), g.y.to(device)
    mats = [comm.ring(g.na).to(device), dense(g.na).to(device)]
    res = {}
    for mode in ("eager", "graph"):
        eng = HipEngine(model_spec(g.cfg), device)
        eng.set_comm(mats[0])
        eng.configure(g.na, g.nb, g.ns, g.img.shape[1:])
        eng.pack({n: v.to(device) for n, v in g.params.items()})
        flat = FlatParams(mo.param_shapes(g.cfg), device)
        flat.load(g.params)
        fa = FusedA2C(eng, flat, 1e-3, g.gamma, use_graph=mode == "graph")
        rows = []
        for it in range(4):
            if it == 2:
                eng.set_comm(mats[1])  # another matrix: the graph must be captured again
            if mode == "graph":
                out, sc = fa.iteration_graph(img, y, 77, it)
            else:
                out, sc = fa.iteration(img, y, draw_episode_device(eng, 77, it))
            th.cuda.synchronize()
            rows.append([t.clone() for t in (out.step_preds, out.step_log_probas, out.step_values, out.step_pos, sc,
                                             flat.grads, flat.params)])
        res[mode] = rows
    names = ("preds", "logp", "values", "pos", "scalars", "grads", "params")
    # iteration 0 runs eagerly in both modes (the capturing call), iteration 1 is the first replay: same parameters
    # going in, so the rollout, the loss and the gradients must be the eager bits.  The parameters coming out may
    # differ in the last bit - a replay computes Adam's bias correction on the device (tests/test_gpu_round2.py) - and
    # with them everything behind: from there on the project's 1e-6 bound of that test applies.
    for it in (0, 1):
        for n, a, b in zip(names, res["eager"][it], res["graph"][it]):
            if n != "params" or it == 0:
                assert th.equal(a, b), f"iteration {it}: {n} differs between eager and replay"
    for it in range(4):
        assert th.equal(res["eager"][it][3], res["graph"][it][3]), f"iteration {it}: positions differ"
        pa, pb = res["eager"][it][6], res["graph"][it][6]
        assert (pa - pb).abs().max().item() <= 1e-6 * pa.abs().max().item()
    # iteration 3 replays the graph captured again under the second matrix (the matrix is part of the key).  Its
    # parameters going in may differ from the eager run's in the last bit (see above), so bits are not comparable;
    # 1e-4 on the predictions separates the two cases that matter: 1-ulp parameter noise moves the predictions by
    # ~1e-6, a stale graph that kept the first matrix moves them by the size of the logits (0.1 and more)
    assert (res["eager"][3][0] - res["graph"][3][0]).abs().max().item() <= 1e-4


# ---- 7: reproducibility ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g1", "resisc16"])
def test_two_runs_give_the_same_bits(device, shape):
    k = _case_with_loss(shape)
    runs = []
    for _ in range(2):
        model = k.model(device)
        model.set_comm(dense(k.na).to(device))
        runs.append(_run(k, model, device))
    for key, v in runs[0].items():
        assert th.equal(v, runs[1][key]), key


def test_two_engines_do_not_see_each_others_matrix(device):
    k = _case_with_loss("g1")
    a, b = k.model(device), k.model(device)
    a.set_comm(dense(k.na).to(device))
    plain = _run(k, b, device)
    ra = _run(k, a, device, plain["act"])
    rb = _run(k, b, device)  # after a call under a's matrix: still the mean
    for key, v in plain.items():
        assert th.equal(v, rb[key]), key
    assert not th.equal(ra["preds"], plain["preds"])


def test_backward_uses_the_matrix_of_its_own_forward(device):
    """An episode node and a step node keep the matrix of their forward: another matrix set before the backward
    (or cleared) does not reach their gradients."""
    k = _case_with_loss("g1")
    model = k.model(device)
    m1, m2 = dense(k.na).to(device), comm.ring(k.na).to(device)
    model.set_comm(m1)
    ref = _run(k, model, device)
    obs, npos, st0, ws = _unroll_inputs(k)
    _, g_ref = _unroll(k, model, device, obs, npos, st0, ws)
    g_ref = [g.clone() for g in g_ref]
    p_ref = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)

    sampler = _sampler(k, model, device)
    img = k.img.to(device).requires_grad_()
    ep = sampler.run_episode(img, replay=_replay(sampler, ref["act"], device))
    loss = _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, k.terms, k.w)
    model.set_comm(m2)
    model.hip_engine(k.cfg.actions)  # (the engine now holds the second matrix)
    loss.backward()
    assert th.equal(img.grad, ref["d_img"])
    for n, p in model.named_parameters():
        assert th.equal(p.grad, ref[n]), n
    model.zero_grad(set_to_none=True)

    from marlclassification_amd.networks.models import RecurrentOutput
    model.set_comm(m1)
    leaves = [t.to(device).requires_grad_() for t in st0]
    rec, msg, total = RecurrentOutput(*leaves[:4]), leaves[4], 0.0
    leaves_engine = model.hip_engine(None)
    for t in range(NS):
        out, rec = model(obs[t].to(device), msg, npos[t].to(device), rec)
        msg = out.messages
        o = (out.actions_probabilities, out.values, out.predictions, out.messages, rec.h, rec.c, rec.h_caret,
             rec.c_caret)
        total = total + sum((w.to(device) * x).sum() for w, x in zip(ws[t], o))
    model.set_comm(None)
    # (ModelsWrapper.forward runs on hip_engine(None) - the step API has no action table - so this IS the engine the
    # step nodes above used: it now holds no matrix)
    assert model.hip_engine(None) is leaves_engine and leaves_engine.comm is None
    total.backward()
    for g, r in zip(leaves, g_ref):
        assert th.equal(g.grad, r)
    for n, p in model.named_parameters():
        assert th.equal(p.grad, p_ref[n]), n


# ---- 8: guards ---------------------------------------------------------------------------------------------------
def test_guards(device):
    import ctypes as C

    from marlclassification_amd import _lib
    from marlclassification_amd.engine import HipEngine
    from tests.util import model_spec

    k = CommCase("g1")
    model = k.model(device)
    for bad in (th.zeros(k.na, k.na + 1), th.zeros(k.na), th.zeros(0, 0)):
        with pytest.raises(ValueError):
            model.set_comm(bad.to(device))
    with pytest.raises(ValueError):
        model.set_comm(comm.ring(k.na))  # a CPU tensor on a device model
    nan = comm.ring(k.na)
    nan[0, 1] = float("inf")
    with pytest.raises(ValueError):
        model.set_comm(nan.to(device))
    with pytest.raises(ValueError):
        model.set_comm(th.zeros(comm.MAX_AGENTS + 1, comm.MAX_AGENTS + 1, device=device))
    assert model.comm is None
    # a matrix of another size than the episode: refused at configure, before anything is enqueued
    model.set_comm(comm.ring(k.na + 1).to(device))
    sampler = _sampler(k, model, device)
    with pytest.raises(ValueError):
        sampler.run_episode(k.img.to(device))
    eng = HipEngine(model_spec(k.cfg), device)
    eng.configure(k.na, k.nb, NS, k.img.shape[1:])
    with pytest.raises(ValueError):
        eng.set_comm(comm.ring(k.na + 1).to(device))
    # the library's own checks
    lib = _lib.load()
    buf = th.zeros(64 * 64, device=device)
    assert lib.marl_comm_matrix(buf.data_ptr(), 0) == -1 and lib.marl_comm_matrix(buf.data_ptr(), 64) == -2
    try:
        assert lib.marl_comm_matrix(buf.data_ptr(), k.na + 1) == 0
        v = C.c_int(0)
        assert lib.marl_plan_query(C.byref(eng.cfg), 1, b"comm", C.byref(v)) == 0 and v.value == 1
        wb, eb = C.c_size_t(0), C.c_size_t(0)
        assert lib.marl_workspace_sizes(C.byref(eng.cfg), 1, C.byref(wb), C.byref(eb)) == 0
        ws = th.zeros(eb.value // 4 + 64, device=device)
        ww = th.zeros(wb.value // 4 + 64, device=device)
        z = th.zeros(1 << 20, device=device)
        rc = lib.marl_episode_backward(C.byref(eng.cfg), ww.data_ptr(), ww.numel() * 4, ws.data_ptr(), ws.numel() * 4,
                                       z.data_ptr(), None, None, None, (C.c_void_p * _lib.MARL_NPARAMS)(), None)
        assert rc == -1 and b"communication matrix" in lib.marl_last_error()
    finally:
        assert lib.marl_comm_matrix(None, 0) == 0
