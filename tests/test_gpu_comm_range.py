"""GPU: range-limited communication - the mixing matrix of the fused episode gated per (step, image) by the agents'
positions (``ModelsWrapper.set_comm_range``, ``marl_comm_range``, the GATE instantiations of the chained panel kernels,
``mix_msg_gated_kernel``).

The float64 reference is the oracle's step loop with ``marl_oracle.aggregate_messages`` replaced, step by step, by
``einsum(w, m)`` with the float64 matrices ``w`` of ``range_matrices64`` below (the builder of THIS file, not the
package's) at the oracle's own positions: step t >= 1 aggregates under the positions at which step t - 1 observed,
step 0 (the zero message) under the initial ones.  The parity, bit-equality and isolation tests run NS = 4 steps, so
three gated exchanges carry a message; the trainer tests keep the NS = 3 helpers and the two-epoch PPO reference of
tests/cases.py.  Every comparison is teacher-forced.  Tolerances are the project's: outputs 1e-5 absolute
(x max(1, |ref|)), gradients 1e-4 of the tensor's scale, Adam update 1e-3 * lr per update.

What a case exercises is asserted from the ORACLE's positions, never from the code under test: in every parity case the
share of in-range ordered pairs a != a' over the gating steps lies in [0.15, 0.85] (Na = 1 has no pair and is
exempt), and a case that claims an empty or a complete receiver row has one (``PARITY`` lists the claims; at least one
case claims each).  Achieved errors go through ``parity.Recorder`` (``comm_range_errors``)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from marlclassification_amd import comm
from oracle import marl_oracle as mo
from tests.cases import NS as NS3
from tests.cases import NS4 as NS
from tests.cases import (TWO_EPOCH, TWO_EPOCH_EPS, CommCase, RangeCase, _case_with_loss, _dist_loss, _family, _force,
                         _grads_of, _oracle_loop, _replay, _run, _run4, _sampler, _y, dense, graph, inputs4,
                         loss_terms4, sampler4, two_epoch_reference)
from tests.loss_ref import assert_clear_of_bounds
from tests.parity import Recorder

pytestmark = pytest.mark.gpu

REC = Recorder("comm_range_errors", "comm_range", _family())
REC_COMM = Recorder("comm_errors", "comm", _family())  # (the trainer tests' updates: tests/test_gpu_comm.py's record)


# ---- the float64 side ----------------------------------------------------------------------------------------------
def range_matrices64(base, pos, radius, metric, normalize):
    """float64 [Nb, Na, Na] for pos [Na, Nb, 2] (integers): w = base * gate, rows rescaled by S_a / s_a."""
    p = pos.to(th.int64).permute(1, 0, 2)                      # [Nb, Na, 2]
    d = (p[:, :, None, :] - p[:, None, :, :]).abs()            # [Nb, receiver, sender, 2]
    gate = d.amax(-1) <= radius if metric == "chebyshev" else (d * d).sum(-1) <= radius * radius
    u = th.where(gate, base.double(), th.zeros((), dtype=th.float64))
    if not normalize:
        return u
    big, small = base.double().sum(-1)[None, :, None], u.sum(-1, keepdim=True)
    return th.where(small > 0, u * (big / th.where(small > 0, small, th.ones_like(small))), th.zeros_like(u))


def pos_dense(na, seed=7):
    """Seeded dense asymmetric non-negative matrix with self-loops."""
    m = th.rand(na, na, generator=th.Generator().manual_seed(seed)) / max(1.0, na ** 0.5) + 0.01
    assert not th.equal(m, m.t()) and (m > 0).all()
    return m


def base_of(name, na):
    if name is None or isinstance(name, th.Tensor):
        return name
    if name == "posdense":
        return pos_dense(na)
    return graph(name, na)  # "ring", and the signed "dense" of tests/cases.py


class GatedOracle:
    """``mo.aggregate_messages`` under a range, driven by the oracle loop itself: ``mo.transition`` is wrapped to
    record the positions, the n-th aggregation of an episode of ``ns`` steps uses the positions step n - 1 observed at
    (n = 0: the initial ones).  ``gates`` keeps the 0/1 gate of every aggregation for the condition asserts."""

    def __init__(self, monkeypatch, k, base, radius, metric, normalize, ns):
        self.base = (comm.full(k.na) if base is None else base).double()
        self.args, self.ns, self.pos0 = (radius, metric, normalize), ns, k.inp.pos0
        self.calls, self.poses, self.gates = 0, [], []
        transition = mo.transition

        def moved(pos, *a, **kw):
            out = transition(pos, *a, **kw)
            self.poses.append(out)
            return out

        def aggregate(msg):
            t = self.calls % self.ns
            if t == 0:
                self.poses = [self.pos0]
                self.gates = []
            self.calls += 1
            pos = self.poses[max(t - 1, 0)]
            self.gates.append(range_matrices64(th.ones(k.na, k.na), pos, self.args[0], self.args[1], False))
            w = range_matrices64(self.base, pos, *self.args).to(msg.dtype)
            return th.einsum("bac,cbk->abk", w, msg)

        monkeypatch.setattr(mo, "transition", moved)
        monkeypatch.setattr(mo, "aggregate_messages", aggregate)

    def stats(self):
        """(share of in-range ordered pairs a != a', an empty receiver row exists, a complete one exists) over the
        aggregations that carry a message (all but the first) of the last episode."""
        g = th.stack(self.gates[1:])                            # [steps, Nb, Na, Na]
        na = g.shape[-1]
        off = g * (1 - th.eye(na, dtype=g.dtype))
        rows = off.sum(-1)
        share = off.sum().item() / max(1, g.shape[0] * g.shape[1] * na * (na - 1))
        return share, bool((rows == 0).any()), bool((rows == na - 1).any())


# tag -> (shape, radius, metric, normalize, base, claims an empty receiver row, claims a complete one)
PARITY = {
    "g1/r6": ("g1", 6, "chebyshev", True, None, True, True),
    "g1/r6/euclid/ring": ("g1", 6, "euclidean", True, "ring", True, False),
    "g1/r6/raw/dense": ("g1", 6, "chebyshev", False, "dense", True, True),
    "g1/r6/posdense": ("g1", 6, "chebyshev", True, "posdense", True, True),
    "g2/r12": ("g2", 12, "chebyshev", True, None, True, True),
    "g2/r12/raw/ring": ("g2", 12, "chebyshev", False, "ring", True, True),
    "resisc16/r12": ("resisc16", 12, "chebyshev", True, None, False, False),
    "resisc16/r24/euclid/posdense": ("resisc16", 24, "euclidean", True, "posdense", False, True),
    "na20/r8/ring": ("na20", 8, "chebyshev", True, "ring", False, False),
}


def _install(model, device, base, radius, metric, normalize):
    model.set_comm(None if base is None else base.to(device))
    model.set_comm_range(radius, metric=metric, normalize=normalize)


# ---- 1: parity with the float64 oracle ---------------------------------------------------------------------------
def oracle_case(monkeypatch, k, spec):
    """The float64 side of a parity case (no device): trajectory, loss, gradients and the condition's statistics."""
    _, radius, metric, normalize, bname, _, _ = spec
    base = base_of(bname, k.na)
    orc = GatedOracle(monkeypatch, k, base, radius, metric, normalize, NS)
    terms = loss_terms4(k)
    w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    p64 = k.params64()
    img64 = k.img.double().requires_grad_()
    tr = _oracle_loop(k, p64, img64, ns=NS)
    _dist_loss(tr["preds"], tr["logp"], tr["values"], tr["probs"], terms, w).backward()
    return base, terms, w, p64, img64, tr, orc.stats()


def _parity(k, spec, device, monkeypatch, tag):
    _, radius, metric, normalize, _, want_empty, want_complete = spec
    base, terms, w, p64, img64, tr, (share, empty, complete) = oracle_case(monkeypatch, k, spec)
    print(f"[comm_range] {tag}: in-range share {share:.3f}, empty row {empty}, complete row {complete}")
    if k.na > 1:
        assert 0.15 <= share <= 0.85, f"{tag}: in-range share {share:.3f} - the case does not exercise the gate"
    assert (not want_empty or empty) and (not want_complete or complete), (tag, empty, complete)

    model = k.model(device)
    _install(model, device, base, radius, metric, normalize)
    sampler = sampler4(k, model, device)
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
    assert eng.plan_query("comm") == 1 and eng.plan_query("comm_range") == radius
    chained = k.na <= 16  # (every shape of this file but na20 is inside the chained panel launch's range)
    assert eng.plan_query("comm_form") == {"panels0": 4, "chain0": 3, "default": 5 if chained else 3}[_family()]
    model.set_comm_range(None)
    assert model.hip_engine(k.cfg.actions).plan_query("comm_range") == -1


def test_the_parity_cases_claim_an_empty_and_a_complete_row():
    assert any(s[5] for s in PARITY.values()) and any(s[6] for s in PARITY.values())
    assert {s[2] for s in PARITY.values() if s[0] == "g1"} == set(comm.METRICS)
    assert {s[3] for s in PARITY.values()} == {True, False}
    assert {s[4] for s in PARITY.values()} == {None, "ring", "dense", "posdense"}
    assert all(s[3] is False for s in PARITY.values() if s[4] == "dense")  # the signed matrix: normalize=False only


@pytest.mark.parametrize("tag", list(PARITY))
def test_parity_with_float64_oracle(device, monkeypatch, tag):
    _parity(RangeCase(PARITY[tag][0]), PARITY[tag], device, monkeypatch, f"{_family()}/{tag}")


@pytest.mark.parametrize("value", [0.0, 0.5])
def test_parity_one_agent(device, monkeypatch, value):
    spec = ("na1", 3, "chebyshev", True, th.tensor([[value]]), False, False)
    _parity(RangeCase("na1"), spec, device, monkeypatch, f"{_family()}/na1/{value}")


# ---- 2: everything in range is the constant matrix, bit for bit ---------------------------------------------------
def _case4(name):
    k = RangeCase(name)
    k.terms = loss_terms4(k)
    k.w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    return k


@pytest.mark.parametrize("shape,bname,normalize", [("g1", "ring", True), ("g1", None, False), ("g2", "posdense", True),
                                                   ("resisc16", None, True), ("na20", "ring", False)])
def test_everything_in_range_is_the_constant_matrix_bit_for_bit(device, shape, bname, normalize):
    k = _case4(shape)
    base = comm.full(k.na) if bname is None else base_of(bname, k.na)
    model = k.model(device)
    model.set_comm(base.to(device))
    ref = _run4(k, model, device)
    _install(model, device, None if bname is None else base, max(k.sizes), "chebyshev", normalize)
    got = _run4(k, model, device, ref["act"])
    for key, v in ref.items():
        assert np.array_equal(v.cpu().numpy(), got[key].cpu().numpy()), f"{_family()}/{shape}: {key} differs"
    model.set_comm_range(0)  # (and the gate does something: nobody in range but co-located agents)
    cut = _run4(k, model, device, ref["act"])
    assert not th.equal(cut["preds"], ref["preds"])


# ---- 3: the other kernel families --------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"MARL_PANEL_CHAIN": "0"}, {"MARL_PANELS": "0"}])
def test_parity_and_bit_equality_in_the_other_kernel_families(device, env):
    """The kernel family is chosen by variables read once per process (the chained panel launch off; the panel
    kernels off = the GEMM + row-kernel path): the parity and the all-in-range cases again in a child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_comm_range.py"), "-x",
                        "-q", "-m", "gpu", "-k", "test_parity_with_float64_oracle or test_parity_one_agent or "
                        "test_everything_in_range or test_out_of_range_nan", "-s", "-p", "no:cacheprovider"],
                       env=dict(os.environ, **env), cwd=root, capture_output=True, text=True, timeout=1500)
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("[comm_range]")))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


# ---- 4: an out-of-range NaN stays with its owner -----------------------------------------------------------------
def loner_setup(k, radius):
    """pos0 and forced actions that keep agent 0 out of everybody's range for the whole episode: agent 0 starts in
    the top-left corner and is sent up (refused at the border: it stays), the others start in the bottom-right part
    and are sent down / right alternately.  Checked on the CPU with the oracle's transition."""
    c = k.cfg
    hi = [s - c.window - 1 for s in k.sizes]
    pos0 = th.stack([th.randint(hi[d] - 3, hi[d] + 1, (k.na, k.nb), generator=k.gen) for d in range(2)], -1)
    pos0[0] = 0
    table = th.tensor(c.actions)
    up = c.actions.index([-1, 0])
    down, right = c.actions.index([1, 0]), c.actions.index([0, 1])
    act = th.empty(NS, k.na, k.nb, dtype=th.int64)
    for t in range(NS):
        act[t] = down if t % 2 == 0 else right
    act[:, 0] = up
    pos, poses = pos0, [pos0]
    for t in range(NS):
        pos = mo.transition(pos, act[t], table, c.window, k.sizes)
        poses.append(pos)
    for p in poses:
        d = (p[1:] - p[:1]).abs().amax(-1)
        assert (d > radius).all(), "the loner came into range"
        assert (p[0] == 0).all()
    return pos0, act


def test_out_of_range_nan_stays_with_its_owner(device):
    k = _case4("g1")
    radius = 6
    pos0, act = loner_setup(k, radius)
    model = k.model(device)
    model.set_comm_range(radius)
    outs = {}
    for name in ("finite", "nan"):
        h0 = k.inp.h0.clone()
        if name == "nan":
            h0[0] = float("nan")
        k.inp = mo.EpisodeInputs(pos0, h0, k.inp.c0, k.inp.hc0, k.inp.cc0, k.inp.q)
        sampler = sampler4(k, model, device)
        with th.no_grad():
            ep = sampler.run_episode(k.img.to(device), replay=_replay(sampler, act, device))
        assert th.equal(ep.step_actions.cpu(), act)
        outs[name] = (ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs)
    for a, b in zip(outs["finite"], outs["nan"]):
        assert bool(th.isfinite(b[:, 1:]).all()), "an out-of-range NaN leaked"
        assert th.equal(a[:, 1:], b[:, 1:]), "the others moved with the loner's state"
    assert not bool(th.isfinite(outs["nan"][0][:, 0]).any()), "the loner's own predictions must be NaN"
    # (in range the same NaN does reach the others: the test can see a leak)
    model.set_comm_range(max(k.sizes))
    sampler = sampler4(k, model, device)
    with th.no_grad():
        ep = sampler.run_episode(k.img.to(device), replay=_replay(sampler, act, device))
    assert not bool(th.isfinite(ep.step_preds[-1, 1:]).all())


# ---- 5: trainers (the NS = 3 helpers of tests/cases.py; the updates are recorded with tests/test_gpu_comm.py's) ----
def test_train_step_matches_the_float64_adam_update(device, monkeypatch):
    from marlclassification_amd.training import Trainer

    k = CommCase("g1")
    base, radius = comm.ring(k.na), 6
    orc = GatedOracle(monkeypatch, k, base, radius, "chebyshev", True, NS3)
    lr, gamma = 1e-3, 0.99
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    p64 = k.params64()
    tr = _oracle_loop(k, p64, k.img.double())
    share = orc.stats()[0]
    assert 0.15 <= share <= 0.85, share
    lo = mo.a2c_loss(tr["preds"], tr["logp"], tr["values"], y, gamma)
    lo.loss.backward()
    g = _grads_of(p64)
    after = {n: v.detach().clone() for n, v in p64.items()}
    mo.adam_step(after, g, {n: th.zeros_like(v) for n, v in after.items()},
                 {n: th.zeros_like(v) for n, v in after.items()}, 1, lr)

    model = k.model(device)
    _install(model, device, base, radius, "chebyshev", True)
    sampler = _sampler(k, model, device, probs=False)
    _force(sampler, tr["act"], device)
    trainer = Trainer(model, k.cfg.nb_class, lr, gamma)
    out, scalars = trainer.train_step(k.img, y, sampler)
    assert th.equal(out.step_actions.cpu(), tr["act"])
    REC.fwd("train_step/g1/preds", out.step_preds, tr["preds"])
    REC.fwd("train_step/g1/loss", scalars[0], lo.loss)
    REC_COMM.updates_match("train_step/g1/update", k, model, after, [g], lr, 1)


def test_two_ppo_epochs_match_the_float64_oracle(device, monkeypatch):
    from marlclassification_amd.training import Trainer

    k = CommCase("g1")
    # (chebyshev: under the euclidean gate one float64 ratio of this case lies 4.5e-5 from the clip bound, inside the
    # margin assert_clear_of_bounds keeps for fp32 - a property of the reference, found on the CPU)
    base, radius, metric = pos_dense(k.na), 6, "chebyshev"
    orc = GatedOracle(monkeypatch, k, base, radius, metric, True, NS3)
    eps, lr = TWO_EPOCH_EPS["g1"], TWO_EPOCH["lr"]
    y = _y(k)
    ref = two_epoch_reference(k, y, eps)
    assert_clear_of_bounds(ref["rho"], eps)
    assert 0.15 <= orc.stats()[0] <= 0.85
    model = k.model(device)
    _install(model, device, base, radius, metric, True)
    sampler = _sampler(k, model, device, probs=False)
    _force(sampler, ref["tr"]["act"], device)
    trainer = Trainer(model, k.cfg.nb_class, lr, TWO_EPOCH["gamma"], ppo_epochs=2, ppo_clip=eps,
                      gae_lambda=TWO_EPOCH["lam"], entropy_coef=TWO_EPOCH["beta"])
    trainer.train_epoch([(k.img, y)], 0, sampler)
    assert trainer.curr_step == 1 and model.flat_state().step == 2
    REC.fwd("ppo/g1/approx_kl", th.tensor(trainer.metrics()["approx_kl"]), ref["scalars2"][5])
    REC_COMM.updates_match("ppo/g1/update", k, model, ref["after"], [ref["g1"], ref["g2"]], lr, 2)


# ---- 6: graph replay and reproducibility ---------------------------------------------------------------------------
def test_graph_replay_equals_eager_under_a_range(device):
    """The captured iteration under a range: the replayed first iteration has the eager iteration's bits, and the
    range is part of the graph key."""
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C, draw_episode_device
    from tests.util import Golden, model_spec

    g = Golden("g2_mnist_c1")
    img, y = g.img.to(device), g.y.to(device)
    res = {}
    for mode in ("eager", "graph"):
        eng = HipEngine(model_spec(g.cfg), device)
        eng.set_comm_range(10)
        eng.configure(g.na, g.nb, g.ns, g.img.shape[1:])
        eng.pack({n: v.to(device) for n, v in g.params.items()})
        flat = FlatParams(mo.param_shapes(g.cfg), device)
        flat.load(g.params)
        fa = FusedA2C(eng, flat, 1e-3, g.gamma, use_graph=mode == "graph")
        rows = []
        for it in range(4):
            if it == 2:
                eng.set_comm_range(3, metric="euclidean")  # another range: the graph must be captured again
            if mode == "graph":
                out, sc = fa.iteration_graph(img, y, 77, it)
            else:
                out, sc = fa.iteration(img, y, draw_episode_device(eng, 77, it))
            th.cuda.synchronize()
            rows.append([t.clone() for t in (out.step_preds, out.step_log_probas, out.step_values, out.step_pos, sc,
                                             flat.grads, flat.params)])
        res[mode] = rows
    names = ("preds", "logp", "values", "pos", "scalars", "grads", "params")
    # (as tests/test_gpu_comm.py: iteration 0 is the eager capturing call, iteration 1 the first replay; the parameters
    # coming out of a replay may differ in the last bit - Adam's bias correction is computed on the device)
    for it in (0, 1):
        for n, a, b in zip(names, res["eager"][it], res["graph"][it]):
            if n != "params" or it == 0:
                assert th.equal(a, b), f"iteration {it}: {n} differs between eager and replay"
    for it in range(4):
        pa, pb = res["eager"][it][6], res["graph"][it][6]
        assert (pa - pb).abs().max().item() <= 1e-6 * pa.abs().max().item()
    # iteration 3 replays the graph captured again under the second range: a stale graph that kept the first one
    # moves the predictions by the size of the logits, 1-ulp parameter noise by ~1e-6
    assert (res["eager"][3][0] - res["graph"][3][0]).abs().max().item() <= 1e-4
    assert not th.equal(res["eager"][3][0], res["eager"][1][0])


def _case3(name, radius=6):
    k = _case_with_loss(name)
    k.radius = radius
    return k


def test_two_free_running_runs_give_the_same_bits(device):
    k = _case3("g1")
    runs = []
    for _ in range(2):
        model = k.model(device)
        _install(model, device, pos_dense(k.na), k.radius, "chebyshev", True)
        runs.append(_run(k, model, device))
    for key, v in runs[0].items():
        assert th.equal(v, runs[1][key]), key


def test_two_engines_do_not_see_each_others_range(device):
    k = _case3("g1")
    a, b = k.model(device), k.model(device)
    a.set_comm_range(k.radius)
    plain = _run(k, b, device)
    ra = _run(k, a, device, plain["act"])
    rb = _run(k, b, device)  # after a call under a's range: still the mean
    for key, v in plain.items():
        assert th.equal(v, rb[key]), key
    assert not th.equal(ra["preds"], plain["preds"])
    assert b.hip_engine(k.cfg.actions).plan_query("comm_range") == -1
    assert a.hip_engine(k.cfg.actions).plan_query("comm_range") == k.radius


def test_backward_uses_the_range_of_its_own_forward(device):
    k = _case3("g1")
    model = k.model(device)
    model.set_comm_range(k.radius)
    ref = _run(k, model, device)
    sampler = _sampler(k, model, device)
    img = k.img.to(device).requires_grad_()
    ep = sampler.run_episode(img, replay=_replay(sampler, ref["act"], device))
    loss = _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, k.terms, k.w)
    model.set_comm_range(1, metric="euclidean", normalize=False)
    assert model.hip_engine(k.cfg.actions).comm_range == comm.CommRange(1, "euclidean", False)
    loss.backward()
    assert th.equal(img.grad, ref["d_img"])
    for n, p in model.named_parameters():
        assert th.equal(p.grad, ref[n]), n
    model.zero_grad(set_to_none=True)
    # (and cleared in between: the backward still gates)
    img2 = k.img.to(device).requires_grad_()
    model.set_comm_range(k.radius)
    ep = sampler.run_episode(img2, replay=_replay(sampler, ref["act"], device))
    loss = _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, k.terms, k.w)
    model.set_comm_range(None)
    model.hip_engine(k.cfg.actions)
    loss.backward()
    assert th.equal(img2.grad, ref["d_img"])
    assert model.hip_engine(k.cfg.actions).comm_range is None


# ---- 7: guards ---------------------------------------------------------------------------------------------------
def test_guards(device):
    import ctypes as C

    from marlclassification_amd import _lib
    from marlclassification_amd.core import MultiAgent
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.networks.models import RecurrentOutput
    from tests.util import model_spec

    k = CommCase("g1")
    model = k.model(device)
    model.set_comm_range(6)
    # the step API: the model's surface names the fused episode, the engine's call is refused by the library
    obs = mo.crop_patches(k.img, k.inp.pos0, k.cfg.window).to(device)
    npos = mo.normalized_positions(k.inp.pos0, k.sizes).to(device)
    st = [t.to(device) for t in (k.inp.h0, k.inp.c0, k.inp.hc0, k.inp.cc0)]
    msg = th.zeros(k.na, k.nb, k.cfg.n_m, device=device)
    with pytest.raises(RuntimeError, match="fused episode"):
        model(obs, msg, npos, RecurrentOutput(*st))
    with pytest.raises(RuntimeError, match="fused episode"):
        MultiAgent(k.na, model).act(obs, npos)
    eng = HipEngine(model_spec(k.cfg), device)
    eng.configure(k.na, k.nb, 1, (obs.shape[2], obs.shape[3] + 1, obs.shape[4] + 1))  # (ModelsWrapper.forward's)
    eng.pack({n: v.to(device) for n, v in k.params.items()})
    ws = eng.train_ws_acquire()
    eng.step_forward(obs, msg, npos, *st, ws=ws)  # (fine without a range)
    eng.set_comm_range(6)
    with pytest.raises(Exception, match="communication range"):
        eng.step_forward(obs, msg, npos, *st)
    with pytest.raises(Exception, match="communication range"):
        eng.step_forward(obs, msg, npos, *st, ws=ws)
    with pytest.raises(Exception, match="communication range"):
        eng.step_backward(ws, obs, {n: th.empty(v.shape, device=device) for n, v in k.params.items()})
    eng.set_comm_range(None)
    eng.configure(k.na, k.nb, NS3, k.img.shape[1:])

    # d_comm: no gradient of a gated base
    eng.set_comm(comm.ring(k.na).to(device))
    eng.set_comm_range(6)
    with pytest.raises(ValueError, match="communication range"):
        eng.episode_backward(None, None, None, {}, d_comm=th.zeros(k.na, k.na, device=device))
    lib = _lib.load()
    buf = comm.ring(k.na).to(device)
    z = th.zeros(1 << 16, device=device)
    try:
        assert lib.marl_comm_matrix(buf.data_ptr(), k.na) == 0 and lib.marl_comm_range(6, 0, 1) == 0
        rc = lib.marl_comm_grad(C.byref(eng.cfg), z.data_ptr(), 4, z.data_ptr(), 4, 1, z.data_ptr(), z.data_ptr(), 4,
                                None)
        assert rc == -1 and b"communication range" in lib.marl_last_error()
        v = C.c_int(0)
        assert lib.marl_plan_query(C.byref(eng.cfg), 1, b"comm_range", C.byref(v)) == 0 and v.value == 6
        # a range without its base matrix: refused by every entry that builds a context
        assert lib.marl_comm_matrix(None, 0) == 0
        rc = lib.marl_episode_backward(C.byref(eng.cfg), z.data_ptr(), z.numel() * 4, z.data_ptr(), z.numel() * 4,
                                       z.data_ptr(), None, None, None, (C.c_void_p * _lib.MARL_NPARAMS)(), None)
        assert rc == -1 and b"base matrix" in lib.marl_last_error()
        # a bad metric; a negative radius clears
        assert lib.marl_comm_range(6, 2, 1) == -1 and lib.marl_comm_range(6, -1, 1) == -1
        assert lib.marl_comm_range(-1, 7, 1) == 0
        assert lib.marl_plan_query(C.byref(eng.cfg), 1, b"comm_range", C.byref(v)) == 0 and v.value == -1
    finally:
        assert lib.marl_comm_matrix(None, 0) == 0 and lib.marl_comm_range(-1, 0, 1) == 0
    eng.set_comm_range(None)
    eng.set_comm(None)

    # a live source, in both orders; a negative base under normalize=True, in both orders; bad radius / metric
    live = comm.LearnableComm(comm.ring(k.na)).to(device)
    for target in (model, eng):
        target.set_comm(None)
        target.set_comm_range(6)
        with pytest.raises(ValueError, match="live"):
            target.set_comm(live)
        target.set_comm_range(None)
        target.set_comm(live)
        with pytest.raises(ValueError, match="live"):
            target.set_comm_range(6)
        target.set_comm(dense(k.na).to(device))
        with pytest.raises(ValueError, match=">= 0"):
            target.set_comm_range(6)
        target.set_comm_range(6, normalize=False)
        target.set_comm(None)
        target.set_comm_range(6)
        with pytest.raises(ValueError, match=">= 0"):
            target.set_comm(dense(k.na).to(device))
        for bad in (-1, 2.5, "6"):
            with pytest.raises(ValueError, match="radius"):
                target.set_comm_range(bad)
        with pytest.raises(ValueError, match="metric"):
            target.set_comm_range(6, metric="manhattan")
        target.set_comm_range(None)

    # more agents than the mixing kernel serves: refused before anything is enqueued
    big = RangeCase.__new__(RangeCase)
    big.cfg, big.na, big.nb = k.cfg, comm.MAX_AGENTS + 1, 2
    big.params, big.img, big.sizes, big.gen = k.params, k.img[:2], k.sizes, k.gen
    inputs4(big, 3)
    wide = big.model(device)
    wide.set_comm_range(6)
    with pytest.raises(ValueError, match="at most"):
        sampler4(big, wide, device).run_episode(big.img.to(device))
    wide.set_comm_range(None)
    sampler4(big, wide, device).run_episode(big.img.to(device))  # (the mean serves any number of agents)
