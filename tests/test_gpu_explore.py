"""GPU: exploration controls of the fused sampling - a temperature, an eps-soft mixture and greedy acting
(``ModelsWrapper.set_exploration``, ``marl_policy_explore``, the EXPLORE instantiations of ``sample_kernel`` and of the
chained panel kernel's sampling epilogue, ``policy_dlogits_explore_kernel``).

The float64 side is the step loop ``explore_loop4`` of THIS file (modelled on tests/cases.py::_oracle_loop, four steps):
it maps the oracle's ``so.probs`` to the behaviour policy ``behaviour64`` - softmax(log p / tau) mixed with the uniform
distribution - and takes ``argmax(pi_b / q)`` or, greedy, ``argmax(pi_b)``.  The free-running cases compare actions and
positions bit for bit; their condition is asserted from the ORACLE, never from the code under test: every decision's
top-two score ratio is >= 1 + 1e-4, and no decision is left out.  The trainer tests reuse the float64 helpers of
tests/cases.py (teacher forcing, the two-epoch PPO reference) with ``mo.step_forward`` wrapped by the same map
(``oracle_explore``).
Tolerances are the project's: outputs 1e-5 x max(1, |ref|), gradients 1e-4 of the tensor's scale, Adam 1e-3 * lr per
update (tests/parity.py).  Achieved errors and margins go through its ``Recorder`` (``explore_errors``)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

from oracle import marl_oracle as mo
from tests import util
from tests.cases import NS4 as NS
from tests.cases import (POL_BIAS, TWO_EPOCH, TWO_EPOCH_EPS, Case, RangeCase, _a2c_like_loss, _act_loop, _dist_loss,
                         _force, _grads_of, _loss_terms, _oracle_loop, _replay, _run4, _sampler, _y, inputs4,
                         loss_terms4, sampler4, two_epoch_reference)
from tests.loss_ref import assert_clear_of_bounds
from tests.parity import GRAD_TOL, Recorder
from tests.parity import close as _close

pytestmark = pytest.mark.gpu

MARGIN = 1.0 + 1e-4
POL_WEIGHT = "_ModelsWrapper__policy.3.weight"

# (tau, eps, greedy)
SETTINGS = [(1.0, 0.0, True), (0.5, 0.0, False), (2.0, 0.1, False), (1.0, 0.25, False), (0.25, 0.0, True)]
GRAD_SETTINGS = [(2.0, 0.1), (0.5, 0.25)]
SHAPES = ("g1", "g2", "resisc16", "na20")
# five actions (the G3 configuration with the stay move): the MARL_MAX_ACTIONS instantiations, the scalar backward rows
FIVE = {"g3stay": (util.CASES["g3_mnist_ckpt"], 3, 4, (1, 28, 28), 31)}
# where the forward loop samples by default: 1 = the chained launch's epilogue, 2 = sample_kernel (past the chain's 16
# rows, or more than four actions)
FORM = {"g1": 1, "g2": 1, "resisc16": 1, "na20": 2, "g3stay": 2}


def _family():
    for var, name in (("MARL_PANELS", "panels0"), ("MARL_PANEL_CHAIN", "chain0"), ("MARL_PANEL_SAMPLE", "sample0")):
        if os.environ.get(var) == "0":
            return name
    return "default"


class ExploreCase(RangeCase):
    def __init__(self, name):
        if name in FIVE:
            self.cfg, self.na, self.nb, shape, seed = FIVE[name]
            self.params = util.uniform_params(self.cfg, seed)
            self.img = th.rand(self.nb, *shape, generator=th.Generator().manual_seed(seed))
            self.gen = th.Generator().manual_seed(seed + 1000)
            self.sizes = list(self.img.shape[2:])
            inputs4(self, seed)
        else:
            super().__init__(name)
        self.name = name


# ---- the float64 side ----------------------------------------------------------------------------------------------
def behaviour64(p, tau, eps):
    """pi_b = (1 - eps) softmax(log p / tau) + eps / nA in the dtype of p (zeros stay zeros before the mixture)."""
    s = th.softmax(th.log(p) / tau, dim=-1)
    return (1.0 - eps) * s + eps / p.shape[-1]


def explore_loop4(k, p64, img64, tau, eps, greedy, forced=None, ns=NS):
    """The episode in float64 under exploration controls; also the smallest top-two score ratio over the decisions."""
    c, i = k.cfg, k.inp
    table = th.tensor(c.actions)
    pos = i.pos0
    h, cst, hc, cc = (t.double() for t in (i.h0, i.c0, i.hc0, i.cc0))
    msg = th.zeros(k.na, k.nb, c.n_m, dtype=th.float64)
    acc = {"preds": [], "logp": [], "values": [], "pos": [], "probs": [], "act": []}
    ratio, decisions = math.inf, 0
    for t in range(ns):
        so = mo.step_forward(p64, c, mo.crop_patches(img64, pos, c.window), msg,
                             mo.normalized_positions(pos, k.sizes).double(), h, cst, hc, cc)
        h, cst, hc, cc, msg = so.h, so.c, so.hc, so.cc, so.msg
        pib = behaviour64(so.probs, tau, eps)
        score = pib.detach() if greedy else pib.detach() / i.q[t].double()
        top = score.topk(2, dim=-1).values
        ratio = min(ratio, (top[..., 0] / top[..., 1]).min().item())
        decisions += score[..., 0].numel()
        a = th.argmax(score, dim=-1) if forced is None else forced[t]
        logp = th.gather(pib, -1, a.unsqueeze(-1)).squeeze(-1).log()
        pos = mo.transition(pos, a, table, c.window, k.sizes)
        for key, v in zip(acc, (so.preds, logp, so.values, pos, pib, a)):
            acc[key].append(v)
    out = {key: th.stack(v) for key, v in acc.items()}
    out["ratio"], out["decisions"] = ratio, decisions
    return out


@pytest.fixture
def oracle_explore(monkeypatch):
    """Every float64 loop that goes through ``mo.step_forward`` / ``mo.sample_actions`` under a setting."""
    def use(tau, eps, greedy=False):
        step = mo.step_forward

        def wrapped(*a, **kw):
            so = step(*a, **kw)
            so.probs = behaviour64(so.probs, tau, eps)
            return so
        monkeypatch.setattr(mo, "step_forward", wrapped)
        if greedy:
            monkeypatch.setattr(mo, "sample_actions", lambda probs, q: th.argmax(probs, dim=-1))
    return use


REC = Recorder("explore_errors", "explore", _family())  # (a child process of another family keeps its own record)


def _tag(shape, tau, eps, greedy=False):
    return f"{_family()}/{shape}/t{tau:g}_e{eps:g}" + ("_greedy" if greedy else "")


def _expect_form(shape):
    return FORM[shape] if _family() == "default" else 2


# ---- 1: free-running parity ----------------------------------------------------------------------------------------
def _free_running(k, device, tau, eps, greedy):
    tag = _tag(k.name, tau, eps, greedy)
    tr = explore_loop4(k, {n: v.double() for n, v in k.params.items()}, k.img.double(), tau, eps, greedy)
    print(f"[explore] {tag}: min top-two score ratio {tr['ratio']:.6f} over {tr['decisions']} decisions")
    REC.put(f"{tag}/margin", {"min_top_two_ratio": tr["ratio"], "decisions": tr["decisions"]})
    assert tr["decisions"] == NS * k.na * k.nb, "a decision was left out"
    assert tr["ratio"] >= MARGIN, f"{tag}: top-two ratio {tr['ratio']:.7f}: fp32 could decide otherwise"
    model = k.model(device)
    model.set_exploration(tau, eps, greedy)
    assert model.exploration == (tau, eps, greedy)
    sampler = sampler4(k, model, device)
    with th.no_grad():
        ep = sampler.run_episode(k.img.to(device))
    assert th.equal(ep.step_actions.cpu(), tr["act"]), f"{tag}: actions differ from the float64 loop"
    assert th.equal(ep.step_pos.cpu(), tr["pos"]), f"{tag}: positions differ from the float64 loop"
    for key, got in (("probs", ep.step_probs), ("logp", ep.step_log_probas), ("values", ep.step_values),
                     ("preds", ep.step_preds)):
        REC.fwd(f"{tag}/{key}", got, tr[key])
    eng = model.hip_engine(k.cfg.actions)
    assert eng.plan_query("explore") == 1 and eng.plan_query("explore_form") == _expect_form(k.name)
    return tr


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: f"t{s[0]:g}_e{s[1]:g}" + ("_greedy" if s[2] else ""))
@pytest.mark.parametrize("shape", SHAPES)
def test_free_running_parity(device, shape, setting):
    _free_running(ExploreCase(shape), device, *setting)


@pytest.mark.parametrize("setting", [(2.0, 0.1, False), (0.25, 0.0, True)], ids=["t2_e0.1", "t0.25_greedy"])
def test_free_running_parity_five_actions(device, setting):
    k = ExploreCase("g3stay")
    assert k.cfg.nb_action == 5
    tr = _free_running(k, device, *setting)
    assert (tr["act"] == 4).any(), "the stay move never acts: the fifth action is not covered"


def test_the_settings_act_differently():
    """The free-running cases are not vacuous: on one shape the settings give action histories of their own (the two
    greedy ones the same: the argmax does not depend on the temperature)."""
    k = ExploreCase("g1")
    p64 = {n: v.double() for n, v in k.params.items()}
    acts = [explore_loop4(k, p64, k.img.double(), *s)["act"] for s in SETTINGS]
    plain = explore_loop4(k, p64, k.img.double(), 1.0, 0.0, False)["act"]
    assert all(not th.equal(a, plain) for a in acts)
    assert th.equal(acts[0], acts[4]) and SETTINGS[0][2] and SETTINGS[4][2]
    assert len({tuple(a.flatten().tolist()) for a in acts}) == len(SETTINGS) - 1


# ---- 2: teacher-forced gradient parity -----------------------------------------------------------------------------
def _gradients(k, device, tau, eps):
    tag = _tag(k.name, tau, eps) + "/forced"
    terms = loss_terms4(k)
    w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    p64 = k.params64()
    img64 = k.img.double().requires_grad_()
    tr = explore_loop4(k, p64, img64, tau, eps, False)
    _dist_loss(tr["preds"], tr["logp"], tr["values"], tr["probs"], terms, w).backward()
    model = k.model(device)
    model.set_exploration(tau, eps)
    sampler = sampler4(k, model, device)
    img = k.img.to(device).requires_grad_()
    ep = sampler.run_episode(img, replay=_replay(sampler, tr["act"], device))
    assert th.equal(ep.step_actions.cpu(), tr["act"]) and th.equal(ep.step_pos.cpu(), tr["pos"])
    for key, got in (("probs", ep.step_probs), ("logp", ep.step_log_probas), ("values", ep.step_values),
                     ("preds", ep.step_preds)):
        REC.fwd(f"{tag}/{key}", got, tr[key])
    _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, terms, w).backward()
    REC.param_grads(f"{tag}/params", model, p64)
    REC.grad(f"{tag}/d_img", img.grad, img64.grad)
    assert model.hip_engine(k.cfg.actions).plan_query("explore_form") == _expect_form(k.name)


@pytest.mark.parametrize("setting", GRAD_SETTINGS, ids=lambda s: f"t{s[0]:g}_e{s[1]:g}")
@pytest.mark.parametrize("shape", SHAPES + ("g3stay",))
def test_teacher_forced_gradient_parity(device, shape, setting):
    _gradients(ExploreCase(shape), device, *setting)


# ---- 3: the other kernel families ----------------------------------------------------------------------------------
FAMILY_SHAPE = {"panels0": "g2", "chain0": "g1", "sample0": "resisc16", "default": "g1"}


def test_family_free_running(device):
    """(run by the child processes of test_other_kernel_families: the shape of this process's kernel family)"""
    k = ExploreCase(FAMILY_SHAPE[_family()])
    for setting in ((2.0, 0.1, False), (0.25, 0.0, True)):
        _free_running(k, device, *setting)


def test_family_gradients(device):
    _gradients(ExploreCase(FAMILY_SHAPE[_family()]), device, 2.0, 0.1)


@pytest.mark.parametrize("env", [{"MARL_PANEL_CHAIN": "0"}, {"MARL_PANELS": "0"}, {"MARL_PANEL_SAMPLE": "0"}],
                         ids=["chain0", "panels0", "sample0"])
def test_other_kernel_families(device, env):
    """The kernel family is chosen by variables read once per process: the free-running and the gradient case of one
    shape each in a child process; ``explore_form`` is asserted there (2: sample_kernel in every one of them)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_explore.py"), "-x", "-q",
                        "-m", "gpu", "-k", "test_family_", "-s", "-p", "no:cacheprovider"],
                       env=dict(os.environ, **env), cwd=root, capture_output=True, text=True, timeout=600)
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("[explore]")))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


# ---- 4: the defaults are today's path ------------------------------------------------------------------------------
def _case4(name):
    k = ExploreCase(name)
    k.terms = loss_terms4(k)
    k.w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    return k


def _all_same_bits(a, b, what):
    for key, v in a.items():
        assert np.array_equal(v.cpu().numpy(), b[key].cpu().numpy()), f"{what}: {key} differs"


@pytest.mark.parametrize("shape", ["g1", "resisc16", "g3stay"])
def test_defaults_are_todays_path(device, monkeypatch, shape):
    from marlclassification_amd import _lib

    k = _case4(shape)
    calls = []
    lib = _lib.load()
    real = lib.marl_policy_explore
    monkeypatch.setattr(lib, "marl_policy_explore", lambda *a: calls.append(a) or real(*a))
    never = _run4(k, k.model(device), device)
    model = k.model(device)
    model.set_exploration(1, 0, False)
    again = _run4(k, model, device)
    _all_same_bits(never, again, f"{shape}: set_exploration(1, 0, False)")
    eng = model.hip_engine(k.cfg.actions)
    assert eng.plan_query("explore") == 0 and eng.plan_query("explore_form") == 0
    assert calls == [], f"marl_policy_explore was called at the defaults: {calls}"
    # ... and after a setting was installed and cleared
    model.set_exploration(2.0, 0.1)
    other = _run4(k, model, device)
    assert not th.equal(other["probs"], never["probs"]), "the setting changed nothing"
    assert calls and all(c == (1.0, 0.0, 0) for c in calls[1::2]), "every install is cleared behind its call"
    model.set_exploration()
    _all_same_bits(never, _run4(k, model, device), f"{shape}: after a setting was cleared")


# ---- 5: greedy -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g1", "na20", "g3stay"])
def test_greedy_is_the_existing_path_with_noise_of_ones(device, shape):
    from marlclassification_amd.fused import EpisodeDraws

    k = _case4(shape)
    i = k.inp
    ones = EpisodeDraws(*(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0, th.ones_like(i.q[:NS]))))
    ref = _run4(k, k.model(device), device, draws=ones)
    model = k.model(device)
    model.set_exploration(greedy=True)
    got = _run4(k, model, device)  # (the case's random noise is injected - and must not be read)
    _all_same_bits(ref, got, f"{shape}: greedy at tau 1, eps 0")


def test_two_greedy_runs_under_different_seeds_are_identical(device):
    from marlclassification_amd.fused import EpisodeDraws

    k = _case4("g1")
    i = k.inp
    runs = {}
    for greedy in (False, True):
        for seed in (1, 2):  # (the generator's key: the sampling kernel draws its own variates)
            model = k.model(device)
            model.set_exploration(greedy=greedy)
            draws = EpisodeDraws(*(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0)), None, (seed, 0))
            th.manual_seed(seed)
            runs[greedy, seed] = _run4(k, model, device, draws=draws)
    _all_same_bits(runs[True, 1], runs[True, 2], "greedy under two seeds")
    assert not th.equal(runs[False, 1]["act"], runs[False, 2]["act"]), "the sampled runs do not depend on the seed"


@pytest.mark.parametrize("setting", [(1.0, 0.0), (2.0, 0.25)])
@pytest.mark.parametrize("shape", ["g1", "g3stay"])
def test_greedy_takes_the_lowest_index_on_a_tie(device, shape, setting):
    k = ExploreCase(shape)
    k.params = dict(k.params)
    k.params[POL_WEIGHT] = th.zeros_like(k.params[POL_WEIGHT])
    k.params[POL_BIAS] = th.zeros_like(k.params[POL_BIAS])
    model = k.model(device)
    model.set_exploration(*setting, greedy=True)
    with th.no_grad():
        ep = sampler4(k, model, device).run_episode(k.img.to(device))
    nA = k.cfg.nb_action
    assert th.equal(ep.step_probs, th.full_like(ep.step_probs, 1.0 / nA)) or setting[1] > 0
    assert (ep.step_probs - 1.0 / nA).abs().max().item() <= 1e-6
    assert (ep.step_actions == 0).all(), "a tie did not go to the lowest index"


# ---- 6: floors and collapse ----------------------------------------------------------------------------------------
def _one_hot_case(shape):
    """The policy's output layer gives the logits (200, 0, 0, ...): softmax is exactly one-hot in fp32."""
    k = _case4(shape)
    k.params = dict(k.params)
    k.params[POL_WEIGHT] = th.zeros_like(k.params[POL_WEIGHT])
    b = th.zeros_like(k.params[POL_BIAS])
    b[0] = 200.0
    k.params[POL_BIAS] = b
    return k


@pytest.mark.parametrize("shape", ["g1", "g3stay"])
def test_eps_floor_keeps_a_forced_excluded_action_finite(device, shape):
    k = _one_hot_case(shape)
    nA = k.cfg.nb_action
    model = k.model(device)
    model.set_exploration(eps=0.1)
    forced = th.ones(NS, k.na, k.nb, dtype=th.int64)  # an action whose softmax probability is exactly 0
    res = _run4(k, model, device, actions=forced)
    assert th.equal(res["act"].cpu(), forced)
    floor = (th.tensor(0.1, dtype=th.float32) / nA).item()  # (eps / nA as the host forms it: in fp32)
    assert (res["probs"][..., 1:] == floor).all(), "the excluded actions' softmax is not exactly 0"
    REC.fwd(f"floor/{shape}/logp", res["logp"], th.full(res["logp"].shape, math.log(0.1 / nA), dtype=th.float64))
    for key in ("d_img", "flat_grad", "preds", "values"):
        assert th.isfinite(res[key]).all(), key


@pytest.mark.parametrize("shape", ["g1", "g3stay"])
def test_a_tiny_temperature_collapses_to_an_exact_one_hot(device, shape):
    k = _one_hot_case(shape)
    k.params[POL_BIAS] = k.params[POL_BIAS] / 100.0  # logits (2, 0, ...): tau = 0.01 restores the gap of 200
    model = k.model(device)
    model.set_exploration(temperature=0.01)
    res = _run4(k, model, device)
    hot = th.zeros_like(res["probs"])
    hot[..., 0] = 1.0
    assert th.equal(res["probs"], hot) and (res["act"] == 0).all()
    assert (res["logp"] == 0).all()
    for key, v in res.items():
        assert not th.isnan(v.double()).any(), key


# ---- 7: steps ------------------------------------------------------------------------------------------------------
def _case3(name):
    k = Case(name)
    k.name = name
    k.terms = _loss_terms(k)
    return k


@pytest.mark.parametrize("setting", [(2.0, 0.1, False), (0.5, 0.0, True)], ids=["t2_e0.1", "t0.5_greedy"])
@pytest.mark.parametrize("shape", ["g1", "wide"])
def test_act_loop_under_a_setting_agrees_with_the_fused_episode(device, shape, setting):
    k = _case3(shape)
    model = k.model(device)
    model.set_exploration(*setting)
    sampler = _sampler(k, model, device)
    ep = sampler.run_episode(k.img.to(device))
    _a2c_like_loss(ep.step_preds, ep.step_log_probas, ep.step_values, k.terms).backward()
    g_ep = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    out = _act_loop(k, model, device)
    assert th.equal(out["act"], ep.step_actions) and th.equal(out["pos"], ep.step_pos)
    tag = f"act_loop/{shape}/t{setting[0]:g}_e{setting[1]:g}"
    for key, ref in (("preds", ep.step_preds), ("logp", ep.step_log_probas), ("values", ep.step_values)):
        REC.fwd(f"{tag}/{key}", out[key], ref)
    _a2c_like_loss(out["preds"], out["logp"], out["values"], k.terms).backward()
    for n, p in model.named_parameters():
        _close(p.grad, g_ep[n], GRAD_TOL, n)
    # (the plain policy acts otherwise: the setting reached both paths)
    model.set_exploration()
    with th.no_grad():
        plain = _sampler(k, model, device).run_episode(k.img.to(device))
    assert not th.equal(plain.step_log_probas, ep.step_log_probas)


def test_step_probabilities_are_the_behaviour_policy(device):
    """ModelsWrapper.forward (probabilities only, no draw) returns pi_b of the plain call's probabilities."""
    from marlclassification_amd.networks.models import RecurrentOutput

    k = _case3("g1")
    i = k.inp
    model = k.model(device)
    obs = mo.crop_patches(k.img, i.pos0, k.cfg.window).to(device)
    npos = mo.normalized_positions(i.pos0, k.sizes).to(device)
    rec = RecurrentOutput(*(t.to(device) for t in (i.h0, i.c0, i.hc0, i.cc0)))
    msg = th.zeros(k.na, k.nb, k.cfg.n_m, device=device)
    with th.no_grad():
        plain = model(obs, msg, npos, rec)[0].actions_probabilities
        model.set_exploration(2.0, 0.1)
        got = model(obs, msg, npos, rec)[0].actions_probabilities
    REC.fwd("step/g1/probs", got, behaviour64(plain.double().cpu(), 2.0, 0.1))


def test_backward_uses_the_setting_of_its_own_forward(device):
    k = _case4("g1")
    model = k.model(device)
    model.set_exploration(2.0, 0.1)
    ref = _run4(k, model, device)
    sampler = sampler4(k, model, device)
    img = k.img.to(device).requires_grad_()
    ep = sampler.run_episode(img)
    loss = _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, k.terms, k.w)
    model.set_exploration(0.5, 0.25)
    assert model.hip_engine(k.cfg.actions).exploration == (0.5, 0.25, False)  # (the engine now holds the second one)
    loss.backward()
    assert th.equal(img.grad, ref["d_img"])
    assert th.equal(th.cat([p.grad.flatten() for _, p in model.named_parameters()]), ref["flat_grad"])
    model.zero_grad(set_to_none=True)
    # the step node likewise
    k3 = _case3("g1")
    m3 = k3.model(device)
    m3.set_exploration(2.0, 0.1)
    out = _act_loop(k3, m3, device)
    _a2c_like_loss(out["preds"], out["logp"], out["values"], k3.terms).backward()
    g_ref = {n: p.grad.clone() for n, p in m3.named_parameters()}
    m3.zero_grad(set_to_none=True)
    out = _act_loop(k3, m3, device)
    loss = _a2c_like_loss(out["preds"], out["logp"], out["values"], k3.terms)
    m3.set_exploration()
    assert m3.hip_engine(None).exploration.is_default
    loss.backward()
    for n, p in m3.named_parameters():
        assert th.equal(p.grad, g_ref[n]), n


def test_two_engines_do_not_see_each_others_setting(device):
    k = _case4("g1")
    a, b = k.model(device), k.model(device)
    a.set_exploration(2.0, 0.1)
    plain = _run4(k, b, device)
    ra = _run4(k, a, device)
    rb = _run4(k, b, device)  # after a call under a's setting: still the plain policy
    ra2 = _run4(k, a, device)
    _all_same_bits(plain, rb, "the plain model after the other's call")
    _all_same_bits(ra, ra2, "the exploring model after the plain one's call")
    assert not th.equal(ra["probs"], plain["probs"])
    assert b.hip_engine(k.cfg.actions).plan_query("explore") == 0
    assert a.hip_engine(k.cfg.actions).plan_query("explore") == 1


# ---- 8: training ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g1", "resisc3"])
def test_train_step_under_a_setting_matches_the_float64_adam_update(device, oracle_explore, shape):
    from marlclassification_amd.training import Trainer

    k = Case(shape)
    tau, eps = 2.0, 0.1
    oracle_explore(tau, eps)
    lr, gamma = 1e-3, 0.99
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    p64 = k.params64()
    tr = _oracle_loop(k, p64, k.img.double())
    lo = mo.a2c_loss(tr["preds"], tr["logp"], tr["values"], y, gamma)
    lo.loss.backward()
    g = _grads_of(p64)
    after = {n: v.detach().clone() for n, v in p64.items()}
    mo.adam_step(after, g, {n: th.zeros_like(v) for n, v in after.items()},
                 {n: th.zeros_like(v) for n, v in after.items()}, 1, lr)
    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    _force(sampler, tr["act"], device)
    trainer = Trainer(model, k.cfg.nb_class, lr, gamma, temperature=tau, explore_eps=eps)
    out, scalars = trainer.train_step(k.img, y, sampler)
    assert model.exploration == (tau, eps, False)
    assert th.equal(out.step_actions.cpu(), tr["act"])
    REC.fwd(f"train_step/{shape}/logp", out.step_log_probas, tr["logp"])
    REC.fwd(f"train_step/{shape}/loss", scalars[0], lo.loss)
    REC.updates_match(f"train_step/{shape}/update", k, model, after, [g], lr, 1)
    # the attributes may change between steps: the next step runs under the new setting
    trainer.temperature, trainer.explore_eps = 1.0, 0.0
    trainer.train_step(k.img, y, sampler)
    assert model.exploration.is_default


def test_two_ppo_epochs_under_a_setting_match_the_float64_oracle(device, oracle_explore):
    from marlclassification_amd.training import Trainer

    # (the shape is chosen from the float64 side alone: under this setting the oracle's own ratios of "g1" come
    # within 9e-5 of the clip bound 0.9 - closer than assert_clear_of_bounds admits -, those of "resisc3" stay 1e-2 away)
    k = Case("resisc3")
    tau, eps_x = 2.0, 0.1
    oracle_explore(tau, eps_x)
    clip, lr = TWO_EPOCH_EPS["resisc3"], TWO_EPOCH["lr"]
    y = _y(k)
    ref = two_epoch_reference(k, y, clip)
    assert_clear_of_bounds(ref["rho"], clip)
    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    _force(sampler, ref["tr"]["act"], device)
    seen = []
    trainer = Trainer(model, k.cfg.nb_class, lr, TWO_EPOCH["gamma"], ppo_epochs=2, ppo_clip=clip,
                      gae_lambda=TWO_EPOCH["lam"], entropy_coef=TWO_EPOCH["beta"], temperature=tau,
                      explore_eps=eps_x)
    eng = model.hip_engine(k.cfg.actions)
    ppo_loss = eng.ppo_loss

    def spy(*a, **kw):
        bufs = ppo_loss(*a, **kw)
        seen.append(bufs[3].clone())
        return bufs
    eng.ppo_loss = spy
    trainer.train_epoch([(k.img, y)], 0, sampler)
    assert trainer.curr_step == 1 and model.flat_state().step == 2 and len(seen) == 2
    # the first epoch replays nothing: the ratio is 1 bit for bit under the rollout's own setting
    assert seen[0][5].item() == 0.0 and seen[0][6].item() == 0.0, "approx_kl / clip_frac of the first epoch"
    REC.fwd("ppo/resisc3/approx_kl", seen[1][5], ref["scalars2"][5])
    REC.fwd("ppo/resisc3/clip_frac", seen[1][6], ref["scalars2"][6])
    REC.fwd("ppo/resisc3/loss", seen[1][0], ref["scalars2"][0])
    REC.updates_match("ppo/resisc3/update", k, model, ref["after"], [ref["g1"], ref["g2"]], lr, 2)


def test_graph_replay_equals_eager_and_a_changed_setting_captures_again(device):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C, draw_episode_device
    from tests.util import Golden, model_spec

    g = Golden("g2_mnist_c1")
    img, y = g.img.to(device), g.y.to(device)
    res, keys = {}, []
    for mode in ("eager", "graph"):
        eng = HipEngine(model_spec(g.cfg), device)
        eng.configure(g.na, g.nb, g.ns, g.img.shape[1:])
        eng.pack({n: v.to(device) for n, v in g.params.items()})
        flat = FlatParams(mo.param_shapes(g.cfg), device)
        flat.load(g.params)
        fa = FusedA2C(eng, flat, 1e-3, g.gamma, use_graph=mode == "graph", temperature=2.0, explore_eps=0.1)
        rows = []
        for it in range(4):
            if it == 2:
                fa.temperature, fa.explore_eps = 0.5, 0.25  # another setting: the graph must be captured again
            if mode == "graph":
                out, sc = fa.iteration_graph(img, y, 77, it)
                keys.append(fa._graph[0])
            else:
                out, sc = fa.iteration(img, y, draw_episode_device(eng, 77, it))
            th.cuda.synchronize()
            rows.append([t.clone() for t in (out.step_preds, out.step_log_probas, out.step_values, out.step_pos, sc,
                                             flat.grads, flat.params)])
        res[mode] = rows
        assert eng.exploration == (0.5, 0.25, False)
    names = ("preds", "logp", "values", "pos", "scalars", "grads", "params")
    # iteration 0 runs eagerly in both modes (the capturing call), iteration 1 is the first replay (see
    # tests/test_gpu_comm.py::test_graph_replay_equals_eager_under_a_matrix for what may differ behind it)
    for it in (0, 1):
        for n, a, b in zip(names, res["eager"][it], res["graph"][it]):
            if n != "params" or it == 0:
                assert th.equal(a, b), f"iteration {it}: {n} differs between eager and replay"
    assert keys[0] == keys[1] and keys[2] != keys[1] and keys[3] == keys[2], "the setting is not part of the graph key"
    # iteration 3 replays the graph captured under the second setting: a stale graph would keep the first setting's
    # log-probabilities, which differ by far more than 1e-4; 1-ulp parameter noise moves them by ~1e-6
    assert th.equal(res["eager"][3][3], res["graph"][3][3]), "iteration 3: positions differ"
    assert (res["eager"][3][1] - res["graph"][3][1]).abs().max().item() <= 1e-4
    assert (res["eager"][1][1] - res["eager"][3][1]).abs().max().item() > 1e-2


# ---- 9: guards -----------------------------------------------------------------------------------------------------
def test_guards(device):
    from marlclassification_amd import _lib
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C
    from marlclassification_amd.training import Trainer
    from tests.util import model_spec

    k = _case4("g1")
    model = k.model(device)
    eng = HipEngine(model_spec(k.cfg), device)
    lib = _lib.load()
    bad = ({"temperature": 0.0}, {"temperature": -1.0}, {"temperature": math.inf}, {"temperature": math.nan},
           {"eps": -0.1}, {"eps": 0.51}, {"eps": math.nan})
    for kw in bad:
        for target in (model.set_exploration, eng.set_exploration):
            with pytest.raises(ValueError):
                target(**kw)
        assert lib.marl_policy_explore(kw.get("temperature", 1.0), kw.get("eps", 0.0), 0) == -1
    assert model.exploration.is_default and eng.exploration.is_default
    for kw in ({"temperature": 0.0}, {"explore_eps": 0.6}):
        with pytest.raises(ValueError):
            Trainer(model, k.cfg.nb_class, 1e-3, 0.99, **kw)
        with pytest.raises(ValueError):
            FusedA2C(eng, FlatParams(mo.param_shapes(k.cfg), device), 1e-3, 0.99, **kw)
    # a bad value assigned to the trainer's attribute is refused by the next step, before anything runs
    trainer = Trainer(model, k.cfg.nb_class, 1e-3, 0.99)
    trainer.explore_eps = 0.7
    sampler = sampler4(k, model, device, probs=False)
    with pytest.raises(ValueError):
        trainer.train_step(k.img, th.zeros(k.nb, dtype=th.int64), sampler)
    assert model.exploration.is_default
    # the library's state is clear behind all of it
    with th.no_grad():
        sampler.run_episode(k.img.to(device))
    assert model.hip_engine(k.cfg.actions).plan_query("explore") == 0
