"""GPU: action sampling as the epilogue of the chained panel launch's policy workgroups (``panel_fwd_kernel<4, MIX,
true>``, ``marl_plan_query`` key ``panel_sample``) against the separate ``sample_kernel`` launch.

Both forms run the same device functions of ``sample.h`` on the same values in the same order, so every comparison
here is ``np.array_equal`` - no tolerance.  The separate launch is chosen by ``MARL_PANEL_SAMPLE=0``, read once per
process: every case runs in-process with the default form and once more in ONE child process (this file run as a
script) with the switch set, same seeds and weights; the child writes its arrays to a directory of ``tmp_path``.

Cases - the smallest shapes at which the epilogue can go wrong (rows R = Na * Nb in 16-row panels, three steps so that
the first, a middle and the last step - the one without a position embedding - all run):
  R = 15 (3, 5): one partial panel;   R = 35 (5, 7): the last panel partial, the chain role owns 3 batch elements per
  workgroup while the policy role is row-tiled;   R = 32 (16, 2): one batch element per chain workgroup, as at the
  flagship shape;   nla = 96 (two of the six column slots in use) and 384 (all six);   n_d = 16 (the embedding's
  four-columns-a-lane form) and 19 (its strided form);   every draw mode: the in-kernel generator, injected noise,
  forced actions;   a ring graph (the MIX instantiation);   eight actions (whichever form the build gives them)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

if __name__ == "__main__":  # the child process: the repository root is not on its path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import marl_oracle as mo  # noqa: E402
from tests.util import uniform_params  # noqa: E402

pytestmark = pytest.mark.gpu

NS = 3
EIGHT = [[1, 0], [-1, 0], [0, 1], [0, -1], [2, 0], [-2, 0], [0, 2], [0, -2]]
KEYS = ("step_actions", "step_pos", "step_log_probas", "step_probs", "step_preds", "step_values")


def _cfg(n_d, nla, actions=None):
    kw = {} if actions is None else {"actions": actions}
    return mo.OracleConfig("mnist", 12, 23, 22, 21, 20, n_d, 10, 24, nla, **kw)


# name -> (config, Na, Nb, draw mode, graph, seed, the fused form is expected)
CASES = {
    "r15_nla96_rng": (_cfg(16, 96), 3, 5, "rng", None, 31, True),
    "r35_nla384_noise": (_cfg(19, 384), 5, 7, "noise", None, 32, True),
    "r32_nla96_forced": (_cfg(16, 96), 16, 2, "forced", None, 33, True),
    "r32_nla384_rng": (_cfg(16, 384), 16, 2, "rng", None, 34, True),
    "r32_nla384_ring_noise": (_cfg(16, 384), 16, 2, "noise", "ring", 35, True),
    "r15_nla96_eight_actions_noise": (_cfg(16, 96, EIGHT), 3, 5, "noise", None, 36, None),
}
IMG = (1, 28, 28)


class _Case:
    def __init__(self, name):
        self.cfg, self.na, self.nb, self.mode, self.graph, self.seed, self.fused = CASES[name]
        self.params = uniform_params(self.cfg, self.seed)
        g = th.Generator().manual_seed(self.seed)
        self.img = th.rand(self.nb, *IMG, generator=g)
        self.inp = mo.draw_episode_inputs(self.cfg, self.na, self.nb, NS, list(IMG[1:]), self.seed)
        nA = self.cfg.nb_action
        self.forced = th.randint(nA, (NS, self.na, self.nb), generator=g)
        self.w = [th.randn(NS, self.na, self.nb, generator=g), th.randn(NS, self.na, self.nb, generator=g),
                  th.randn(NS, self.na, self.nb, self.cfg.nb_class, generator=g),
                  th.randn(NS, self.na, self.nb, nA, generator=g)]

    def model(self, device):
        from marlclassification_amd import comm
        from marlclassification_amd.networks import ModelsWrapper
        from marlclassification_amd.networks.vision import MnistCnn

        c = self.cfg
        m = ModelsWrapper(MnistCnn(c.window), c.n_b, c.n_a, c.n_m, c.n_m_o, c.n_d, 2, c.nb_action, c.nb_class, c.nlb,
                          c.nla)
        m.load_state_dict(self.params)
        m = m.to(device)
        if self.graph == "ring":
            m.set_comm(comm.ring(self.na, 1).to(device))
        return m


def _episode(k, model, device):
    """One episode of case k in its draw mode from a fresh sampler (episode counter 0 under the seed)."""
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.core.episode import Trajectory
    from marlclassification_amd.fused import EpisodeDraws

    sampler = EpisodeSampler(MultiAgent(k.na, model), Environment(k.cfg.actions, k.cfg.window), NS)
    sampler.return_probs = True
    i = k.inp
    draws = EpisodeDraws(*(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0, i.q[:NS])))
    th.manual_seed(k.seed)
    if k.mode == "rng":  # every draw from the library's counter-based generator, Exp(1) inside the sampling chain
        return sampler.run_episode(k.img.to(device))
    sampler.fixed_draws = draws
    replay = Trajectory(draws, k.forced.to(device)) if k.mode == "forced" else None
    return sampler.run_episode(k.img.to(device), replay=replay)


def _arrays(ep):
    return {key: getattr(ep, key).detach().cpu().numpy() for key in KEYS}


def _run_case(name, device):
    """No-grad rollout and training rollout (+ backward) of one case -> {array name: ndarray}, panel_sample."""
    k = _Case(name)
    model = k.model(device)
    out = {}
    with th.no_grad():
        out.update({f"rollout/{key}": v for key, v in _arrays(_episode(k, model, device)).items()})
    ep = _episode(k, model, device)
    out.update({f"train/{key}": v for key, v in _arrays(ep).items()})
    wl, wv, wp, wq = (t.to(device) for t in k.w)
    loss = (ep.step_log_probas * wl).sum() + (ep.step_values * wv).sum() + (ep.step_preds * wp).sum() + \
        (ep.step_probs * wq).sum() + 0.5 * ep.step_preds.square().sum()
    loss.backward()
    out["train/flat_grad"] = th.cat([p.grad.flatten() for p in model.parameters()]).cpu().numpy()
    return out, model.hip_engine(k.cfg.actions).plan_query("panel_sample")


def _child(outdir):
    device = th.device("cuda", 0)
    forms = {}
    for name in CASES:
        out, forms[name] = _run_case(name, device)
        assert forms[name] == 0, f"{name}: MARL_PANEL_SAMPLE=0, yet panel_sample = {forms[name]}"
        np.savez(os.path.join(outdir, name + ".npz"), **out)
    with open(os.path.join(outdir, "forms.json"), "w") as f:
        json.dump(forms, f)


@pytest.fixture(scope="module")
def separate_launch(tmp_path_factory):
    """Every case once in a fresh child process with MARL_PANEL_SAMPLE=0 (chain launch, then sample_kernel)."""
    outdir = str(tmp_path_factory.mktemp("panel_sample_child"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), outdir], cwd=root, capture_output=True, text=True,
                       env=dict(os.environ, MARL_PANEL_SAMPLE="0"), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(outdir, "forms.json")) as f:
        forms = json.load(f)
    assert forms and all(v == 0 for v in forms.values()), forms
    return outdir


@pytest.mark.parametrize("name", list(CASES))
def test_bit_equal_to_the_separate_launch(device, separate_launch, name):
    assert os.environ.get("MARL_PANEL_SAMPLE") != "0", "this test compares the default form with the switch's"
    out, form = _run_case(name, device)
    fused = CASES[name][-1]
    if fused is not None:  # (None: eight actions take whichever form the build has for them)
        assert form == int(fused), f"{name}: panel_sample = {form}"
    ref = np.load(os.path.join(separate_launch, name + ".npz"))
    assert sorted(ref.files) == sorted(out)
    for key, got in out.items():
        assert got.dtype == ref[key].dtype and got.shape == ref[key].shape, key
        assert np.isfinite(got).all(), key
        assert np.array_equal(got, ref[key]), \
            f"{name}/{key}: {int((got != ref[key]).sum())} of {got.size} elements differ from the separate launch"
    assert out["train/flat_grad"].any() and len(np.unique(out["rollout/step_actions"])) > 1


def test_flagship_dimensions_sample_inside_the_chain_launch(device):
    import bench
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import CNN_BY_NAME

    c = bench.C3
    actions = [[1, 0], [-1, 0], [0, 1], [0, -1]]
    model = ModelsWrapper(CNN_BY_NAME[c["ft_extr"]](c["window"]), c["n_b"], c["n_a"], c["n_m"], c["n_m_o"], c["n_d"],
                          2, len(actions), c["nb_class"], c["nlb"], c["nla"]).to(device)
    eng = model.hip_engine(actions)
    eng.configure(bench.NA, 256, bench.NS, bench.IMG)
    assert eng.plan_query("panel_chain") == 1 and eng.plan_query("panel_sample") == 1


if __name__ == "__main__":
    _child(sys.argv[1])
