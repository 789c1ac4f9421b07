"""GPU: the static-shape instantiations of the chained panel kernels (``panel_fwd_static_kernel``, ``panel_bwd_kernel``
over a ``PanelBwdNet``; ``marl_plan_query`` key ``panel_static``) against the run-time-shape kernels.

Both forms are the same source over a shape class: the same MFMAs per accumulator in the same order, the same K-slice
sums, statistics, agent sums, ``sample.h`` chain, cell arithmetic and image stores - so every comparison here is
``np.array_equal``, no tolerance.  The run-time form is chosen by ``MARL_PANEL_STATIC=0``, read once per process: every
case runs in-process with the default form and once more in ONE child process (this file run as a script) with the
switch set, same seeds and weights; the child writes its arrays to a directory of ``tmp_path``.

Widths are the instantiation's (n_b = n_a = 256, n_m = 64, n_m_o = 96, nla = 384, n_d = 16, four actions); everything
else is small (MNIST extractor, window 12, 28 x 28 images, nlb = 24, three steps: the first step, a middle step and the
last one - the two-layer forms - all run).  Rows R = Na * Nb:
  (16, 2): one image per chain workgroup, as at the flagship shape;   (3, 5): one partial panel, by_batch = 5;
  (5, 7): by_batch = 3, the last chain workgroup partial, while the policy role is row-tiled.
One width off (nla = 320) and a ring graph keep the run-time form (``panel_static == 0``) and run green.
The kernels' own entry points (``marl_panel_fwd`` / ``marl_panel_bwd``) are compared the same way at m = 35 rows."""
import ctypes as C
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
from tests import panel_harness as H  # noqa: E402
from tests.util import uniform_params  # noqa: E402

pytestmark = pytest.mark.gpu

NS = 3
KEYS = ("step_actions", "step_pos", "step_log_probas", "step_probs", "step_preds", "step_values")
IMG = (1, 28, 28)


def _cfg(nla=384):
    return mo.OracleConfig("mnist", 12, 256, 256, 64, 96, 16, 10, 24, nla)


# name -> (config, Na, Nb, draw mode, graph, seed, panel_static of the default form)
CASES = {
    "r32_rng": (_cfg(), 16, 2, "rng", None, 41, 1),
    "r15_noise": (_cfg(), 3, 5, "noise", None, 42, 1),
    "r35_rng": (_cfg(), 5, 7, "rng", None, 43, 1),
    "r15_nla320_noise": (_cfg(320), 3, 5, "noise", None, 44, 0),
    "r15_ring_noise": (_cfg(), 3, 5, "noise", "ring", 45, 0),
}


class _Case:
    def __init__(self, name):
        self.cfg, self.na, self.nb, self.mode, self.graph, self.seed, self.static = CASES[name]
        self.params = uniform_params(self.cfg, self.seed)
        g = th.Generator().manual_seed(self.seed)
        self.img = th.rand(self.nb, *IMG, generator=g)
        self.inp = mo.draw_episode_inputs(self.cfg, self.na, self.nb, NS, list(IMG[1:]), self.seed)
        nA = self.cfg.nb_action
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
    from marlclassification_amd.fused import EpisodeDraws

    sampler = EpisodeSampler(MultiAgent(k.na, model), Environment(k.cfg.actions, k.cfg.window), NS)
    sampler.return_probs = True
    i = k.inp
    th.manual_seed(k.seed)
    if k.mode == "noise":  # injected Exp(1) draws; "rng": every draw from the library's counter-based generator
        sampler.fixed_draws = EpisodeDraws(*(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0, i.q[:NS])))
    return sampler.run_episode(k.img.to(device))


def _arrays(ep):
    return {key: getattr(ep, key).detach().cpu().numpy() for key in KEYS}


def _run_case(name, device):
    """No-grad rollout (no saved z / stats) and training rollout + backward of one case -> arrays, panel_static."""
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
    eng = model.hip_engine(k.cfg.actions)
    assert eng.plan_query("panel_chain") == 1, name
    return out, eng.plan_query("panel_static")


# ---- the kernels' own entry points, exact widths, m = 35 (5 agents x 7 images: by_batch = 3, partial panels) ------------
M, NA, NB = 35, 5, 7
ENTRY_FWD = {
    # the chain launch of a middle step and of the last step: chain role beside the row-tiled policy layer
    # (the decoder's output also goes into a k16 image, as the episode has it)
    "fwd_chain4_policy": (H.Fwd("static_chain4", 256, (128, 64, 128, 96), M, "chain", NA, NB, agg_at=2, image=(5, 16, 8)),
                          H.Fwd("static_policy", 256, (384,), M)),
    # the no-grad forms: nothing kept for backward (z and stats null), the image still written
    "fwd_chain4_policy_nosave": (H.Fwd("static_chain4_nosave", 256, (128, 64, 128, 96), M, "chain", NA, NB, agg_at=2,
                                       save=0, image=(5, 16, 8)),
                                 H.Fwd("static_policy_nosave4", 256, (384,), M, save=0)),
    "fwd_chain2_policy_nosave": (H.Fwd("static_chain2", 256, (128, 64), M, "chain", NA, NB, save=0),
                                 H.Fwd("static_policy_nosave", 256, (384,), M, save=0)),
}
_CHAIN_BWD = ((96, 128), (128, 64), (64, 128), (128, 256))
ENTRY_BWD = {
    "bwd_chain4_cells": H.Bwd("static_bwd4_cells", _CHAIN_BWD, M, "chain", NA, NB, agg_at=2, da2=1, accumulate=1,
                              cell=H.Cell(256, rows=77, g3=1), cellb=H.Cell(256, g3=1)),
    "bwd_chain4_no_cell": H.Bwd("static_bwd4", _CHAIN_BWD, M, "chain", NA, NB, agg_at=2, da2=1, accumulate=1),
    "bwd_decoder_step0": H.Bwd("static_bwd2", _CHAIN_BWD[:2], M, "chain", NA, NB, da2=1),
}


def _np(t):
    return t.detach().cpu().numpy()


def _run_entry_fwd(device, cases):
    from marlclassification_amd import _lib

    lib = _lib.load()
    bufs = [H.FwdBufs(c, H.fwd_inputs(c), device) for c in cases]
    for b in bufs:
        if b.case.image:
            row0, _, steps = b.case.image
            b.a3 = th.full((lib.marl_image_bytes(b.case.m + row0 + 2, 16 * steps) + 256,), 0x5A, dtype=th.uint8,
                           device=device)
    need = H.fwd_scratch_bytes(lib, cases)
    scratch = th.full((need // 4 + 64,), float("nan"), device=device)
    _lib.check(lib.marl_panel_fwd(H.fwd_descs(bufs), len(bufs), scratch.data_ptr(), need, None))
    th.cuda.synchronize()
    out = {}
    for i, b in enumerate(bufs):
        for l in range(len(b.case.widths)):
            out[f"p{i}/a{l}"] = _np(b.a[l])
            if b.case.save:
                out[f"p{i}/z{l}"], out[f"p{i}/stats{l}"] = _np(b.z[l]), _np(b.stats[l])
        if b.xbar is not None:
            out[f"p{i}/xbar"] = _np(b.xbar)
        if b.a3 is not None:
            out[f"p{i}/a3_image"] = _np(b.a3)
            assert (out[f"p{i}/a3_image"] != 0x5A).any()
    return out


def _run_entry_bwd(device, case):
    from marlclassification_amd import _lib

    lib = _lib.load()
    bufs = H.BwdBufs(case, H.bwd_inputs(case), device, lib)
    need = H.bwd_scratch_bytes(lib, case)
    scratch = th.full((need // 4 + 64,), float("nan"), device=device)
    d = bufs.desc()
    _lib.check(lib.marl_panel_bwd(C.byref(d), scratch.data_ptr(), need, None))
    th.cuda.synchronize()
    out = {"dx": _np(bufs.dx)}
    for l in range(len(case.layers)):
        out[f"dz{l}"], out[f"part{l}"] = _np(bufs.dz[l]), _np(bufs.part[l])
    for tag, cb in (("cell", bufs.cell), ("cellb", bufs.cellb)):
        if cb is not None:
            out[f"{tag}/gates"], out[f"{tag}/dc"] = _np(cb.gates), _np(cb.dc)
            if cb.g3 is not None:
                out[f"{tag}/g3"] = _np(cb.g3)
            assert getattr(d, f"{tag}_img_done") == 1, tag
    return out


def _run_entry(name, device):
    if name in ENTRY_FWD:
        return _run_entry_fwd(device, ENTRY_FWD[name])
    return _run_entry_bwd(device, ENTRY_BWD[name])


ENTRIES = list(ENTRY_FWD) + list(ENTRY_BWD)


def _child(outdir):
    device = th.device("cuda", 0)
    forms = {}
    for name in CASES:
        out, forms[name] = _run_case(name, device)
        assert forms[name] == 0, f"{name}: MARL_PANEL_STATIC=0, yet panel_static = {forms[name]}"
        np.savez(os.path.join(outdir, name + ".npz"), **out)
    for name in ENTRIES:
        np.savez(os.path.join(outdir, name + ".npz"), **_run_entry(name, device))
    with open(os.path.join(outdir, "forms.json"), "w") as f:
        json.dump(forms, f)


@pytest.fixture(scope="module")
def runtime_form(tmp_path_factory):
    """Every case once in a fresh child process with MARL_PANEL_STATIC=0 (the run-time-shape kernels)."""
    outdir = str(tmp_path_factory.mktemp("panel_static_child"))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), outdir], cwd=root, capture_output=True, text=True,
                       env=dict(os.environ, MARL_PANEL_STATIC="0"), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(os.path.join(outdir, "forms.json")) as f:
        forms = json.load(f)
    assert sorted(forms) == sorted(CASES) and all(v == 0 for v in forms.values()), forms
    return outdir


def _same(name, out, ref):
    assert sorted(ref.files) == sorted(out)
    for key, got in out.items():
        assert got.dtype == ref[key].dtype and got.shape == ref[key].shape, key
        assert np.array_equal(got, ref[key], equal_nan=True), \
            f"{name}/{key}: {int((got != ref[key]).sum())} of {got.size} elements differ from the run-time form"


@pytest.mark.parametrize("name", list(CASES))
def test_episode_bit_equal_to_the_runtime_form(device, runtime_form, name):
    assert os.environ.get("MARL_PANEL_STATIC") != "0", "this test compares the default form with the switch's"
    out, form = _run_case(name, device)
    assert form == CASES[name][-1], f"{name}: panel_static = {form}"
    for key, got in out.items():
        assert np.isfinite(got).all(), key
    _same(name, out, np.load(os.path.join(runtime_form, name + ".npz")))
    assert out["train/flat_grad"].any() and len(np.unique(out["rollout/step_actions"])) > 1


@pytest.mark.parametrize("name", ENTRIES)
def test_entry_points_bit_equal_to_the_runtime_form(device, runtime_form, name):
    assert os.environ.get("MARL_PANEL_STATIC") != "0", "this test compares the default form with the switch's"
    out = _run_entry(name, device)
    for key in ("p0/a3", "p1/a0", "dx", "dz3", "dz1"):
        if key in out:  # (the outputs are written: the sentinel rows and columns apart, finite values)
            assert np.isfinite(out[key][:M, :64]).all() and (out[key][:M, :64] != H.SENT).all(), key
    _same(name, out, np.load(os.path.join(runtime_form, name + ".npz")))


def test_flagship_dimensions_take_the_static_kernels(device):
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
    assert eng.plan_query("panel_static") == 1


if __name__ == "__main__":
    _child(sys.argv[1])
