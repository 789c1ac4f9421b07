"""GPU: episode rollout, loss, backward and Adam of the HIP path against the golden
vectors generated from the real reference and against the CPU oracle.

Tolerances (BASELINE.json north_star): agent positions and sampled action indices
bit-exact; logits / log-probs / values within 1e-5 fp32 ABSOLUTE; gradients within 1e-4 of the
tensor's scale; one Adam step within 1e-3 of lr per weight."""
import os

import pytest
import torch as th

from oracle import marl_oracle as mo
from tests import episode_checks as E
from tests.episode_checks import ATOL, BIG_CASES, FLIPS, _forward, _maxerr, _relerr, flip_budget
from tests.episode_checks import golden_engine as _engine
from tests.util import Golden

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", ["g1_conftest", "g2_mnist_c1", "g3_mnist_ckpt"])
@pytest.mark.parametrize("train", [True, False])
def test_rollout_matches_reference(device, tag, train):
    E.rollout_matches_reference(device, tag, train)


def test_rollout_intermediates_conftest(device):
    """Localises a mismatch: per-step u_t, h_t, h^_t, msg_t against the oracle trace."""
    g = Golden("g1_conftest")
    eng = _engine(g, device)
    _forward(eng, g, device)
    tr = mo.run_episode(g.params, g.cfg, g.img, g.inp, g.ns)
    R = g.na * g.nb
    for t in range(g.ns):
        u = eng.debug_buffer("U", t)[:, : g.cfg.nin]
        assert _maxerr(u, tr.step_u[t].reshape(R, -1)) <= ATOL, ("u", t)
        h = eng.debug_buffer("H", t + 1)[:, : g.cfg.n_b]
        assert _maxerr(h, tr.step_h[t].reshape(R, -1)) <= ATOL, ("h", t)
        hc = eng.debug_buffer("HC", t + 1)[:, : g.cfg.n_a]
        assert _maxerr(hc, tr.step_hc[t].reshape(R, -1)) <= ATOL, ("hc", t)
        m = eng.debug_buffer("MSG", t + 1)[:, : g.cfg.n_m]
        assert _maxerr(m, tr.step_msg[t].reshape(R, -1)) <= ATOL, ("msg", t)


def test_rollout_resisc_dims_teacher_forced(device):
    """RESISC45 dims (16 agents, 16 steps, f=12, 256x256): actions teacher-forced to the
    reference's so one ulp in a probability cannot fork the trajectory."""
    g = Golden("g4_resisc_b2")
    eng = _engine(g, device)
    out = _forward(eng, g, device, forced=g.ref("step_actions"))
    assert th.equal(out.step_pos.cpu(), g.ref("step_pos"))
    errs = {
        "preds": _maxerr(out.step_preds, g.ref("step_preds")),
        "logp": _maxerr(out.step_log_probas, g.ref("step_log_probas")),
        "values": _maxerr(out.step_values, g.ref("step_values")),
    }
    assert max(errs.values()) <= ATOL, errs
    # free-running: the sampled trajectory itself (512 x 16 samples) must agree too
    free = _forward(eng, g, device)
    nflip = (free.step_actions.cpu() != g.ref("step_actions")).sum().item()
    assert nflip == 0, f"{nflip} sampled actions differ from the reference"


@pytest.mark.parametrize("tag", ["g1_conftest", "g2_mnist_c1", "g3_mnist_ckpt"])
def test_loss_and_output_gradients(device, tag):
    E.loss_and_output_gradients(device, tag)


@pytest.mark.parametrize("tag", ["g1_conftest", "g2_mnist_c1", "g3_mnist_ckpt"])
def test_backward_and_adam_match_reference(device, tag):
    E.backward_and_adam_match_reference(device, tag)


def test_backward_resisc_dims_gradient_samples(device):
    E.backward_resisc_dims_gradient_samples(device)


def test_step_api_matches_oracle(device):
    """MultiAgent.act / ModelsWrapper.forward used standalone (marl_step_forward)."""
    g = Golden("g1_conftest")
    eng = _engine(g, device, ns=1)
    i = g.inp
    sizes = list(g.img.shape[2:])
    obs = mo.crop_patches(g.img, i.pos0, g.cfg.window)
    msg = th.randn(g.na, g.nb, g.cfg.n_m, generator=th.Generator().manual_seed(5))
    npos = mo.normalized_positions(i.pos0, sizes)
    so = mo.step_forward(g.params, g.cfg, obs, msg, npos, i.h0, i.c0, i.hc0, i.cc0)
    got = eng.step_forward(*(t.to(device) for t in (obs, msg, npos, i.h0, i.c0, i.hc0, i.cc0)))
    for a, b, n in zip(got, (so.probs, so.values, so.preds, so.msg, so.h, so.c, so.hc, so.cc),
                       ("probs", "values", "preds", "msg", "h", "c", "hc", "cc")):
        assert _maxerr(a, b) <= ATOL, n


# ---- the other BASELINE.json configurations (tests/episode_checks.py::BIG_CASES) ---------------
@pytest.mark.parametrize("tag", list(BIG_CASES))
def test_other_baseline_configs_match_oracle(device, tag):
    """Episode + full update at the shapes of BASELINE.json configs[1], [3], [4]: trajectory
    teacher-forced to the oracle's (so a 1-ulp probability difference cannot fork it),
    logits / values within 1e-5 of scale, every gradient within 1e-4 of its scale, and the
    free-running sampled trajectory compared as well."""
    from marlclassification_amd.engine import HipEngine
    from tests.util import model_spec, uniform_params

    cfg, na, nb, ns, shape = BIG_CASES[tag]
    params = uniform_params(cfg, 7)
    img = th.rand(nb, *shape, generator=th.Generator().manual_seed(11))
    y = th.randint(0, cfg.nb_class, (nb,), generator=th.Generator().manual_seed(12))
    inp = mo.draw_episode_inputs(cfg, na, nb, ns, shape[1:], 13)
    th.set_num_threads(max(1, th.get_num_threads()))
    tr, lo, grads = mo.train_iteration(params, cfg, img, y, inp, ns, 0.99)

    eng = HipEngine(model_spec(cfg), device)
    eng.configure(na, nb, ns, shape)
    eng.pack({k: v.to(device) for k, v in params.items()})
    args = [t.to(device) for t in (img, inp.pos0, inp.h0, inp.c0, inp.hc0, inp.cc0, inp.q)]
    out = eng.episode_forward(*args, tr.step_actions.to(device), True)
    assert th.equal(out.step_pos.cpu(), tr.step_pos)
    errs = {"preds": _relerr(out.step_preds, tr.step_preds.detach()),
            "logp": _relerr(out.step_log_probas, tr.step_log_probas.detach()),
            "values": _relerr(out.step_values, tr.step_values.detach())}
    assert max(errs.values()) <= ATOL, errs
    gp, gl, gv, sc, st = eng.a2c_loss(out, y.to(device), 0.99)
    assert abs(sc[0].item() - lo.loss.item()) <= 5e-5 * max(1.0, abs(lo.loss.item()))
    g_out = {k: th.zeros_like(v, device=device) for k, v in params.items()}
    eng.episode_backward(gp, gl, gv, g_out)
    bad = {}
    for k, ref in grads.items():
        err = _maxerr(g_out[k], ref)
        if not err <= 1e-4 * ref.abs().max().item() + 1e-7:
            bad[k.replace("_ModelsWrapper__", "")] = "%.2e/%.2e" % (err, ref.abs().max().item())
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())
    free = eng.episode_forward(*args, None, False)
    nflip = (free.step_actions.cpu() != tr.step_actions).sum().item()
    # budget: samples whose two largest p / q ratios are closer than the probabilities' error
    allowed = flip_budget(tr, inp, errs["logp"])
    FLIPS.append({"numel": tr.step_actions.numel(), "flips": nflip, "allowed": allowed})
    assert nflip <= allowed, f"{nflip} sampled actions differ (budget {allowed})"


@pytest.mark.parametrize("env", [{"MARL_CNN_FUSED": "0", "MARL_PANELS": "0"},
                                 {"MARL_PANEL_CHAIN": "0", "MARL_RED_DEFER": "0"}])
def test_alternative_kernel_paths_in_subprocess(device, env):
    """The unfused CNN / LayerNorm-GEMM fallbacks (used for shapes outside the fused kernels'
    range) and the opt-in GEMM schedules are selected by environment variables read once per
    process, so the parity cases are re-run in a child process with them set."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    child_env = dict(os.environ, **env)
    r = subprocess.run(
        [sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_episode.py"), "-x", "-q",
         "-m", "gpu", "-k", "rollout_matches_reference or backward_and_adam or conftest"],
        cwd=root, env=child_env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
