"""Episode-level parity checks that several test files run: the golden-vector checks of tests/test_gpu_episode.py (also
run under moved knobs by the round 4 and round 6 files), the oracle check of tests/test_gpu_round2.py with its budget of
sampled actions that may flip, and the larger BASELINE.json shapes.

Tolerances (BASELINE.json north_star): agent positions and sampled action indices bit-exact; logits / log-probs /
values within 1e-5 fp32 ABSOLUTE; gradients within 1e-4 of the tensor's scale; one Adam step within 1e-3 of lr per
weight."""
import torch as th

from oracle import marl_oracle as mo
from tests.util import Golden, model_spec, uniform_params

ATOL = 1e-5


def golden_engine(g, device, ns=None):
    from marlclassification_amd.engine import HipEngine

    eng = HipEngine(model_spec(g.cfg), device)
    eng.configure(g.na, g.nb, ns or g.ns, g.img.shape[1:])
    eng.pack({k: v.to(device) for k, v in g.params.items()})
    return eng


def _forward(eng, g, device, forced=None, train=True):
    i = g.inp
    return eng.episode_forward(
        g.img.to(device), i.pos0.to(device), i.h0.to(device), i.c0.to(device), i.hc0.to(device),
        i.cc0.to(device), i.q.to(device), None if forced is None else forced.to(device), train)


def _maxerr(a, b):
    return (a.detach().cpu().double() - b.double()).abs().max().item()


def _relerr(a, b):
    """max |a - b|, ABSOLUTE (north_star: logits within 1e-5 fp32).  Achieved on the fixtures
    (tests/test_gpu_round2.py::test_record_achieved_errors): <= 2e-6 for
    O(1) logits, 7.2e-6 for the trained checkpoint whose logits reach 14.6."""
    return _maxerr(a, b)


def rollout_matches_reference(device, tag, train):
    g = Golden(tag)
    eng = golden_engine(g, device)
    out = _forward(eng, g, device, train=train)
    assert th.equal(out.step_actions.cpu(), g.ref("step_actions")), "sampled actions differ"
    assert th.equal(out.step_pos.cpu(), g.ref("step_pos")), "agent positions differ"
    errs = {
        "preds": _relerr(out.step_preds, g.ref("step_preds")),
        "logp": _relerr(out.step_log_probas, g.ref("step_log_probas")),
        "values": _relerr(out.step_values, g.ref("step_values")),
    }
    assert max(errs.values()) <= ATOL, errs


def loss_and_output_gradients(device, tag):
    g = Golden(tag)
    eng = golden_engine(g, device)
    out = _forward(eng, g, device)
    gp, gl, gv, sc, st = eng.a2c_loss(out, g.y.to(device), g.gamma)
    # oracle: autograd of the restated loss w.r.t. the reference's episode outputs
    p = g.ref("step_preds").clone().requires_grad_(True)
    l = g.ref("step_log_probas").clone().requires_grad_(True)
    v = g.ref("step_values").clone().requires_grad_(True)
    lo = mo.a2c_loss(p, l, v, g.y, g.gamma)
    lo.loss.backward()
    ref_sc = th.stack([lo.loss, lo.path, lo.error, lo.critic]).detach()
    assert th.allclose(sc.cpu(), ref_sc, rtol=2e-5, atol=2e-5), (sc.cpu(), ref_sc)
    assert th.allclose(sc.cpu(), g.ref("loss"), rtol=2e-5, atol=2e-5), (sc.cpu(), g.ref("loss"))
    for a, b, n in ((gp, p.grad, "g_preds"), (gl, l.grad, "g_logp"), (gv, v.grad, "g_values")):
        scale = b.abs().max().item()
        assert _maxerr(a, b) <= 2e-5 * scale + 1e-8, (n, _maxerr(a, b), scale)


def backward_and_adam_match_reference(device, tag):
    g = Golden(tag)
    eng = golden_engine(g, device)
    out = _forward(eng, g, device)
    gp, gl, gv, sc, st = eng.a2c_loss(out, g.y.to(device), g.gamma)
    grads = {k: th.full_like(v, float("nan"), device=device) for k, v in g.params.items()}
    eng.episode_backward(gp, gl, gv, grads)
    bad = {}
    for k in g.params:
        ref = g.grad(k)
        err = _maxerr(grads[k], ref)
        tol = 1e-4 * ref.abs().max().item() + 1e-7
        if not err <= tol:
            bad[k.replace("_ModelsWrapper__", "")] = "%.2e/%.2e" % (err, ref.abs().max().item())
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())
    # one Adam step on the flat buffers (th.optim.Adam defaults, trainer.py:33)
    names = list(g.params)
    flat_p = th.cat([g.params[k].flatten() for k in names]).to(device)
    flat_g = th.cat([grads[k].flatten() for k in names])
    m, v = th.zeros_like(flat_p), th.zeros_like(flat_p)
    eng.adam(flat_p, flat_g, m, v, 1, g.lr)
    ref_after = th.cat([g.after(k).flatten() for k in names])
    ref_before = th.cat([g.params[k].flatten() for k in names])
    # the first Adam step moves every weight by ~lr * sign(g); compare the update itself
    upd, ref_upd = flat_p.cpu() - ref_before, ref_after - ref_before
    big = th.cat([g.grad(k).flatten() for k in names]).abs() > 1e-6
    # achieved: <= 1e-4 of lr on every fixture
    err = (upd[big] - ref_upd[big]).abs().max().item()
    assert err <= 1e-3 * g.lr, f"Adam update: err {err:.3e}, bound {1e-3 * g.lr:.3e}"


def backward_resisc_dims_gradient_samples(device):
    g = Golden("g4_resisc_b2")
    eng = golden_engine(g, device)
    out = _forward(eng, g, device, forced=g.ref("step_actions"))
    gp, gl, gv, sc, st = eng.a2c_loss(out, g.y.to(device), g.gamma)
    assert th.allclose(sc.cpu(), g.ref("loss"), rtol=5e-5, atol=5e-5), (sc.cpu(), g.ref("loss"))
    grads = {k: th.zeros_like(v, device=device) for k, v in g.params.items()}
    eng.episode_backward(gp, gl, gv, grads)
    bad = {}
    for i, k in enumerate(g.params):
        idx = th.from_numpy(g.z["gradidx/" + k])
        ref = th.from_numpy(g.z["gradsample/" + k])
        got = grads[k].flatten()[idx.to(device)].cpu()
        scale = float(g.z["grads_abs_sum"][i]) / max(1, g.params[k].numel())  # mean |g|
        err = (got - ref).abs().max().item()
        if not err <= 1e-4 * max(ref.abs().max().item(), scale) + 1e-7:
            bad[k] = (err, ref.abs().max().item())
    assert not bad, bad


# ---- the other BASELINE.json configurations, at a batch the oracle finishes in seconds -------
BIG_CASES = {
    # C2: MNIST shapes at a larger batch (configs[1] uses batch 1024; 64 keeps the oracle fast)
    "c2_mnist": (mo.OracleConfig("mnist", 6, 64, 64, 16, 24, 8, 10, 96, 96), 3, 64, 5, (3, 28, 28)),
    # C4: AID 600x600, f=24, 4 conv layers (128 channels), stride-3 moves, 30 classes
    "c4_aid": (mo.OracleConfig("aid", 24, 256, 256, 64, 96, 16, 30, 320, 320,
                               actions=[[3, 0], [-3, 0], [0, 3], [0, -3]]), 16, 2, 16, (3, 600, 600)),
    # C5: synthetic 1024x1024, 64 agents, 32 steps, f=32 (AidCnn + RESISC hidden sizes)
    "c5_synth": (mo.OracleConfig("aid", 32, 256, 256, 64, 96, 16, 45, 384, 384,
                                 actions=[[4, 0], [-4, 0], [0, 4], [0, -4]]), 64, 1, 32, (3, 1024, 1024)),
}



# ---- against the oracle alone -----------------------------------------------------------------------------------------
def oracle_engine(cfg, device, na, nb, ns, shape, params, img_u8=False):
    from marlclassification_amd.engine import HipEngine

    eng = HipEngine(model_spec(cfg), device)
    eng.configure(na, nb, ns, shape, img_u8=img_u8)
    eng.pack({k: v.to(device) for k, v in params.items()})
    return eng


def oracle_case(cfg, na, nb, ns, shape, seed=7):
    params = uniform_params(cfg, seed)
    img = th.rand(nb, *shape, generator=th.Generator().manual_seed(seed + 4))
    y = th.randint(0, cfg.nb_class, (nb,), generator=th.Generator().manual_seed(seed + 5))
    inp = mo.draw_episode_inputs(cfg, na, nb, ns, shape[1:], seed + 6)
    return params, img, y, inp


def check_against_oracle(eng, cfg, device, params, img, y, inp, ns, img_dev=None, free_running=True):
    """Teacher-forced episode + loss + every gradient against the oracle; returns achieved errors."""
    tr, lo, grads = mo.train_iteration(params, cfg, img, y, inp, ns, 0.99)
    args = [t.to(device) for t in (inp.pos0, inp.h0, inp.c0, inp.hc0, inp.cc0, inp.q)]
    img_dev = img.to(device) if img_dev is None else img_dev
    out = eng.episode_forward(img_dev, *args, tr.step_actions.to(device), True)
    assert th.equal(out.step_pos.cpu(), tr.step_pos), "agent positions differ"
    errs = {"preds": _maxerr(out.step_preds, tr.step_preds), "logp": _maxerr(out.step_log_probas, tr.step_log_probas),
            "values": _maxerr(out.step_values, tr.step_values)}
    assert max(errs.values()) <= ATOL, errs
    gp, gl, gv, sc, _ = eng.a2c_loss(out, y.to(device), 0.99)
    assert abs(sc[0].item() - lo.loss.item()) <= 5e-5 * max(1.0, abs(lo.loss.item())), (sc[0].item(), lo.loss.item())
    g_out = {k: th.full_like(v, float("nan"), device=device) for k, v in params.items()}
    eng.episode_backward(gp, gl, gv, g_out)
    bad, worst = {}, 0.0
    for k, ref in grads.items():
        err = _maxerr(g_out[k], ref)
        rel = err / (ref.abs().max().item() + 1e-30)
        worst = max(worst, rel if ref.abs().max().item() > 1e-12 else 0.0)
        if not err <= 1e-4 * ref.abs().max().item() + 1e-7:
            bad[k.replace("_ModelsWrapper__", "")] = "%.2e/%.2e" % (err, ref.abs().max().item())
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())
    if free_running:
        free = eng.episode_forward(img_dev, *args, None, False)
        nflip = (free.step_actions.cpu() != tr.step_actions).sum().item()
        allowed = flip_budget(tr, inp, errs["logp"])
        FLIPS.append({"numel": tr.step_actions.numel(), "flips": nflip, "allowed": allowed})
        assert nflip <= allowed, f"{nflip} sampled actions differ (budget {allowed})"
    errs["grad_rel"] = worst
    return errs


FLIPS = []  # (numel, flips, allowed) of every oracle-only free-running comparison of this session


def flip_budget(tr, inp, logp_err):
    """How many sampled indices MAY differ from the oracle's: a sample is argmax_k p_k / q_k
    (core/agent.py:53-55); it can only flip where the two largest ratios are closer than the
    relative error of the probabilities.  Counted on the oracle's own probabilities and noise
    with 4x the measured log-prob error (>= 2e-6) as that relative error: 0 for almost every case."""
    eps = 4.0 * max(logp_err, 5e-7)
    if not hasattr(tr, "step_probs") or tr.step_probs is None:
        return 0
    ratio = tr.step_probs.double() / inp.q.double().view_as(tr.step_probs)
    top2 = ratio.topk(2, dim=-1).values
    return int(((top2[..., 0] - top2[..., 1]) <= eps * top2[..., 0]).sum().item())
