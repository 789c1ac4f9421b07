"""The shapes, settings and synthetic episode outputs of the loss-option tests (class weights, label smoothing, step
weights, weighted rewards, soft targets), and the call sequence that runs every loss entry once."""
import torch as th

from oracle import marl_oracle as mo
from tests import loss_ref
from tests.cases import NS
from tests.loss_ref import ratio_deltas
from tests.util import model_spec

A2C_SCALARS = ("loss", "path", "error", "critic", "entropy")
PPO_SCALARS = ("loss", "surrogate", "error", "critic", "entropy", "approx_kl", "clip_frac")
GAMMA, BETA = 0.97, 0.05
# nC = 3 (less than a wave), 45, 70 (a second lane-stride pass with a ragged tail); Na = 1, 3 with Nb = 5, Ns = 3
# (Ns Nb = 15 and Ns R leave partial four-wave blocks); and Na = 16, Nb = 6 (Ns R = 288 > 256: the extra partials of the
# entropy / PPO passes sit where the weighted rewards were)
SHAPES = [(3, 1, 5), (3, 3, 5), (45, 1, 5), (45, 3, 5), (70, 1, 5), (70, 3, 5), (45, 16, 6)]  # (nC, Na, Nb), Ns = 3
STEP_W = (0.0, 0.5, 2.0)


def weights(nc, seed, zero=None):
    """fp32 class weights in [0.25, 2.25); ``zero``: a class of weight exactly 0."""
    w = th.rand(nc, generator=th.Generator().manual_seed(seed)) * 2.0 + 0.25
    if zero is not None:
        w[zero] = 0.0
    return w


def all_on(nc, y, ns=NS):
    """Every option at once; the first image's class has weight exactly 0."""
    from marlclassification_amd import class_loss as cl

    return cl.ClassLoss(nc, ns, weights(nc, 50 + nc, zero=int(y[0])), 0.1, STEP_W[:ns], True)


def _engine(nc, na, nb, ns, device, n_act=4):
    from marlclassification_amd.engine import HipEngine

    actions = [[1, 0], [-1, 0], [0, 1], [0, -1], [0, 0], [2, 2]][:n_act]
    cfg = mo.OracleConfig("mnist", 6, 32, 32, 8, 12, 8, nc, 48, 48, actions=actions)
    eng = HipEngine(model_spec(cfg), device)
    eng.configure(na, nb, ns, (1, 28, 28))
    return eng


def synthetic(nc, na, nb, ns, device, n_act=4, seed=0, gap=None):
    """Episode outputs with votes from vague to confident (logit scale 1 .. 15 per image); ``gap``: one class of every
    second image is ``gap`` above the rest - the label on image 0, another class on image 2."""
    from marlclassification_amd.engine import EpisodeTensors

    gen = th.Generator().manual_seed(1000 + seed + nc * na * nb)
    scale = th.linspace(1.0, 15.0, nb).view(1, 1, nb, 1)
    preds = th.randn(ns, na, nb, nc, generator=gen) * scale
    y = th.randint(nc, (nb,), generator=gen)
    if gap is not None:
        for b in range(0, nb, 2):
            k = int(y[b]) if b % 4 == 0 else (int(y[b]) + 1) % nc
            preds[:, :, b, k] += gap
    values = th.randn(ns, na, nb, generator=gen)
    probs = th.randn(ns, na, nb, n_act, generator=gen).softmax(-1)
    act = th.randint(n_act, (ns, na, nb), generator=gen)
    logp = probs.gather(-1, act.unsqueeze(-1)).squeeze(-1).log()
    host = EpisodeTensors(preds, logp, values, th.zeros(ns, na, nb, 2, dtype=th.int64), act, probs)
    out = EpisodeTensors(*(t.to(device) for t in (preds, logp, values, host.step_pos, act, probs)))
    return host, out, y


def _leaves(o):
    return [t.detach().double().cpu().requires_grad_()
            for t in (o.step_preds, o.step_log_probas, o.step_values, o.step_probs)]


def _entries(eng, out, y, device):
    """The outputs of every entry (cloned) under whatever is installed in the engine."""
    yd = y.to(device)
    res = []
    for beta in (0.0, BETA):
        res += [t.clone() for t in eng.a2c_loss(out, yd, GAMMA, entropy_coef=beta)]
    for lam in (1.0, 0.9):
        adv = eng.advantages(out, yd, GAMMA, lam)
        res += [adv[j].clone() for j in (4, 5, 6)]
    advn, ret = res[-2], res[-1]
    old_logp = out.step_log_probas - ratio_deltas(out.step_log_probas.shape).float().to(device)
    for beta in (0.0, BETA):
        bufs = eng.ppo_loss(out, yd, old_logp, advn, ret, 0.1, entropy_coef=beta)
        res += [bufs[j].clone() for j in (0, 1, 2, 3) + ((7,) if beta > 0 else ())]
    return res


def check_entries(rec, eng, out, y, c, q, tag, device):
    """a2c_loss (plain and entropy entry), advantages (lambda 1 and 0.9), ppo_loss (without and with the bonus) under
    the options ``c`` and the targets ``q`` (host fp32; either may be None) against float64, recorded by ``rec``; phases
    1 + 2 against phase 0 and a second run, bit for bit.  The caller has installed ``c`` and ``q`` in the engine.
    Returns the cloned buffers."""
    yd = y.to(device)
    kept = {}
    for beta in (0.0, BETA):
        bufs = [t.clone() for t in eng.a2c_loss(out, yd, GAMMA, entropy_coef=beta)]
        lv = _leaves(out)
        loss, ref_scalars = loss_ref.a2c(*lv, y, GAMMA, beta, c, q)
        loss.backward()
        for j, what in enumerate(A2C_SCALARS[:bufs[3].numel()]):
            rec.fwd(f"{tag}/a2c/beta{beta}/scalar_{what}", bufs[3][j], ref_scalars[j])
        grads = [bufs[0], bufs[1], bufs[2]] + ([bufs[5]] if beta > 0 else [])
        for got, leaf, what in zip(grads, lv, ("g_preds", "g_logp", "g_values", "g_probs")):
            rec.grad(f"{tag}/a2c/beta{beta}/{what}", got, leaf.grad)
        assert all(bool(th.isfinite(t).all()) for t in bufs), f"{tag}: a2c_loss (beta {beta}) wrote a NaN or an Inf"
        two = eng.new_loss_bufs(out, beta > 0)
        eng.a2c_loss(out, yd, GAMMA, 1, two, entropy_coef=beta)
        eng.a2c_loss(out, yd, GAMMA, 2, two, entropy_coef=beta)
        again = eng.a2c_loss(out, yd, GAMMA, entropy_coef=beta)
        for a, b, d in zip(bufs, two, again):
            assert th.equal(a, b), "a2c_loss: phases 1 + 2 differ from phase 0"
            assert th.equal(a, d), "a2c_loss: two runs differ"
        kept[f"a2c{beta}"] = bufs
    for lam in (1.0, 0.9):
        adv = [t.clone() for t in eng.advantages(out, yd, GAMMA, lam)]
        advn64, ret64, _ = loss_ref.advantages(out.step_preds.double().cpu(), out.step_values.double().cpu(), y, GAMMA,
                                               lam, c, q)
        rec.fwd(f"{tag}/lam{lam}/advn", adv[5], advn64)
        rec.fwd(f"{tag}/lam{lam}/ret", adv[6], ret64)
        two = eng.new_ppo_bufs(out, True)
        eng.advantages(out, yd, GAMMA, lam, 1, two)
        eng.advantages(out, yd, GAMMA, lam, 2, two)
        again = eng.advantages(out, yd, GAMMA, lam)
        for j in (4, 5, 6):
            assert th.equal(adv[j], two[j]), "advantages: phases 1 + 2 differ from phase 0"
            assert th.equal(adv[j], again[j]), "advantages: two runs differ"
        kept[f"adv{lam}"] = adv
    advn, ret = kept["adv0.9"][5], kept["adv0.9"][6]
    old_logp = out.step_log_probas - ratio_deltas(out.step_log_probas.shape).float().to(device)
    eps = 0.1
    for beta in (0.0, BETA):
        bufs = [t.clone() for t in eng.ppo_loss(out, yd, old_logp, advn, ret, eps, entropy_coef=beta)]
        lv = _leaves(out)
        loss, ref_scalars, rho, _ = loss_ref.ppo(*lv, y, old_logp.double().cpu(), advn.double().cpu(),
                                                 ret.double().cpu(), eps, beta, c, q)
        loss_ref.assert_clear_of_bounds(rho, eps)
        loss.backward()
        for j, what in enumerate(PPO_SCALARS):
            rec.fwd(f"{tag}/ppo/beta{beta}/scalar_{what}", bufs[3][j], ref_scalars[j])
        grads = [bufs[0], bufs[1], bufs[2]] + ([bufs[7]] if beta > 0 else [])
        for got, leaf, what in zip(grads, lv, ("g_preds", "g_logp", "g_values", "g_probs")):
            rec.grad(f"{tag}/ppo/beta{beta}/{what}", got, leaf.grad)
        again = eng.ppo_loss(out, yd, old_logp, advn, ret, eps, entropy_coef=beta)
        for j in (0, 1, 2, 3) + ((7,) if beta > 0 else ()):
            assert th.equal(bufs[j], again[j]), "ppo_loss: two runs differ"
        kept[f"ppo{beta}"] = bufs
    return kept


def _trainer_options(k, y):
    return dict(class_weights=weights(k.cfg.nb_class, 21, zero=int(y[0])).tolist(), label_smoothing=0.1,
                error_step_weights="last:2", weight_rewards=True)


def _setting(k, opts):
    from marlclassification_amd import class_loss as cl

    return cl.from_options(k.cfg.nb_class, NS, **opts)
