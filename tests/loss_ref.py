"""The float64 reference of the fused loss, written from the oracle's pieces: rewards -> returns or GAE(lambda) ->
standardise, the vote error, the A2C path term or PPO's clipped surrogate (``torch.minimum`` / ``clamp``),
``smooth_l1_loss`` and the entropy bonus (training/trainer.py:76-111).

``c`` is a ``class_loss.ClassLoss`` (class weights, label smoothing, step weights, weighted rewards), ``q`` a target
distribution per image [Nb, nC].  With neither, the vote error is ``F.cross_entropy`` on the agent-mean logits and the
rewards are the oracle's ``classification_rewards`` - nothing of the package's ``class_loss`` module is read; with
either, they are ``class_loss.vote_error`` / ``class_loss.rewards`` (held to torch by tests/test_class_loss_host.py and
tests/test_mix_host.py)."""
import torch as th
import torch.nn.functional as F

from oracle import marl_oracle as mo


def masked_entropy(p):
    """H = -sum_j p_j log p_j over the last dimension with 0 log 0 = 0: a zero probability adds nothing and gets a
    zero gradient (Categorical.entropy clamps instead; the naive sum is NaN there)."""
    safe = th.where(p > 0, p, th.ones_like(p))
    return -(p * safe.log()).sum(-1)


def gae(rewards, values, gamma, lam):
    """Plain GAE(lambda) over dimension 0, V_Ns = 0 (no bootstrap): delta_t = r_t + gamma V_{t+1} - V_t,
    A_t = delta_t + gamma lam A_{t+1}.  Returns (A, A + V)."""
    ns = rewards.shape[0]
    adv = th.zeros_like(rewards)
    nxt_a = th.zeros_like(rewards[0])
    nxt_v = th.zeros_like(values[0])
    for t in range(ns - 1, -1, -1):
        delta = rewards[t] + gamma * nxt_v - values[t]
        nxt_a = delta + gamma * lam * nxt_a
        adv[t] = nxt_a
        nxt_v = values[t]
    return adv, adv + values


def ratio_deltas(shape):
    """old_logp = logp - delta with delta on a fixed grid over [-0.5, 0.5], permuted by a fixed stride so that
    neighbouring entries differ: rho = exp(delta) spans [0.607, 1.649] on both sides of 1 +- eps."""
    n = 1
    for d in shape:
        n *= d
    i = (th.arange(n, dtype=th.float64) * 37) % n
    return (i / max(n - 1, 1) - 0.5).view(*shape)


def _t(v):
    return None if v is None else th.tensor(v, dtype=th.float64)


def _opts(c):
    if c is None:
        return None, 0.0, None, False
    return _t(c.class_weights), c.label_smoothing, _t(c.step_weights), c.weight_rewards


def error(preds, y, c=None, q=None):
    """[Ns, 1, Nb], as the reference's error term broadcasts over the agents."""
    if c is None and q is None:
        ns, _, nb, _ = preds.shape
        return F.cross_entropy(preds.mean(dim=1).flatten(0, 1), y.unsqueeze(0).repeat(ns, 1).flatten(0, 1),
                               reduction="none").unflatten(0, (ns, 1, nb))
    from marlclassification_amd import class_loss as cl

    w, eps, sw, _ = _opts(c)
    return cl.vote_error(preds, y, w, eps, sw, targets=None if q is None else q.double()).unsqueeze(1)


def rewards(preds, y, c=None, q=None):
    if c is None and q is None:
        return mo.classification_rewards(preds.detach(), y)
    from marlclassification_amd import class_loss as cl

    w, _, _, wrew = _opts(c)
    return cl.rewards(preds.detach(), y, w if wrew else None, targets=None if q is None else q.double())


def a2c(preds, logp, values, probs, y, gamma, beta, c=None, q=None):
    """training/trainer.py:76-111; returns (loss, scalars[5]: loss, path, error, critic, entropy)."""
    err = error(preds, y, c, q)
    returns = mo.discounted_returns(rewards(preds, y, c, q), gamma)
    adv = mo.standardize(returns - values.detach())
    path = -logp * adv
    critic = F.smooth_l1_loss(values, returns, reduction="none")
    ent = masked_entropy(probs) if beta > 0 else th.zeros_like(logp)
    loss = th.sum(path + err + critic, 0).mean() - beta * ent.sum(0).mean()
    return loss, th.stack([loss, path.sum(0).mean(), err.mean(), critic.sum(0).mean(), ent.mean()]).detach()


def advantages(preds, values, y, gamma, lam, c=None, q=None):
    """(standardised advantage, critic target, raw advantage): rewards -> GAE(lam) -> standardise, all detached."""
    adv, ret = gae(rewards(preds, y, c, q), values.detach(), gamma, lam)
    return mo.standardize(adv), ret, adv


def clip_mask(rho, advn, eps):
    return ((advn > 0) & (rho > 1 + eps)) | ((advn < 0) & (rho < 1 - eps))


def ppo(preds, logp, values, probs, y, old_logp, advn, ret, eps, beta, c=None, q=None):
    """The loss of marl_ppo_loss_fwd_bwd (the path term replaced by the clipped surrogate); returns (loss, scalars[7]:
    loss, surrogate, error, critic, entropy, approx_kl, clip_frac; the ratios; the mask of the clipped entries)."""
    err = error(preds, y, c, q)
    rho = (logp - old_logp).exp()
    surr = -th.minimum(rho * advn, rho.clamp(1 - eps, 1 + eps) * advn)
    critic = F.smooth_l1_loss(values, ret, reduction="none")
    ent = masked_entropy(probs) if beta > 0 else th.zeros_like(logp)
    loss = th.sum(surr + err + critic, 0).mean() - beta * ent.sum(0).mean()
    clipped = clip_mask(rho.detach(), advn, eps)
    scalars = th.stack([loss, surr.sum(0).mean(), err.mean(), critic.sum(0).mean(), ent.mean(),
                        (old_logp - logp).mean(), clipped.double().mean()]).detach()
    return loss, scalars, rho.detach(), clipped


def assert_clear_of_bounds(rho, eps):
    for bound in (1 - eps, 1 + eps):
        gap = (rho - bound).abs().min().item()
        assert gap >= 1e-4, f"a reference ratio lies {gap:.2e} from {bound}: fp32 could clip it otherwise"


class under:
    """``with under(eng, c):`` - the engine's loss calls run under ``c`` (None: nothing installed)."""

    def __init__(self, eng, c):
        self.eng, self.c = eng, c

    def __enter__(self):
        self.eng.set_class_loss(self.c)

    def __exit__(self, *exc):
        self.eng.set_class_loss(None)


class soft:
    """``with soft(eng, q):`` - the engine's loss calls run under the targets ``q`` (None: the labels)."""

    def __init__(self, eng, q):
        self.eng, self.q = eng, q

    def __enter__(self):
        self.eng.set_soft_targets(self.q)

    def __exit__(self, *exc):
        self.eng.set_soft_targets(None)
