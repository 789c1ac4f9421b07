"""The cases of the GPU parity tests and what builds an episode from one: the named shapes (``Case`` and its
subclasses), the samplers with fixed draws, the float64 oracle loop, the A2C-like and distribution losses, teacher
forcing, and the two-epoch PPO reference.  Host tests import this module too, so everything of the package is imported
inside the functions that need it."""
import os

import torch as th
import torch.nn.functional as F

from oracle import marl_oracle as mo
from tests import loss_ref, util
from tests.loss_ref import masked_entropy  # noqa: F401  (the entropy of _dist_loss; test files take it from here too)
from tests.util import Golden, model_spec, uniform_params

NS = 3
NS4 = 4  # the range-limited and exploration cases: three exchanges that carry a message
STRIDE3 = [[3, 0], [-3, 0], [0, 3], [0, -3]]
POL_BIAS = "_ModelsWrapper__policy.3.bias"

# name -> (config, Na, Nb, image [C, H, W], seed); "g1" takes everything from the g1_conftest fixture
CASES = {
    "g1": None,
    "resisc3": (mo.OracleConfig("resisc45", 12, 32, 32, 8, 12, 8, 10, 48, 48), 3, 4, (3, 40, 40), 11),
    "aid4": (mo.OracleConfig("aid", 16, 32, 32, 8, 12, 8, 5, 48, 48, actions=STRIDE3), 3, 4, (3, 48, 48), 12),
    "na1": (mo.OracleConfig("mnist", 12, 23, 22, 21, 20, 19, 10, 24, 25), 1, 5, (1, 28, 28), 13),
    # nA = 6 and nla = 400: the heads' backward without the rank-kin LayerNorm kernel (and, with nla past
    # the panel limit, the unfused message chain)
    "wide": (mo.OracleConfig("mnist", 12, 23, 22, 21, 20, 19, 10, 24, 400,
                             actions=[[1, 0], [-1, 0], [0, 1], [0, -1], [0, 0], [2, 2]]), 2, 5, (1, 28, 28), 14),
}
# the communication shapes; "g1" is the g1_conftest fixture (Na = 5, odd dimensions)
EXTRA = {
    "g2": (util.CASES["g2_mnist_c1"], 3, 6, (1, 28, 28), 21),
    "resisc16": (util.CASES["g4_resisc_b2"], 16, 2, (3, 48, 48), 22),
}
# "na20": twenty agents - past the chained panel launch (16 rows), so every family takes mix_msg_gated_kernel<32>
WIDE = {"na20": (util.CASES["g1_conftest"], 20, 3, (1, 28, 28), 23)}


class Case:
    def __init__(self, name):
        if CASES[name] is None:
            g = Golden("g1_conftest")
            self.cfg, self.na, self.nb, self.params, self.img = g.cfg, g.na, g.nb, g.params, g.img
            self.inp = g.inp
            seed = 10
        else:
            self.cfg, self.na, self.nb, shape, seed = CASES[name]
            self.params = uniform_params(self.cfg, seed)
            self.img = th.rand(self.nb, *shape, generator=th.Generator().manual_seed(seed))
            self.inp = mo.draw_episode_inputs(self.cfg, self.na, self.nb, NS, list(shape[1:]), seed)
        self.gen = th.Generator().manual_seed(seed + 1000)
        self.sizes = list(self.img.shape[2:])

    def randn(self, *shape):
        return th.randn(*shape, generator=self.gen)

    def model(self, device):
        from marlclassification_amd.networks import ModelsWrapper
        from marlclassification_amd.networks.vision import AidCnn, MnistCnn, Resisc45Cnn

        c = self.cfg
        cnn = {"mnist": MnistCnn, "resisc45": Resisc45Cnn, "aid": AidCnn}[c.ft_extr](c.window)
        m = ModelsWrapper(cnn, c.n_b, c.n_a, c.n_m, c.n_m_o, c.n_d, 2, c.nb_action, c.nb_class, c.nlb, c.nla)
        m.load_state_dict(self.params)
        return m.to(device)

    def params64(self):
        return {k: v.double().requires_grad_() for k, v in self.params.items()}


class CommCase(Case):
    def __init__(self, name):
        if name in CASES:
            super().__init__(name)
            return
        self.cfg, self.na, self.nb, shape, seed = EXTRA[name]
        self.params = uniform_params(self.cfg, seed)
        self.img = th.rand(self.nb, *shape, generator=th.Generator().manual_seed(seed))
        self.inp = mo.draw_episode_inputs(self.cfg, self.na, self.nb, NS, list(shape[1:]), seed)
        self.gen = th.Generator().manual_seed(seed + 1000)
        self.sizes = list(self.img.shape[2:])


def inputs4(k, seed):
    """The case's random draws for NS4 = 4 steps (the fixtures carry three)."""
    k.inp = mo.draw_episode_inputs(k.cfg, k.na, k.nb, NS4, k.sizes, seed)
    return k


class RangeCase(CommCase):
    def __init__(self, name):
        if name in WIDE:
            self.cfg, self.na, self.nb, shape, seed = WIDE[name]
            self.params = uniform_params(self.cfg, seed)
            self.img = th.rand(self.nb, *shape, generator=th.Generator().manual_seed(seed))
            self.gen = th.Generator().manual_seed(seed + 1000)
            self.sizes = list(self.img.shape[2:])
        else:
            super().__init__(name)
        inputs4(self, {"g1": 10, "g2": 21, "resisc16": 22, "na1": 13, "na20": 23}[name])


# ---- episodes ------------------------------------------------------------------------------------------------------
def _sampler(k, model, device, probs=True, ns=NS):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.fused import EpisodeDraws

    i = k.inp
    sampler = EpisodeSampler(MultiAgent(k.na, model), Environment(k.cfg.actions, k.cfg.window), ns)
    sampler.fixed_draws = EpisodeDraws(*(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0, i.q[:ns])))
    sampler.return_probs = probs
    return sampler


def sampler4(k, model, device, probs=True):
    return _sampler(k, model, device, probs, NS4)


def _golden_sampler(g, device):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.fused import EpisodeDraws
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import MnistCnn

    c = g.cfg
    model = ModelsWrapper(MnistCnn(c.window), c.n_b, c.n_a, c.n_m, c.n_m_o, c.n_d, 2,
                          c.nb_action, c.nb_class, c.nlb, c.nla)
    model.load_state_dict(g.params)
    model.to(device)
    sampler = EpisodeSampler(MultiAgent(g.na, model), Environment(c.actions, c.window), g.ns)
    i = g.inp
    sampler.fixed_draws = EpisodeDraws(*(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0, i.q)))
    return model, sampler


def _engine_episode(k, device):
    from marlclassification_amd.engine import HipEngine

    eng = HipEngine(model_spec(k.cfg), device)
    eng.configure(k.na, k.nb, NS, k.img.shape[1:])
    eng.pack({n: v.to(device) for n, v in k.params.items()})
    i = k.inp
    out = eng.episode_forward(k.img.to(device), *(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0, i.q[:NS])),
                              None, True, probs=True)
    return eng, out


def _oracle_loop(k, p64, img64, forced=None, ns=NS):
    """The episode in float64: the oracle's step loop with the crops taken from ``img64`` (may require grad), the
    distributions, the actions and teacher forcing (``forced``: the actions to take instead of the sampled ones)."""
    c, i = k.cfg, k.inp
    table = th.tensor(c.actions)
    pos = i.pos0
    h, cst, hc, cc = (t.double() for t in (i.h0, i.c0, i.hc0, i.cc0))
    msg = th.zeros(k.na, k.nb, c.n_m, dtype=th.float64)
    acc = {"preds": [], "logp": [], "values": [], "pos": [], "probs": [], "act": []}
    for t in range(ns):
        so = mo.step_forward(p64, c, mo.crop_patches(img64, pos, c.window), msg,
                             mo.normalized_positions(pos, k.sizes).double(), h, cst, hc, cc)
        h, cst, hc, cc, msg = so.h, so.c, so.hc, so.cc, so.msg
        a = mo.sample_actions(so.probs, i.q[t].double()) if forced is None else forced[t]
        logp = th.gather(so.probs, -1, a.unsqueeze(-1)).squeeze(-1).log()
        pos = mo.transition(pos, a, table, c.window, k.sizes)
        for key, v in zip(acc, (so.preds, logp, so.values, pos, so.probs, a)):
            acc[key].append(v)
    return {key: th.stack(v) for key, v in acc.items()}


def _act_loop(k, model, device):
    from marlclassification_amd.core import Environment, MultiAgent
    from marlclassification_amd.networks.models import RecurrentOutput

    i = k.inp
    agents, env = MultiAgent(k.na, model), Environment(k.cfg.actions, k.cfg.window)
    env.place(k.img.to(device), k.na, positions=i.pos0.to(device))
    obs = env.observe()
    agents.reset(k.nb)
    agents._MultiAgent__hidden = RecurrentOutput(*(t.to(device) for t in (i.h0, i.c0, i.hc0, i.cc0)))
    acc = {"preds": [], "logp": [], "values": [], "act": [], "pos": []}
    for t in range(NS):
        agents.fixed_noise = i.q[t].to(device)
        o = agents.act(obs, env.normalized_positions)
        obs = env.step(o.actions)
        for key, v in zip(acc, (o.predictions, o.actions_log_probs, o.values, o.actions, env.positions)):
            acc[key].append(v)
    return {key: th.stack(v) for key, v in acc.items()}


# ---- losses --------------------------------------------------------------------------------------------------------
def _loss_terms(k, ns=NS):
    na, nb, c = k.na, k.nb, k.cfg
    adv = k.randn(ns, na, nb)
    y = th.randint(c.nb_class, (ns, na, nb), generator=k.gen)
    ret = k.randn(ns, na, nb)
    return adv, y, ret


def loss_terms4(k):
    return _loss_terms(k, NS4)


def _a2c_like_loss(preds, logp, values, terms):
    adv, y, ret = (t.to(preds.device) for t in terms)
    ce = F.cross_entropy(preds.flatten(0, 2), y.flatten(), reduction="sum")
    return -(logp * adv.to(logp.dtype)).sum() + ce + F.mse_loss(values, ret.to(values.dtype), reduction="sum")


def _dist_loss(preds, logp, values, probs, terms, w, only_probs=False):
    """An A2C-like loss + an entropy bonus + a fixed random linear form of the distributions (a general g_probs)."""
    dist = -0.37 * masked_entropy(probs).sum(0).mean() + (w.to(probs.device, probs.dtype) * probs).sum()
    return dist if only_probs else _a2c_like_loss(preds, logp, values, terms) + dist


# ---- communication -------------------------------------------------------------------------------------------------
def _family():
    """The kernel family of this process (variables read once per process; a child process of another family keeps a
    record of its own)."""
    return "panels0" if os.environ.get("MARL_PANELS") == "0" else (
        "chain0" if os.environ.get("MARL_PANEL_CHAIN") == "0" else "default")


def dense(na, seed=5):
    """Seeded dense asymmetric matrix with self-loops and (at least) one negative entry."""
    m = th.randn(na, na, generator=th.Generator().manual_seed(seed)) / max(1.0, na ** 0.5)
    m[0, na - 1] = -abs(m[0, na - 1]) - 0.1
    m[na - 1, 0] = abs(m[na - 1, 0]) + 0.2
    assert not th.equal(m, m.t()) and (m.diagonal() != 0).all() and (m < 0).any(), "dense(): not the matrix promised"
    return m


def graph(name, na):
    from marlclassification_amd import comm

    if name == "ring":
        return comm.ring(na, 1)
    if name == "star":
        return comm.star(na, na // 2)
    if name == "none":
        return comm.none(na)
    if name == "teams":
        return comm.teams([2, na - 2]) if na > 2 else comm.teams([1] * na)
    return dense(na)


def _replay(sampler, actions, device):
    from marlclassification_amd.core.episode import Trajectory

    return Trajectory(sampler.fixed_draws, actions.to(device))


def _force(sampler, actions, device):
    """Teacher-forces the trainer's rollouts: run_episode_raw with the fixed draws and the oracle's actions."""
    raw = sampler.run_episode_raw
    forced = actions.to(device)

    def run(x, train, draws=None, probs=False, forced_=None, **kw):
        f = kw.get("forced", forced_)
        return raw(x, train, draws=sampler.fixed_draws if draws is None else draws, probs=probs,
                   forced=forced if f is None else f)
    sampler.run_episode_raw = run


def _case_with_loss(name):
    k = CommCase(name)
    k.name = name
    k.terms = _loss_terms(k)
    k.w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    return k


def _run(k, model, device, actions=None):
    """One episode under ``k.terms`` / ``k.w`` + backward: outputs, actions, image and parameter gradients"""
    sampler = _sampler(k, model, device)
    img = k.img.to(device).requires_grad_()
    replay = None if actions is None else _replay(sampler, actions, device)
    ep = sampler.run_episode(img, replay=replay)
    _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, k.terms, k.w).backward()
    res = {"preds": ep.step_preds.detach().clone(), "logp": ep.step_log_probas.detach().clone(),
           "values": ep.step_values.detach().clone(), "probs": ep.step_probs.detach().clone(),
           "act": ep.step_actions.clone(), "d_img": img.grad.clone()}
    res.update({n: p.grad.clone() for n, p in model.named_parameters()})
    model.zero_grad(set_to_none=True)
    return res


def _run4(k, model, device, actions=None, draws=None):
    """``_run`` over NS4 steps (``draws``: in place of the case's fixed ones); the parameters' gradients flattened."""
    sampler = sampler4(k, model, device)
    if draws is not None:
        sampler.fixed_draws = draws
    img = k.img.to(device).requires_grad_()
    replay = None if actions is None else _replay(sampler, actions, device)
    ep = sampler.run_episode(img, replay=replay)
    _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, k.terms, k.w).backward()
    res = {"preds": ep.step_preds.detach().clone(), "logp": ep.step_log_probas.detach().clone(),
           "values": ep.step_values.detach().clone(), "probs": ep.step_probs.detach().clone(),
           "act": ep.step_actions.clone(), "pos": ep.step_pos.clone(), "d_img": img.grad.clone(),
           "flat_grad": th.cat([p.grad.flatten() for _, p in model.named_parameters()])}
    model.zero_grad(set_to_none=True)
    return res


def _unroll_inputs(k):
    c, na, nb = k.cfg, k.na, k.nb
    pos = [th.stack([th.randint(s - c.window, (na, nb), generator=k.gen) for s in k.sizes], -1) for _ in range(NS)]
    obs = [mo.crop_patches(k.img, p, c.window) for p in pos]
    npos = [mo.normalized_positions(p, k.sizes) for p in pos]
    i = k.inp
    st0 = [i.h0, i.c0, i.hc0, i.cc0, 0.5 * k.randn(na, nb, c.n_m)]
    widths = [c.nb_action, None, c.nb_class, c.n_m, c.n_b, c.n_b, c.n_a, c.n_a]
    ws = [[k.randn(na, nb, w) if w else k.randn(na, nb) for w in widths] for _ in range(NS)]
    return obs, npos, st0, ws


def _unroll(k, model, device, obs, npos, st0, ws):
    """ModelsWrapper.forward over NS steps, message and state chained, every output in the loss; returns the
    outputs and the gradients of the initial state / message."""
    from marlclassification_amd.networks.models import RecurrentOutput

    leaves = [t.to(device).requires_grad_() for t in st0]
    h, cst, hc, cc, msg = leaves
    rec = RecurrentOutput(h, cst, hc, cc)
    loss, outs = 0.0, []
    for t in range(NS):
        out, rec = model(obs[t].to(device), msg, npos[t].to(device), rec)
        msg = out.messages
        o = (out.actions_probabilities, out.values, out.predictions, out.messages, rec.h, rec.c, rec.h_caret,
             rec.c_caret)
        outs.append(o)
        loss = loss + sum((w.to(device) * x).sum() for w, x in zip(ws[t], o))
    loss.backward()
    return outs, [g.grad for g in leaves]


# ---- two PPO epochs in float64 -------------------------------------------------------------------------------------
# epsilon of the two-epoch tests: the first Adam step (lr = 1e-3, every parameter moves by lr) spreads the float64
# reference's ratios over [0.65, 1.53]; at 0.1 it clips 23.5 % (g1) and 33.3 % (resisc3) of the entries in epoch 2 and
# the nearest ratio stays 6.1e-4 / 5.7e-3 from a bound (scanned on the CPU; the tests assert >= 1e-4 again)
TWO_EPOCH_EPS = {"g1": 0.1, "resisc3": 0.1}
TWO_EPOCH = {"lr": 1e-3, "gamma": 0.99, "lam": 0.9, "beta": 0.05}


def _y(k):
    return th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)


def _grads_of(p):
    return {n: (v.grad if v.grad is not None else th.zeros_like(v)) for n, v in p.items()}


def two_epoch_reference(k, y, eps):
    """Two PPO epochs on one batch in float64: oracle loop -> advantages and the loss at rho = 1 -> Adam 1 -> the
    loop again under the updated parameters with the sampled actions forced -> the loss against the stored old
    log-probabilities -> Adam 2 with carried moments."""
    lr, gamma, lam, beta = (TWO_EPOCH[n] for n in ("lr", "gamma", "lam", "beta"))
    img64 = k.img.double()
    p = k.params64()
    tr = _oracle_loop(k, p, img64)
    advn, ret, _ = loss_ref.advantages(tr["preds"], tr["values"], y, gamma, lam)
    old_logp = tr["logp"].detach()
    loss, sc1, _, _ = loss_ref.ppo(tr["preds"], tr["logp"], tr["values"], tr["probs"], y, old_logp, advn, ret, eps,
                                   beta)
    loss.backward()
    g1 = _grads_of(p)
    after = {n: v.detach().clone() for n, v in p.items()}
    m = {n: th.zeros_like(v) for n, v in after.items()}
    v2 = {n: th.zeros_like(v) for n, v in after.items()}
    mo.adam_step(after, g1, m, v2, 1, lr)
    p2 = {n: v.clone().requires_grad_() for n, v in after.items()}
    tr2 = _oracle_loop(k, p2, img64, forced=tr["act"])
    assert th.equal(tr2["pos"], tr["pos"]), "the forced loop moved otherwise than the sampled one"
    loss2, sc2, rho, clipped = loss_ref.ppo(tr2["preds"], tr2["logp"], tr2["values"], tr2["probs"], y, old_logp, advn,
                                            ret, eps, beta)
    loss2.backward()
    g2 = _grads_of(p2)
    mo.adam_step(after, g2, m, v2, 2, lr)
    return {"tr": tr, "after": after, "g1": g1, "g2": g2, "scalars1": sc1, "scalars2": sc2, "rho": rho,
            "clipped": clipped}
