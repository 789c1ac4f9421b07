"""GPU: autograd through single steps - ModelsWrapper.forward and MultiAgent.act are autograd nodes
(marl_step_forward_train / marl_step_backward), as every forward / act call of the reference adds to its
graph (networks/models.py:78-138, core/agent.py:40-68).  Gradients of the parameters and of the carried
message / recurrent state are checked against float64 autograd through the oracle, and the act loop
against the fused episode node (_EpisodeFunction)."""
import pytest
import torch as th
import torch.nn.functional as F

from oracle import marl_oracle as mo
from tests.util import Golden, uniform_params

pytestmark = pytest.mark.gpu

NS = 3
FWD_TOL = 1e-5   # forward outputs (x max(1, |ref|))
GRAD_TOL = 1e-4  # gradients (x max |ref|), the project's gradient tolerance
STRIDE3 = [[3, 0], [-3, 0], [0, 3], [0, -3]]

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


def _close(got, ref, tol, what):
    got = got.detach().double().cpu()
    # (no float64 gradient: the oracle's graph does not reach this tensor - Na = 1 has no message path)
    ref = th.zeros_like(got) if ref is None else ref.detach().double().cpu()
    assert got.shape == ref.shape, what
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    assert err <= tol * ref.abs().max().item() + 1e-7, f"{what}: max err {err:.3e} (ref max {ref.abs().max().item():.3e})"


def _close_fwd(got, ref, what):
    err = (got.detach().double().cpu() - ref.detach().double()).abs().max().item()
    assert err <= FWD_TOL * max(1.0, ref.abs().max().item()), f"{what}: max err {err:.3e}"


def _param_grads_match(model, p64, tol=GRAD_TOL):
    for k, p in model.named_parameters():
        assert p.grad is not None, f"{k}: no gradient"
        _close(p.grad, p64[k].grad, tol, k)


# ---- 1: ModelsWrapper.forward unrolled over 3 steps, every output in the loss ----------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_forward_unroll_matches_float64_oracle(device, name):
    from marlclassification_amd.networks.models import RecurrentOutput

    k = Case(name)
    c, na, nb = k.cfg, k.na, k.nb
    model = k.model(device)
    pos = [th.stack([th.randint(s - c.window, (na, nb), generator=k.gen) for s in k.sizes], -1) for _ in range(NS)]
    obs = [mo.crop_patches(k.img, p, c.window) for p in pos]
    npos = [mo.normalized_positions(p, k.sizes) for p in pos]
    i = k.inp
    st0 = [i.h0, i.c0, i.hc0, i.cc0, 0.5 * k.randn(na, nb, c.n_m)]
    widths = [c.nb_action, None, c.nb_class, c.n_m, c.n_b, c.n_b, c.n_a, c.n_a]
    ws = [[k.randn(na, nb, w) if w else k.randn(na, nb) for w in widths] for _ in range(NS)]

    # GPU: ModelsWrapper.forward, message and state chained
    leaves = [t.to(device).requires_grad_() for t in st0]
    h, cst, hc, cc, msg = leaves
    rec = RecurrentOutput(h, cst, hc, cc)
    loss, outs = 0.0, []
    for t in range(NS):
        out, rec = model(obs[t].to(device), msg, npos[t].to(device), rec)
        msg = out.messages
        o = (out.actions_probabilities, out.values, out.predictions, out.messages, rec.h, rec.c, rec.h_caret,
             rec.c_caret)
        assert all(x.grad_fn is not None for x in o)
        outs.append(o)
        loss = loss + sum((w.to(device) * x).sum() for w, x in zip(ws[t], o))
    loss.backward()

    # float64 oracle
    p64 = k.params64()
    leaves64 = [t.double().requires_grad_() for t in st0]
    h, cst, hc, cc, msg = leaves64
    loss64 = 0.0
    for t in range(NS):
        so = mo.step_forward(p64, c, obs[t].double(), msg, npos[t].double(), h, cst, hc, cc)
        h, cst, hc, cc, msg = so.h, so.c, so.hc, so.cc, so.msg
        o = (so.probs, so.values, so.preds, so.msg, so.h, so.c, so.hc, so.cc)
        for j, (g, r) in enumerate(zip(outs[t], o)):
            _close_fwd(g, r, f"step {t} output {j}")
        loss64 = loss64 + sum((w.double() * x).sum() for w, x in zip(ws[t], o))
    loss64.backward()

    _param_grads_match(model, p64)
    for n, g, r in zip(("h0", "c0", "hc0", "cc0", "msg0"), leaves, leaves64):
        _close(g.grad, r.grad, GRAD_TOL, n)


# ---- 2 / 3: MultiAgent.act loop ------------------------------------------------------------------------------
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


def _oracle_act_loop(k, p64):
    """The same loop in float64 (oracle run_episode with a float64 message)."""
    c, i = k.cfg, k.inp
    table = th.tensor(c.actions)
    pos = i.pos0
    h, cst, hc, cc = (t.double() for t in (i.h0, i.c0, i.hc0, i.cc0))
    msg = th.zeros(k.na, k.nb, c.n_m, dtype=th.float64)
    acc = {"preds": [], "logp": [], "values": [], "act": []}
    img = k.img.double()
    for t in range(NS):
        so = mo.step_forward(p64, c, mo.crop_patches(img, pos, c.window), msg,
                             mo.normalized_positions(pos, k.sizes).double(), h, cst, hc, cc)
        h, cst, hc, cc, msg = so.h, so.c, so.hc, so.cc, so.msg
        a = mo.sample_actions(so.probs, i.q[t].double())
        logp = th.gather(so.probs, -1, a.unsqueeze(-1)).squeeze(-1).log()
        pos = mo.transition(pos, a, table, c.window, k.sizes)
        for key, v in zip(acc, (so.preds, logp, so.values, a)):
            acc[key].append(v)
    return {key: th.stack(v) for key, v in acc.items()}


def _loss_terms(k):
    na, nb, c = k.na, k.nb, k.cfg
    adv = k.randn(NS, na, nb)
    y = th.randint(c.nb_class, (NS, na, nb), generator=k.gen)
    ret = k.randn(NS, na, nb)
    return adv, y, ret


def _a2c_like_loss(preds, logp, values, terms):
    adv, y, ret = (t.to(preds.device) for t in terms)
    ce = F.cross_entropy(preds.flatten(0, 2), y.flatten(), reduction="sum")
    return -(logp * adv.to(logp.dtype)).sum() + ce + F.mse_loss(values, ret.to(values.dtype), reduction="sum")


@pytest.mark.parametrize("name", list(CASES))
def test_act_loop_matches_float64_oracle(device, name):
    k = Case(name)
    model = k.model(device)
    terms = _loss_terms(k)
    out = _act_loop(k, model, device)
    assert out["logp"].grad_fn is not None and not out["act"].requires_grad
    _a2c_like_loss(out["preds"], out["logp"], out["values"], terms).backward()

    p64 = k.params64()
    tr = _oracle_act_loop(k, p64)
    assert th.equal(out["act"].cpu(), tr["act"]), "sampled actions differ from mo.sample_actions"
    for key in ("preds", "logp", "values"):
        _close_fwd(out[key], tr[key], key)
    _a2c_like_loss(tr["preds"], tr["logp"], tr["values"], terms).backward()
    _param_grads_match(model, p64)


@pytest.mark.parametrize("name", list(CASES))
def test_act_loop_gradients_equal_the_fused_episode(device, name):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.fused import EpisodeDraws

    k = Case(name)
    model = k.model(device)
    terms = _loss_terms(k)
    i = k.inp
    sampler = EpisodeSampler(MultiAgent(k.na, model), Environment(k.cfg.actions, k.cfg.window), NS)
    sampler.fixed_draws = EpisodeDraws(*(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0, i.q[:NS])))
    ep = sampler.run_episode(k.img.to(device))
    _a2c_like_loss(ep.step_preds, ep.step_log_probas, ep.step_values, terms).backward()
    g_ep = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)

    out = _act_loop(k, model, device)
    assert th.equal(out["pos"], ep.step_pos), "the act loop moved otherwise than the episode"
    _a2c_like_loss(out["preds"], out["logp"], out["values"], terms).backward()
    for n, p in model.named_parameters():
        _close(p.grad, g_ep[n], GRAD_TOL, n)


# ---- 5: the autograd node leaves the forward untouched -------------------------------------------------------
@pytest.mark.parametrize("name", ["g1", "wide"])
def test_forward_under_grad_equals_no_grad(device, name):
    from marlclassification_amd.networks.models import RecurrentOutput

    k = Case(name)
    model = k.model(device)
    i = k.inp
    obs = mo.crop_patches(k.img, i.pos0, k.cfg.window).to(device)
    npos = mo.normalized_positions(i.pos0, k.sizes).to(device)
    msg = k.randn(k.na, k.nb, k.cfg.n_m).to(device)
    rec = RecurrentOutput(*(t.to(device) for t in (i.h0, i.c0, i.hc0, i.cc0)))

    def flat(o, r):
        return (o.actions_probabilities, o.values, o.predictions, o.messages, r.h, r.c, r.h_caret, r.c_caret)

    with th.no_grad():
        ref = flat(*model(obs, msg, npos, rec))
    got = flat(*model(obs, msg, npos, rec))
    assert got[0].grad_fn is not None
    for a, b in zip(got, ref):
        assert th.equal(a.detach(), b)
    # act: same actions and log-probabilities with and without the graph
    outs = []
    for grad in (False, True):
        with th.set_grad_enabled(grad):
            outs.append(_act_loop(k, model, device))
    assert outs[1]["logp"].grad_fn is not None and outs[0]["logp"].grad_fn is None
    for key in outs[0]:
        assert th.equal(outs[0][key], outs[1][key].detach()), key


# ---- 6: guards -----------------------------------------------------------------------------------------------
def _one_step(k, model, device, nb=None):
    from marlclassification_amd.networks.models import RecurrentOutput

    nb = nb or k.nb
    i = k.inp
    obs = mo.crop_patches(k.img[:nb], i.pos0[:, :nb], k.cfg.window).to(device)
    npos = mo.normalized_positions(i.pos0[:, :nb], k.sizes).to(device)
    msg = th.zeros(k.na, nb, k.cfg.n_m, device=device)
    rec = RecurrentOutput(*(t[:, :nb].to(device) for t in (i.h0, i.c0, i.hc0, i.cc0)))
    out, rec = model(obs, msg, npos, rec)
    return out.predictions.sum() + out.values.sum() + rec.h.square().sum() + out.messages.sum()


def test_guards(device):
    k = Case("g1")
    model = k.model(device)
    eng = model.hip_engine(None)

    # reference gradients of one step
    _one_step(k, model, device).backward()
    ref = {n: p.grad.clone() for n, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)

    # a second backward: the workspace went back to the pool at the first
    loss = _one_step(k, model, device)
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="already released"):
        loss.backward()
    model.zero_grad(set_to_none=True)

    # an optimiser step between forward and backward
    loss = _one_step(k, model, device)
    p0 = next(model.parameters())
    p0.grad = th.ones_like(p0)
    th.optim.SGD([p0], lr=0.1).step()
    with pytest.raises(RuntimeError):
        loss.backward()
    model.load_state_dict(k.params)
    model.zero_grad(set_to_none=True)

    # weights re-packed between forward and backward
    loss = _one_step(k, model, device)
    eng.pack(model.flat_state().param_views())
    with pytest.raises(RuntimeError, match="re-packed"):
        loss.backward()
    model.zero_grad(set_to_none=True)

    # another configuration in between is switched back for the backward
    loss = _one_step(k, model, device)
    with th.no_grad():
        _one_step(k, model, device, nb=k.nb - 2)
    loss.backward()
    for n, p in model.named_parameters():
        assert th.equal(p.grad, ref[n]), n
    model.zero_grad(set_to_none=True)

    # observation / positions that require grad are refused
    from marlclassification_amd.networks.models import RecurrentOutput

    i = k.inp
    obs = mo.crop_patches(k.img, i.pos0, k.cfg.window).to(device).requires_grad_()
    npos = mo.normalized_positions(i.pos0, k.sizes).to(device)
    rec = RecurrentOutput(*(t.to(device) for t in (i.h0, i.c0, i.hc0, i.cc0)))
    msg = th.zeros(k.na, k.nb, k.cfg.n_m, device=device)
    with pytest.raises(RuntimeError, match="requires grad"):
        model(obs, msg, npos, rec)
    with pytest.raises(RuntimeError, match="requires grad"):
        model(obs.detach(), msg, npos.requires_grad_(), rec)
    npos = npos.detach()

    # no graph without grad mode, or with nothing that requires grad
    with th.no_grad():
        out, r = model(obs.detach(), msg, npos, rec)
    assert out.predictions.grad_fn is None and r.h.grad_fn is None
    for p in model.parameters():
        p.requires_grad_(False)
    out, r = model(obs.detach(), msg, npos, rec)
    assert out.predictions.grad_fn is None
    for p in model.parameters():
        p.requires_grad_(True)

    # a step whose graph is dropped without backward gives its workspace back to the pool
    from marlclassification_amd import engine

    key = (eng._cfg_key, engine._tune_epoch)
    eng._ws_pool.get(key, []).clear()
    loss = _one_step(k, model, device)
    assert len(eng._ws_pool.get(key, [])) == 0
    del loss
    assert len(eng._ws_pool.get(key, [])) == 1
