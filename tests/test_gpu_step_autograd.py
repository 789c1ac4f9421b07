"""GPU: autograd through single steps - ModelsWrapper.forward and MultiAgent.act are autograd nodes
(marl_step_forward_train / marl_step_backward), as every forward / act call of the reference adds to its
graph (networks/models.py:78-138, core/agent.py:40-68).  Gradients of the parameters and of the carried
message / recurrent state are checked against float64 autograd through the oracle, and the act loop
against the fused episode node (_EpisodeFunction)."""
import pytest
import torch as th

from oracle import marl_oracle as mo
from tests.cases import CASES, NS, Case, _a2c_like_loss, _act_loop, _loss_terms
from tests.parity import GRAD_TOL
from tests.parity import close as _close
from tests.parity import close_fwd as _close_fwd
from tests.parity import param_grads_match as _param_grads_match

pytestmark = pytest.mark.gpu


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
