"""GPU: the gradient with respect to the mixing matrix (``marl_comm_grad``) - through the fused episode node, the step
nodes, ``comm.LearnableComm``, the trainers (``comm_lr``), PPO replay and two data-parallel ranks.

The float64 reference is the oracle's step loop (tests/cases.py::_oracle_loop) with
``marl_oracle.aggregate_messages`` replaced by ``einsum(M64.requires_grad_(), m)``, teacher-forced: autograd's
``M64.grad`` is what ``d_comm`` must be.  Tolerances are the project's: gradients ``GRAD_TOL`` = 1e-4 of the tensor's
scale (here max |dM|), Adam updates 1e-3 * lr per update (tests/parity.py).  Achieved errors go through its ``Recorder``
(``comm_grad_errors``)."""
import os
import subprocess
import sys

import pytest
import torch as th

from marlclassification_amd import comm
from oracle import marl_oracle as mo
from tests import loss_ref as ref64
from tests import util
from tests.cases import (NS, TWO_EPOCH, TWO_EPOCH_EPS, CommCase, _a2c_like_loss, _act_loop, _case_with_loss, _dist_loss,
                         _family, _force, _golden_sampler, _grads_of, _loss_terms, _oracle_loop, _replay, _run,
                         _sampler, _unroll, _unroll_inputs, _y, dense, graph)
from tests.dp import run_ranks
from tests.loss_ref import assert_clear_of_bounds
from tests.parity import GRAD_TOL, Recorder
from tests.util import uniform_params

pytestmark = pytest.mark.gpu

REC = Recorder("comm_grad_errors", "comm_grad", _family())
REC_COMM = Recorder("comm_errors", "comm", _family())  # (the PPO test's model update: tests/test_gpu_comm.py's record)

GRAPHS = ("ring", "star", "teams", "dense")
# (shape, graph): Na = 5 / 3 / 16 on the MNIST, RESISC45 and AID shapes, and one agent (a 1 x 1 matrix)
D_CASES = [(s, g) for s in ("g1", "g2", "resisc16", "resisc3", "aid4") for g in GRAPHS] + [("na1", "zero"),
                                                                                            ("na1", "half")]
# the kernel's other regimes: more than 1024 (step, batch) pairs, so that a workgroup owns SEVERAL pairs and its range
# crosses a step boundary (the flagship shape runs 4 pairs per workgroup), and more than 16 agents, so that a thread
# owns several entries of the matrix (up to four at the limit of 32 agents)
BIG = {
    "pairs2100": (util.CASES["g2_mnist_c1"], 3, 700, (1, 28, 28), 31),   # 2100 pairs: 3 per workgroup
    "pairs1251": (util.CASES["g1_conftest"], 5, 417, (1, 28, 28), 32),   # 1251 pairs: 2 per workgroup, a ragged tail
    "na20": (util.CASES["g1_conftest"], 20, 4, (1, 28, 28), 33),         # 400 entries: two per thread
    "na32": (util.CASES["g2_mnist_c1"], 32, 344, (1, 28, 28), 34),       # 1024 entries: four per thread; 1032 pairs
}
D_CASES += [(s, g) for s in BIG for g in ("ring", "dense")]


class BigCase(CommCase):
    def __init__(self, name):
        self.cfg, self.na, self.nb, shape, seed = BIG[name]
        self.params = uniform_params(self.cfg, seed)
        self.img = th.rand(self.nb, *shape, generator=th.Generator().manual_seed(seed))
        self.inp = mo.draw_episode_inputs(self.cfg, self.na, self.nb, NS, list(shape[1:]), seed)
        self.gen = th.Generator().manual_seed(seed + 1000)
        self.sizes = list(self.img.shape[2:])


def _case(name):
    return BigCase(name) if name in BIG else CommCase(name)


def _matrix(gname, na):
    if gname in ("zero", "half"):
        return th.tensor([[0.0 if gname == "zero" else 0.5]])
    return graph(gname, na)


def _grad(tag, got, ref):
    assert got is not None, f"{tag}: no gradient"
    REC.grad(tag, got, ref)


@pytest.fixture
def oracle_live(monkeypatch):
    """aggregate_messages of the float64 oracle under a matrix that requires grad: ``use(fn)`` installs the einsum
    with whatever ``fn()`` returns at call time (a float64 [Na, Na] tensor attached to its graph)."""
    def use(fn):
        monkeypatch.setattr(mo, "aggregate_messages", lambda msg: th.einsum("ac,cbk->abk", fn().to(msg.dtype), msg))
    return use


def _oracle_dm(k, m, oracle_live, terms, w):
    """(the teacher-forcing trace, float64 dL/dM) of the A2C-like loss plus the distribution term."""
    m64 = m.double().cpu().clone().requires_grad_()
    oracle_live(lambda: m64)
    tr = _oracle_loop(k, k.params64(), k.img.double())
    _dist_loss(tr["preds"], tr["logp"], tr["values"], tr["probs"], terms, w).backward()
    return tr, m64.grad


def _episode_dm(k, model, source, device, actions, terms, w, img_grad=False):
    """run_episode under the live ``source`` + backward of the same loss; returns the episode's image leaf."""
    model.set_comm(source)
    sampler = _sampler(k, model, device)
    img = k.img.to(device)
    if img_grad:
        img.requires_grad_()
    ep = sampler.run_episode(img, replay=_replay(sampler, actions, device))
    assert th.equal(ep.step_actions.cpu(), actions)
    assert ep.step_preds.grad_fn is not None
    _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, terms, w).backward()
    return img


# ---- 1: d_comm against the float64 oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("shape,gname", D_CASES)
def test_d_comm_matches_float64_oracle(device, oracle_live, shape, gname):
    k = _case(shape)
    m = _matrix(gname, k.na)
    terms = _loss_terms(k)
    w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    tr, ref = _oracle_dm(k, m, oracle_live, terms, w)
    live = m.to(device).requires_grad_()
    _episode_dm(k, k.model(device), live, device, tr["act"], terms, w)
    assert live.grad is not None and live.grad.shape == m.shape and live.grad.dtype == th.float32
    _grad(f"{_family()}/{shape}/{gname}/d_comm", live.grad, ref)
    if k.na > 1:
        assert ref.abs().max().item() > 0.0, "the reference gradient must not vanish"


@pytest.mark.parametrize("env", [{"MARL_PANEL_CHAIN": "0"}, {"MARL_PANELS": "0"}])
def test_d_comm_in_the_other_kernel_families(device, env):
    """DAD1 and the messages are written by every family of the backward (chained panels by default; the unchained
    panels; the GEMM + row-kernel path): every oracle case again in a child process, and the step loop."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_gpu_comm_grad.py"), "-x",
                        "-q", "-m", "gpu", "-k", "test_d_comm_matches_float64_oracle or test_step_loop", "-s",
                        "-p", "no:cacheprovider"],
                       env=dict(os.environ, **env), cwd=root, capture_output=True, text=True, timeout=1500)
    print("\n".join(line for line in r.stdout.splitlines() if line.startswith("[comm_grad]")))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


# ---- 2: the gradient is dense ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,gname", [("g1", "ring"), ("resisc16", "teams")])
def test_entries_where_the_matrix_is_zero_carry_the_oracles_gradient(device, oracle_live, shape, gname):
    k = CommCase(shape)
    m = graph(gname, k.na)
    terms = _loss_terms(k)
    w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    tr, ref = _oracle_dm(k, m, oracle_live, terms, w)
    live = m.to(device).requires_grad_()
    _episode_dm(k, k.model(device), live, device, tr["act"], terms, w)
    zero = m == 0
    got0, ref0 = live.grad.cpu()[zero].double(), ref[zero]
    assert zero.any() and (ref0 != 0).all(), "the oracle's gradient is non-zero where M is 0"
    assert (got0 != 0).all()
    err = (got0 - ref0).abs().max().item()
    REC.rec(f"dense/{shape}/{gname}", got0, ref0, GRAD_TOL)
    assert err <= GRAD_TOL * ref.abs().max().item() + 1e-7, f"max err {err:.3e} on the entries where M == 0"
    assert ref0.abs().max().item() > 100 * GRAD_TOL * ref.abs().max().item(), "the zero entries must be visible"


# ---- 3: nothing else moves ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g1", "resisc16"])
def test_other_gradients_are_bit_equal_whether_the_matrix_requires_grad_or_not(device, shape):
    k = _case_with_loss(shape)
    m = dense(k.na).to(device)
    const_model = k.model(device)
    const_model.set_comm(m)
    ref = _run(k, const_model, device)
    live = m.clone().requires_grad_()
    model = k.model(device)
    model.set_comm(live)
    got = _run(k, model, device, ref["act"])
    assert live.grad is not None and live.grad.abs().max().item() > 0
    for key, v in ref.items():
        assert th.equal(v, got[key]), f"{key} moved when the matrix asked for its gradient"
    assert th.equal(model.comm, m) and not model.comm.requires_grad


@pytest.mark.parametrize("shape", ["g1", "resisc16"])
def test_frozen_model_with_only_the_matrix_requiring_grad(device, shape):
    k = _case_with_loss(shape)
    m = dense(k.na).to(device)
    live = m.clone().requires_grad_()
    model = k.model(device)
    model.set_comm(live)
    base = _run(k, model, device)
    want = live.grad.clone()
    live.grad = None
    frozen = k.model(device)
    frozen.requires_grad_(False)
    frozen.set_comm(live)
    sampler = _sampler(k, frozen, device)
    img = k.img.to(device)  # (does not require grad either: the node is built for the matrix alone)
    ep = sampler.run_episode(img, replay=_replay(sampler, base["act"], device))
    assert ep.step_preds.grad_fn is not None and ep.step_probs.grad_fn is not None
    _dist_loss(ep.step_preds, ep.step_log_probas, ep.step_values, ep.step_probs, k.terms, k.w).backward()
    assert all(p.grad is None for p in frozen.parameters())
    assert th.equal(live.grad, want)
    with th.no_grad():  # no graph without grad mode, whatever the matrix asks for
        ep = sampler.run_episode(img, replay=_replay(sampler, base["act"], device))
    assert ep.step_preds.grad_fn is None and not ep.step_preds.requires_grad


# ---- 4: the step nodes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g1", "resisc16"])
def test_step_loop_accumulates_the_fused_nodes_gradient(device, shape):
    k = _case_with_loss(shape)
    live = dense(k.na).to(device).requires_grad_()
    model = k.model(device)
    model.set_comm(live)
    sampler = _sampler(k, model, device)
    ep = sampler.run_episode(k.img.to(device))
    _a2c_like_loss(ep.step_preds, ep.step_log_probas, ep.step_values, k.terms).backward()
    fused = live.grad.clone()
    live.grad = None
    model.zero_grad(set_to_none=True)
    out = _act_loop(k, model, device)
    assert th.equal(out["pos"], ep.step_pos), "the act loop moved otherwise than the episode"
    _a2c_like_loss(out["preds"], out["logp"], out["values"], k.terms).backward()
    _grad(f"{_family()}/step_loop/{shape}/d_comm", live.grad, fused)


@pytest.mark.parametrize("shape", ["g1", "g2", "resisc16"])
def test_step_loop_with_a_carried_message_that_requires_grad(device, oracle_live, shape):
    """ModelsWrapper.forward unrolled, every output in the loss, the initial state and message leaves: dM sums over
    the steps' nodes (step 0 included: its message is the caller's) and agrees with float64 autograd."""
    k = CommCase(shape)
    m = dense(k.na)
    m64 = m.double().clone().requires_grad_()
    oracle_live(lambda: m64)
    live = m.to(device).requires_grad_()
    model = k.model(device)
    model.set_comm(live)
    obs, npos, st0, ws = _unroll_inputs(k)
    _, grads = _unroll(k, model, device, obs, npos, st0, ws)
    p64 = k.params64()
    leaves64 = [t.double().requires_grad_() for t in st0]
    h, cst, hc, cc, msg = leaves64
    loss64 = 0.0
    for t in range(NS):
        so = mo.step_forward(p64, k.cfg, obs[t].double(), msg, npos[t].double(), h, cst, hc, cc)
        h, cst, hc, cc, msg = so.h, so.c, so.hc, so.cc, so.msg
        o = (so.probs, so.values, so.preds, so.msg, so.h, so.c, so.hc, so.cc)
        loss64 = loss64 + sum((w.double() * x).sum() for w, x in zip(ws[t], o))
    loss64.backward()
    _grad(f"{_family()}/unroll/{shape}/d_comm", live.grad, m64.grad)
    _grad(f"{_family()}/unroll/{shape}/d_msg0", grads[4], leaves64[4].grad)


# ---- 5: LearnableComm ----------------------------------------------------------------------------------------------
def _softmax64(logits64, support):
    z = logits64.masked_fill(~support, float("-inf"))
    rows = support.any(1, keepdim=True)
    z = th.where(rows, z, th.zeros_like(z))  # (an empty row: softmax of zeros, masked away below)
    return th.where(support, th.softmax(z, dim=1), th.zeros_like(z))


@pytest.mark.parametrize("shape,gname", [("g1", "ring"), ("g1", "teams"), ("resisc16", "star")])
def test_logit_gradients_match_float64_through_the_masked_softmax(device, oracle_live, shape, gname):
    k = CommCase(shape)
    lc = comm.LearnableComm(graph(gname, k.na))
    with th.no_grad():
        lc.logits.add_(0.5 * k.randn(k.na, k.na) * lc.support)
    l64 = lc.logits.detach().double().requires_grad_()
    sup = lc.support.clone()
    oracle_live(lambda: _softmax64(l64, sup))
    terms = _loss_terms(k)
    w = k.randn(NS, k.na, k.nb, k.cfg.nb_action)
    tr = _oracle_loop(k, k.params64(), k.img.double())
    _dist_loss(tr["preds"], tr["logp"], tr["values"], tr["probs"], terms, w).backward()
    lc = lc.to(device)
    model = k.model(device)
    _episode_dm(k, model, lc, device, tr["act"], terms, w)
    assert model.comm_parameters()[0] is lc.logits
    _grad(f"logits/{shape}/{gname}", lc.logits.grad, l64.grad)
    assert (lc.logits.grad[~lc.support] == 0).all()


# ---- 6: reproducibility --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["g1", "resisc16"])
def test_two_runs_give_the_same_bits(device, shape):
    k = _case_with_loss(shape)
    grads, act = [], None
    for _ in range(2):
        live = dense(k.na).to(device).requires_grad_()
        model = k.model(device)
        model.set_comm(live)
        act = _run(k, model, device, act)["act"]
        grads.append(live.grad.clone())
    assert th.equal(grads[0], grads[1])


# ---- 7: trainers -----------------------------------------------------------------------------------------------------
def _adam64(x, grads, lr):
    """The float64 Adam updates of one tensor over a list of gradients (carried moments)."""
    p, m, v = {"x": x.clone()}, {"x": th.zeros_like(x)}, {"x": th.zeros_like(x)}
    for step, g in enumerate(grads, 1):
        mo.adam_step(p, {"x": g}, m, v, step, lr)
    return p["x"]


def _logits_match(tag, lc, l0, grads, lr):
    ref = _adam64(l0, grads, lr)
    got = lc.logits.detach().double().cpu()
    big = th.ones_like(l0, dtype=th.bool)
    for g in grads:  # (Adam's sign-like first update amplifies a gradient that is zero up to rounding)
        big &= g.abs() > 1e-6
    assert big.any()
    err = ((got - l0)[big] - (ref - l0)[big]).abs().max().item()
    bound = len(grads) * 1e-3 * lr
    print(f"[comm_grad] {tag}: max err {err:.3e} (bound {bound:.1e})")
    REC.put(tag, {"max_err": err, "tol": bound})
    assert err <= bound, f"{tag}: {err:.3e}"
    off = ~lc.support.cpu()
    assert th.equal(got[off], l0[off]), "logits off the support must not move"


@pytest.mark.parametrize("shape", ["g1", "resisc16"])
def test_train_step_updates_the_logits_like_float64_adam_and_the_model_like_a_constant_matrix(device, oracle_live,
                                                                                              shape):
    from marlclassification_amd.training import Trainer

    k = CommCase(shape)
    lr, comm_lr, gamma = 1e-3, 1e-2, 0.99
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    lc = comm.LearnableComm(comm.ring(k.na))
    l0 = lc.logits.detach().double().clone()
    l64 = l0.clone().requires_grad_()
    sup = lc.support.clone()
    oracle_live(lambda: _softmax64(l64, sup))
    tr = _oracle_loop(k, k.params64(), k.img.double())
    mo.a2c_loss(tr["preds"], tr["logp"], tr["values"], y, gamma).loss.backward()

    lc = lc.to(device)
    const = lc().detach().clone()
    model = k.model(device)
    model.set_comm(lc)
    sampler = _sampler(k, model, device, probs=False)
    _force(sampler, tr["act"], device)
    trainer = Trainer(model, k.cfg.nb_class, lr, gamma, comm_lr=comm_lr)
    out, _ = trainer.train_step(k.img, y, sampler)
    assert th.equal(out.step_actions.cpu(), tr["act"])
    _logits_match(f"train_step/{shape}/logits", lc, l0, [l64.grad], comm_lr)
    assert not th.equal(model.comm, const), "the next forward must see the updated matrix"

    plain = k.model(device)
    plain.set_comm(const)
    sampler2 = _sampler(k, plain, device, probs=False)
    _force(sampler2, tr["act"], device)
    Trainer(plain, k.cfg.nb_class, lr, gamma).train_step(k.img, y, sampler2)
    assert th.equal(model.flat_state().params, plain.flat_state().params), "the model's update moved"
    assert th.equal(model.flat_state().grads, plain.flat_state().grads)


def test_two_ppo_epochs_with_a_learnable_matrix_match_the_float64_oracle(device, oracle_live):
    from marlclassification_amd.training import Trainer

    k = CommCase("g1")
    eps = TWO_EPOCH_EPS["g1"]
    lr, gamma, lam, beta = (TWO_EPOCH[n] for n in ("lr", "gamma", "lam", "beta"))
    comm_lr = 1e-2
    y = _y(k)
    lc = comm.LearnableComm(comm.ring(k.na))
    sup = lc.support.clone()
    l0 = lc.logits.detach().double().clone()
    cur = {"l": l0.clone().requires_grad_()}
    oracle_live(lambda: _softmax64(cur["l"], sup))
    # float64: epoch 1 at rho = 1 -> Adam 1 on the parameters AND the logits -> the loop again under both, the
    # sampled actions forced -> the loss against the stored old log-probabilities -> Adam 2 with carried moments
    img64 = k.img.double()
    p = k.params64()
    tr = _oracle_loop(k, p, img64)
    advn, ret, _ = ref64.advantages(tr["preds"], tr["values"], y, gamma, lam)
    old_logp = tr["logp"].detach()
    ref64.ppo(tr["preds"], tr["logp"], tr["values"], tr["probs"], y, old_logp, advn, ret, eps, beta)[0].backward()
    g1 = _grads_of(p)
    gl1 = cur["l"].grad.clone()
    after = {n: v.detach().clone() for n, v in p.items()}
    m1 = {n: th.zeros_like(v) for n, v in after.items()}
    v1 = {n: th.zeros_like(v) for n, v in after.items()}
    mo.adam_step(after, g1, m1, v1, 1, lr)
    p2 = {n: v.clone().requires_grad_() for n, v in after.items()}
    cur["l"] = _adam64(l0, [gl1], comm_lr).requires_grad_()  # the matrix is evaluated again for the second epoch
    tr2 = _oracle_loop(k, p2, img64, forced=tr["act"])
    loss2, _, rho, _ = ref64.ppo(tr2["preds"], tr2["logp"], tr2["values"], tr2["probs"], y, old_logp, advn, ret, eps,
                               beta)
    assert_clear_of_bounds(rho, eps)
    loss2.backward()
    g2 = _grads_of(p2)
    gl2 = cur["l"].grad.clone()
    mo.adam_step(after, g2, m1, v1, 2, lr)

    lc = lc.to(device)
    model = k.model(device)
    model.set_comm(lc)
    sampler = _sampler(k, model, device, probs=False)
    _force(sampler, tr["act"], device)
    trainer = Trainer(model, k.cfg.nb_class, lr, gamma, ppo_epochs=2, ppo_clip=eps, gae_lambda=lam,
                      entropy_coef=beta, comm_lr=comm_lr)
    trainer.train_epoch([(k.img, y)], 0, sampler)
    assert trainer.curr_step == 1 and model.flat_state().step == 2
    REC_COMM.updates_match("comm_grad/ppo/g1/update", k, model, after, [g1, g2], lr, 2)
    _logits_match("ppo/g1/logits", lc, l0, [gl1, gl2], comm_lr)
    # (the second epoch ran under the updated matrix: with the first one its gradient would be another)
    assert (gl1 - gl2).abs().max().item() > 1e-6


# ---- 8: two ranks ----------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from marlclassification_amd.fused import EpisodeDraws
    from marlclassification_amd.parallel import BucketedGradAllReduce, broadcast_parameters, shard_bounds
    from marlclassification_amd.training import Trainer
    from tests.util import Golden

    device = th.device("cuda:0")  # both ranks share the one GPU of the test box
    g = Golden("g2_mnist_c1")
    model, sampler = _golden_sampler(g, device)
    flat = model.flat_state()
    lc = comm.LearnableComm(comm.ring(g.na)).to(device)
    model.set_comm(lc)
    l0 = lc.logits.detach().cpu().clone()
    hook = None
    if world > 1:
        broadcast_parameters(flat.params)
        hook = BucketedGradAllReduce(world, None, flat.offsets, flat.numel, device)
    # world == 1: the parent's reference pass - the shard of `rank` out of two, alone, no collective
    lo, hi = shard_bounds(g.nb, rank, 2)
    i = g.inp
    sampler.fixed_draws = EpisodeDraws(*(t.to(device) for t in (
        i.pos0[:, lo:hi].contiguous(), i.h0[:, lo:hi].contiguous(), i.c0[:, lo:hi].contiguous(),
        i.hc0[:, lo:hi].contiguous(), i.cc0[:, lo:hi].contiguous(), i.q[:, :, lo:hi].contiguous())))
    trainer = Trainer(model, g.cfg.nb_class, g.lr, g.gamma, allreduce=hook, comm_lr=1e-2)
    trainer.train_epoch([(g.img[lo:hi], g.y[lo:hi])], 0, sampler)
    th.cuda.synchronize()
    out_q.put((rank, l0.numpy(), lc.logits.detach().cpu().numpy(), lc.logits.grad.cpu().numpy(),
               flat.params.cpu().numpy()))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _spawn(world, ranks):
    """{rank: what it put} of the ranks started (world 1: one shard alone, no collective)"""
    return {r[0]: r[1:] for r in run_ranks(_dp_worker, world, results=len(ranks), ranks=ranks)}


def test_two_ranks_take_the_same_logit_update_from_the_averaged_gradient(device):
    import numpy as np

    both = _spawn(2, (0, 1))
    assert np.array_equal(both[0][1], both[1][1]), "the logits differ between the ranks"
    assert np.array_equal(both[0][2], both[1][2]), "the ranks back-propagated different averaged gradients"
    assert np.array_equal(both[0][3], both[1][3]), "the parameters differ between the ranks"
    # the reference: every shard alone (one process each, no collective), gradients averaged here
    alone = [_spawn(1, (r,))[r] for r in (0, 1)]
    l0 = th.from_numpy(both[0][0]).double()
    g_avg = 0.5 * (th.from_numpy(alone[0][2]).double() + th.from_numpy(alone[1][2]).double())
    err = (th.from_numpy(both[0][2]).double() - g_avg).abs().max().item()
    print(f"[comm_grad] two_ranks/logit_grad: max err {err:.3e}, ref max {g_avg.abs().max().item():.3e}")
    assert err <= GRAD_TOL * g_avg.abs().max().item() + 1e-7
    ref = _adam64(l0, [g_avg], 1e-2)
    big = g_avg.abs() > 1e-6
    assert big.any()
    upd = th.from_numpy(both[0][1]).double() - l0
    assert ((upd - (ref - l0))[big]).abs().max().item() <= 1e-3 * 1e-2
    assert not np.array_equal(both[0][1], both[0][0]), "the logits did not move"


# ---- 9: guards -----------------------------------------------------------------------------------------------------
def _fused(k, device, source, **kw):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C
    from tests.util import model_spec

    eng = HipEngine(model_spec(k.cfg), device)
    eng.set_comm(source)
    eng.configure(k.na, k.nb, NS, k.img.shape[1:])
    flat = FlatParams(mo.param_shapes(k.cfg), device)
    flat.load(k.params)
    return eng, flat, FusedA2C(eng, flat, 1e-3, 0.99, **kw)


def test_fused_a2c_learns_the_matrix_and_refuses_graph_capture(device):
    from marlclassification_amd.fused import EpisodeDraws

    k = CommCase("g1")
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen).to(device)
    i = k.inp
    draws = EpisodeDraws(*(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0, i.q[:NS])))
    img = k.img.to(device)
    lc = comm.LearnableComm(comm.ring(k.na)).to(device)
    with pytest.raises(ValueError):
        _fused(k, device, lc, use_graph=True, comm_lr=1e-2)
    eng, flat, fa = _fused(k, device, lc, comm_lr=1e-2)
    with pytest.raises(ValueError):
        fa.iteration_graph(img, y, 5, 0)
    before = lc.logits.detach().clone()
    const = lc().detach().clone()
    fa.iteration(img, y, draws)
    assert not th.equal(lc.logits.detach(), before) and th.equal(lc.logits.detach()[~lc.support], before[~lc.support])
    # the model's update is the constant-matrix iteration's, bit for bit
    eng2, flat2, fa2 = _fused(k, device, const)
    fa2.iteration(img, y, draws)
    assert th.equal(flat.params, flat2.params) and th.equal(flat.grads, flat2.grads)
    # PPO epochs: the matrix is evaluated again before every replay
    lc3 = comm.LearnableComm(comm.ring(k.na)).to(device)
    eng3, flat3, fa3 = _fused(k, device, lc3, comm_lr=1e-2, ppo_epochs=2)
    seen = []
    refresh = eng3.refresh_comm
    eng3.refresh_comm = lambda: seen.append(refresh().detach().clone())
    fa3.iteration(img, y, draws)
    assert len(seen) == 2 and not th.equal(seen[0], seen[1]) and flat3.step == 2


def test_without_a_comm_lr_a_live_source_launches_nothing_new(device, monkeypatch):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.training import Trainer

    k = CommCase("g1")
    y = th.randint(k.cfg.nb_class, (k.nb,), generator=k.gen)
    lc = comm.LearnableComm(comm.ring(k.na)).to(device)
    const = lc().detach().clone()
    model = k.model(device)
    model.set_comm(lc)

    def boom(*a, **kw):
        raise AssertionError("marl_comm_grad was asked for without a comm_lr")
    monkeypatch.setattr(HipEngine, "comm_grad", boom)
    before = lc.logits.detach().clone()
    Trainer(model, k.cfg.nb_class, 1e-3, 0.99).train_step(k.img, y, _sampler(k, model, device, probs=False))
    assert th.equal(lc.logits.detach(), before) and lc.logits.grad is None
    plain = k.model(device)
    plain.set_comm(const)
    Trainer(plain, k.cfg.nb_class, 1e-3, 0.99).train_step(k.img, y, _sampler(k, plain, device, probs=False))
    assert th.equal(model.flat_state().params, plain.flat_state().params)


def test_library_guards_on_the_device(device):
    import ctypes as C

    from marlclassification_amd.engine import _nbytes

    k = _case_with_loss("g1")
    eng, flat, fa = _fused(k, device, dense(k.na).to(device))
    fa.pack()
    d_comm = th.empty(k.na, k.na, device=device)
    with pytest.raises(ValueError):
        eng.comm_grad(eng.episode_ws(True), NS, th.empty(k.na, k.na + 1, device=device))
    with pytest.raises(ValueError):
        eng.comm_grad(eng.episode_ws(True), NS, th.empty(k.na, k.na))
    m = eng.comm
    eng.comm = None
    with pytest.raises(ValueError):
        eng.episode_backward(None, None, None, flat.grad_views(), d_comm=d_comm)
    eng.comm = m
    lib, cfg = eng.lib, eng.cfg
    wws, ews = eng.packed_weights_ws(), eng.episode_ws(True)
    need = lib.marl_comm_grad_scratch_bytes(C.byref(cfg))
    sc = th.empty(need // 4, device=device)
    head = (C.byref(cfg), wws.data_ptr(), _nbytes(wws), ews.data_ptr(), _nbytes(ews), NS, d_comm.data_ptr(),
            sc.data_ptr())
    assert lib.marl_comm_grad(*head, need, None) == -1  # no matrix installed
    try:
        assert lib.marl_comm_matrix(m.data_ptr(), k.na) == 0
        assert lib.marl_comm_grad(*head, need - 4, None) == -4
        assert lib.marl_comm_grad(*head[:6], None, sc.data_ptr(), need, None) == -1
        assert lib.marl_comm_grad(*head[:4], _nbytes(ews) // 2, *head[5:], need, None) == -4
        other = th.zeros(k.na + 1, k.na + 1, device=device)
        assert lib.marl_comm_matrix(other.data_ptr(), k.na + 1) == 0
        assert lib.marl_comm_grad(*head, need, None) == -1
    finally:
        assert lib.marl_comm_matrix(None, 0) == 0


# ---- 10: the command line ------------------------------------------------------------------------------------------
def test_train_learn_comm_writes_a_matrix_that_comm_file_loads(device, tmp_path, capsys):
    import json

    import numpy as np

    from marlclassification_amd.__main__ import main

    out = str(tmp_path / "run")
    main(["--run-id", "r", "-a", "3", "--step", "3", "--cuda", "train", "--res-folder", "synthetic", "--nb-epoch", "2",
          "--batch-size", "8", "--learn-comm", "--comm", "ring", "--comm-lr", "0.05", "-o", out])
    capsys.readouterr()
    assert json.load(open(os.path.join(out, "marl.json")))["comm"] == "ring"
    mats = []
    for e in (0, 1):
        path = os.path.join(out, "models", f"comm_epoch_{e}.npy")
        assert os.path.exists(path) and os.path.exists(os.path.join(out, "models", f"nn_models_epoch_{e}.pt"))
        m = comm.parse(path, 3)  # what `test` / `infer --comm FILE.npy` do
        assert m.dtype == th.float32 and bool(th.isfinite(m).all())
        assert th.equal(m != 0, comm.ring(3) != 0) and (m.double().sum(1) - 1).abs().max().item() <= 1e-6
        mats.append(m)
        assert np.load(path).shape == (3, 3)
    assert not th.equal(mats[0], comm.ring(3)) and not th.equal(mats[0], mats[1]), "the graph did not move"
    sd = th.load(os.path.join(out, "models", "nn_models_epoch_1.pt"))
    assert not any("comm" in k or "logits" in k for k in sd)
