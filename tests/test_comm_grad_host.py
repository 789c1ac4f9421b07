"""CPU: learnable communication graphs - ``comm.LearnableComm``, ``set_comm`` with a live source, the exports of the
mixing-matrix gradient (``marl_comm_grad``), their host-side argument checks, the ``--learn-comm`` command line, and
the float64 reference the GPU tests use."""
import ctypes as C
import os
import re

import pytest
import torch as th

from marlclassification_amd import comm
from tests.util import ROOT
from tests.util import small_model_config as _model_config


def _row_normalised(m):
    m = m.double()
    s = m.sum(1, keepdim=True)
    return th.where(s != 0, m / th.where(s != 0, s, th.ones_like(s)), th.zeros_like(m))


def _masked_softmax64(logits, support):
    z = logits.double().masked_fill(~support, float("-inf"))
    out = th.zeros_like(z)
    rows = support.any(1)
    out[rows] = th.softmax(z[rows], dim=1)
    return out


GRAPHS = {"ring": comm.ring(5), "star": comm.star(5, 2), "grid": comm.grid(2, 3), "teams": comm.teams([2, 3]),
          "full": comm.full(4), "ring16": comm.ring(16, 2), "full16": comm.full(16)}


# ---- LearnableComm ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRAPHS))
def test_learnable_comm_starts_at_the_row_normalised_graph(name):
    g = GRAPHS[name]
    lc = comm.LearnableComm(g)
    m = lc()
    assert m.shape == g.shape and m.dtype == th.float32 and m.requires_grad
    assert (m.double() - _row_normalised(g)).abs().max().item() <= 1e-6
    assert (m[g == 0] == 0).all(), "off-support entries must be exact zeros"
    assert th.equal(lc.support, g != 0) and lc.nb_agents == g.shape[0]
    assert [n for n, _ in lc.named_parameters()] == ["logits"]


def test_learnable_comm_normalises_an_unnormalised_init_and_takes_a_mask():
    init = th.tensor([[0.0, 2.0, 6.0], [1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    m = comm.LearnableComm(init)()
    assert (m.double() - _row_normalised(init)).abs().max().item() <= 1e-6 and (m[2] == 0).all()
    mask = th.tensor([[False, True, True], [True, False, True], [False, False, False]])
    init2 = th.tensor([[9.0, 1.0, 3.0], [1.0, 0.0, 1.0], [5.0, 5.0, 5.0]])  # entries off the mask are ignored
    m2 = comm.LearnableComm(init2, mask)()
    assert th.allclose(m2, th.tensor([[0.0, 0.25, 0.75], [0.5, 0.0, 0.5], [0.0, 0.0, 0.0]]), atol=1e-6)
    assert (m2[~mask] == 0).all()


@pytest.mark.parametrize("name", ["ring", "star", "teams", "grid"])
def test_off_support_stays_exactly_zero_through_optimiser_steps(name):
    g = GRAPHS[name]
    lc = comm.LearnableComm(g)
    off = g == 0
    opt = th.optim.Adam(lc.parameters(), lr=0.1)
    gen = th.Generator().manual_seed(3)
    before = lc().detach().clone()
    for _ in range(3):
        opt.zero_grad()
        (lc() * th.randn(g.shape, generator=gen)).sum().backward()
        assert (lc.logits.grad[off] == 0).all(), "off-support logit gradients must be exactly 0"
        assert bool(th.isfinite(lc.logits.grad).all())
        opt.step()
    after = lc().detach()
    assert (after[off] == 0).all() and not th.equal(after, before)
    rows = (~off).any(1)
    assert (after[rows].double().sum(1) - 1).abs().max().item() <= 1e-6
    assert (lc.logits.detach()[off] == 0).all(), "Adam must not move a logit whose gradient is exactly 0"


@pytest.mark.parametrize("name", ["ring", "star", "teams", "full"])
def test_jacobian_agrees_with_a_float64_masked_softmax(name):
    g = GRAPHS[name]
    lc = comm.LearnableComm(g)
    with th.no_grad():
        lc.logits.add_(0.3 * th.randn(g.shape, generator=th.Generator().manual_seed(1)) * lc.support)
    w = th.randn(g.shape, generator=th.Generator().manual_seed(2))
    (lc() * w).sum().backward()
    l64 = lc.logits.detach().double().requires_grad_()
    m64 = _masked_softmax64(l64, lc.support)
    assert (lc().detach().double() - m64.detach()).abs().max().item() <= 1e-6
    (m64 * w.double()).sum().backward()
    ref = th.where(lc.support, l64.grad, th.zeros_like(l64.grad))
    assert (lc.logits.grad.double() - ref).abs().max().item() <= 1e-6 * max(1.0, ref.abs().max().item())
    jac = th.autograd.functional.jacobian(lambda z: _masked_softmax64(z, lc.support), l64.detach())
    jac32 = th.autograd.functional.jacobian(
        lambda z: th.func.functional_call(lc, {"logits": z}, ()), lc.logits.detach())
    assert (jac32.double() - jac).abs().max().item() <= 1e-6


def test_empty_rows_give_zeros_and_finite_gradients():
    g = comm.teams([1, 3])  # agent 0 is alone: its row is empty
    lc = comm.LearnableComm(g)
    m = lc()
    assert (m[0] == 0).all() and bool(th.isfinite(m).all())
    m.sum().backward()
    assert bool(th.isfinite(lc.logits.grad).all()) and (lc.logits.grad[0] == 0).all()
    none = comm.LearnableComm(comm.none(3))  # no support at all: legal as a module, all zeros
    assert (none() == 0).all()


def test_learnable_comm_guards_and_checkpoint_round_trip():
    with pytest.raises(ValueError):
        comm.LearnableComm(th.tensor([[0.0, -0.5], [1.0, 0.0]]))  # a negative weight on the support
    with pytest.raises(ValueError):
        comm.LearnableComm(comm.ring(3), th.ones(3, 3, dtype=th.bool))  # zeros of init on the support
    for bad in (th.ones(2, 3), th.tensor([[float("nan")]]), th.ones(comm.MAX_AGENTS + 1, comm.MAX_AGENTS + 1)):
        with pytest.raises(ValueError):
            comm.LearnableComm(bad)
    for bad_mask in (th.ones(3, 3), th.ones(2, 2, dtype=th.bool)):
        with pytest.raises(ValueError):
            comm.LearnableComm(comm.ring(3), bad_mask)
    lc = comm.LearnableComm(comm.ring(5))
    with th.no_grad():
        lc.logits.add_(th.randn(5, 5, generator=th.Generator().manual_seed(4)) * lc.support)
    m = lc.to_matrix()
    assert m.dtype == th.float32 and m.device.type == "cpu" and not m.requires_grad
    assert th.equal(comm.validate(m, 5), m)  # what --comm FILE.npy loads
    back = comm.LearnableComm.from_matrix(m)
    assert th.equal(back.support, lc.support) and (back().detach() - m).abs().max().item() <= 1e-6
    # a link whose weight underflowed to exactly 0 stays on the support when the mask is stored with the matrix
    with th.no_grad():
        lc.logits[0, 1] = -200.0
    m = lc.to_matrix()
    assert m[0, 1] == 0 and lc.to_mask().dtype == th.bool and th.equal(lc.to_mask(), lc.support)
    kept = comm.LearnableComm.from_matrix(m, lc.to_mask())
    assert th.equal(kept.support, lc.support) and (kept().detach() - m).abs().max().item() <= 1e-6
    assert not th.equal(comm.LearnableComm.from_matrix(m).support, lc.support)
    with pytest.raises(ValueError):
        comm.LearnableComm.from_matrix(m, th.ones(2, 2, dtype=th.bool))


# ---- set_comm with a live source -------------------------------------------------------------------------------------
def test_set_comm_with_a_live_source_leaves_the_state_dict_alone():
    nets = _model_config().build_networks()
    keys = list(nets.state_dict())
    n_params = len(list(nets.parameters()))
    lc = comm.LearnableComm(comm.ring(3))
    nets.set_comm(lc)
    assert list(nets.state_dict()) == keys and len(list(nets.parameters())) == n_params
    assert all(m is not lc for m in nets.modules()), "the source must not be registered"
    assert all(p is not lc.logits for p in nets.flat_state().param_views().values())
    fresh = _model_config().build_networks()
    fresh.load_state_dict(nets.state_dict())  # strict
    m = nets.comm
    assert m is not None and not m.requires_grad and m.grad_fn is None and m.dtype == th.float32
    assert (m.double() - comm.ring(3).double()).abs().max().item() <= 1e-6
    assert nets.comm_source is lc
    leaves = nets.comm_parameters()
    assert len(leaves) == 1 and leaves[0] is lc.logits
    # the source is live: a step of its optimiser shows in model.comm without another set_comm
    with th.no_grad():
        lc.logits[0, 1] += 1.0
    assert nets.comm[0, 1] > 0.5
    nets.set_comm(None)
    assert nets.comm is None and nets.comm_source is None and nets.comm_parameters() == []


def test_a_tensor_that_requires_grad_is_live_and_a_constant_is_still_cloned():
    nets = _model_config().build_networks()
    t = comm.ring(3).clone().requires_grad_()
    nets.set_comm(t)
    assert nets.comm_source is t and nets.comm_parameters()[0] is t
    assert th.equal(nets.comm, t.detach()) and not nets.comm.requires_grad
    with th.no_grad():
        t[0, 1] = 0.75
    assert nets.comm[0, 1] == 0.75, "a live tensor is held by reference"
    fn = lambda: t * 2.0  # noqa: E731 - a plain callable is a live source too (it offers no leaves of its own)
    nets.set_comm(fn)
    assert nets.comm_source is fn and nets.comm[0, 1] == 1.5 and nets.comm_parameters() == []
    given = comm.ring(3)
    nets.set_comm(given)
    given[0, 1] = 7.0
    assert nets.comm[0, 1] == 0.5 and nets.comm_source is None and nets.comm_parameters() == []
    for bad in (th.zeros(2, 3, requires_grad=True), th.zeros(3, requires_grad=True),
                lambda: th.zeros(2, 3), lambda: 1.0, lambda: th.zeros(3, 3, dtype=th.int64),
                th.zeros(comm.MAX_AGENTS + 1, comm.MAX_AGENTS + 1, requires_grad=True)):
        with pytest.raises((ValueError, TypeError)):
            nets.set_comm(bad)
    assert comm.is_live(t) and comm.is_live(fn) and not comm.is_live(given)


def test_comm_lr_guards():
    from marlclassification_amd.fused import CommUpdate, comm_update_for
    from marlclassification_amd.training import Trainer

    nets = _model_config().build_networks()
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            Trainer(nets, 10, 1e-3, 0.99, comm_lr=bad)
    lc = comm.LearnableComm(comm.ring(3))
    assert comm_update_for(None, None, list, 0.1) is None and comm_update_for(None, lc, list, None) is None
    cu = comm_update_for(None, lc, lambda: list(lc.parameters()), 0.1)
    assert isinstance(cu, CommUpdate) and comm_update_for(cu, lc, list, 0.1) is cu
    assert comm_update_for(cu, comm.LearnableComm(comm.ring(3)), lambda: [lc.logits], 0.1) is not cu
    with pytest.raises(ValueError):
        comm_update_for(None, lambda: None, list, 0.1)  # a source without leaves has nothing to learn
    with pytest.raises(RuntimeError):
        cu.step(None, None, 1.0)


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_library_exports_the_gradient_entries_and_the_abi_stays_5():
    from marlclassification_amd import _lib

    for name in ("marl_comm_grad", "marl_comm_grad_scratch_bytes"):
        assert name in _lib.EXPORTS
    assert _lib.MARL_ABI_VERSION == 5
    header = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    assert re.search(r"#define\s+MARL_ABI_VERSION\s+5\b", header)
    assert re.search(r"size_t\s+marl_comm_grad_scratch_bytes\(const marl_config\*\s*cfg\);", header)
    assert re.search(r"int\s+marl_comm_grad\(const marl_config\*\s*cfg,", header)
    assert "networks/message.py:5-17" in header[header.index("Gradient with respect to the mixing matrix"):
                                                 header.index("size_t marl_comm_grad_scratch_bytes")]
    lib = _lib.load()
    assert lib.marl_abi_version() == 5 and hasattr(lib, "marl_comm_grad")


def test_host_side_argument_checks_return_the_documented_codes():
    """Every guard of marl_comm_grad answers before anything is enqueued: no device is needed to see the codes."""
    from marlclassification_amd import _lib
    from marlclassification_amd.engine import ModelSpec

    lib = _lib.load()
    spec = ModelSpec("mnist", 6, 12, 10, 8, 9, 4, 10, 16, 16)
    cfg = spec.config(3, 4, 2, 1, 28, 28)
    need = lib.marl_comm_grad_scratch_bytes(C.byref(cfg))
    assert need == 8 * 3 * 3 * 4  # one [Na, Na] partial per (step, batch) pair while there are at most 1024 pairs
    big = spec.config(16, 256, 16, 1, 28, 28)
    assert lib.marl_comm_grad_scratch_bytes(C.byref(big)) == 1024 * 16 * 16 * 4
    bad = spec.config(0, 4, 2, 1, 28, 28)
    assert lib.marl_comm_grad_scratch_bytes(C.byref(bad)) == 0
    wb, eb = C.c_size_t(0), C.c_size_t(0)
    assert lib.marl_workspace_sizes(C.byref(cfg), 1, C.byref(wb), C.byref(eb)) == 0
    fake = 1 << 20  # (never dereferenced: every call below is refused on the host)
    args = dict(w=fake, wb=wb.value, e=fake, eb=eb.value, steps=2, out=fake, sc=fake, scb=need)

    def call(**kw):
        a = dict(args, **kw)
        return lib.marl_comm_grad(C.byref(cfg), a["w"], a["wb"], a["e"], a["eb"], a["steps"], a["out"], a["sc"],
                                  a["scb"], None)

    assert lib.marl_comm_matrix(None, 0) == 0
    assert call() == -1 and b"no communication matrix" in lib.marl_last_error()  # MARL_EINVAL: nothing installed
    try:
        assert lib.marl_comm_matrix(fake, 3) == 0
        assert call(out=None) == -1 and call(sc=None) == -1 and call(e=None) == -1  # MARL_EINVAL: null pointers
        assert call(steps=0) == -1
        assert call(scb=need - 1) == -4 and b"scratch" in lib.marl_last_error()  # MARL_ESIZE
        assert call(eb=eb.value - 256) == -4 and call(wb=wb.value - 256) == -4
        assert call(steps=3) == -4  # a three-step layout does not fit the two-step workspace
        assert lib.marl_comm_matrix(fake, 4) == 0
        assert call() == -1 and b"4 x 4" in lib.marl_last_error()  # MARL_EINVAL: another agent count
        # MARL_ELIMIT: a decoder weight [2 n_m, n_m] that does not fit the kernel's LDS
        wide = ModelSpec("mnist", 6, 12, 10, 512, 9, 4, 10, 16, 16).config(4, 4, 2, 1, 28, 28)
        assert lib.marl_workspace_sizes(C.byref(wide), 1, C.byref(wb), C.byref(eb)) == 0
        rc = lib.marl_comm_grad(C.byref(wide), fake, wb.value, fake, eb.value, 2, fake, fake,
                                lib.marl_comm_grad_scratch_bytes(C.byref(wide)), None)
        assert rc == -2 and b"outside the kernel's range" in lib.marl_last_error()
    finally:
        assert lib.marl_comm_matrix(None, 0) == 0


# ---- the command line ------------------------------------------------------------------------------------------------
def test_cli_learn_comm(capsys):
    from marlclassification_amd.__main__ import build_parser, check_learn_comm

    p = build_parser()
    head, tail = ["--run-id", "r", "train"], ["-o", "out"]
    a = p.parse_args(head + tail)
    assert a.learn_comm is False and a.comm_lr is None
    a = p.parse_args(head + ["--learn-comm"] + tail)
    assert a.learn_comm is True and a.comm_lr is None and a.comm is None
    check_learn_comm(p, a)
    a = p.parse_args(head + ["--learn-comm", "--comm-lr", "0.05", "--comm", "ring:2"] + tail)
    assert a.learn_comm and a.comm_lr == 0.05 and a.comm == "ring:2"
    check_learn_comm(p, a)
    for bad in (["--learn-comm", "--comm", "none"], ["--comm-lr", "0.1"], ["--learn-comm", "--comm-lr", "0"],
                ["--learn-comm", "--comm-lr", "-1"]):
        with pytest.raises(SystemExit):
            check_learn_comm(p, p.parse_args(head + bad + tail))
    with pytest.raises(SystemExit):
        p.parse_args(head + ["--comm-lr", "x"] + tail)
    others = {"test": ["--dataset-path", "d", "--json-path", "j", "--state-dict-path", "s", "-o", "out"],
              "infer": ["--images", "i", "--json-path", "j", "--state-dict-path", "s", "--class2idx", "c", "-o", "out"]}
    for mode, t in others.items():
        for flag in (["--learn-comm"], ["--comm-lr", "0.1"]):
            with pytest.raises(SystemExit):
                p.parse_args(["--run-id", "r", mode] + flag + t)
        assert p.parse_args(["--run-id", "r", mode, "--comm", "comm_epoch_3.npy"] + t).comm == "comm_epoch_3.npy"
    capsys.readouterr()


def test_train_config_defaults_keep_the_plain_run():
    from marlclassification_amd.config import TrainConfig

    t = TrainConfig(img_size=28, nb_epoch=1, learning_rate=1e-3, batch_size=8, resources_dir="synthetic",
                    output_dir="o", gamma=0.99)
    assert t.learn_comm is False and t.comm_lr is None


# ---- the float64 reference of the GPU tests --------------------------------------------------------------------------
@pytest.mark.parametrize("na", [1, 3, 5, 16])
def test_float64_reference_of_the_gpu_tests(na):
    """autograd's dM of einsum('ac,cbk->abk', M64, m) is sum_{b,k} dmbar[a,b,k] m[a',b,k] - dense, also where M is 0."""
    gen = th.Generator().manual_seed(na)
    m = th.randn(na, 4, 7, dtype=th.float64, generator=gen)
    w = th.randn(na, 4, 7, dtype=th.float64, generator=gen)
    mat = comm.ring(na).double().requires_grad_() if na > 1 else th.zeros(1, 1, dtype=th.float64, requires_grad=True)
    mbar = th.einsum("ac,cbk->abk", mat, m)
    (mbar.tanh() * w).sum().backward()
    dmbar = (1 - mbar.detach().tanh() ** 2) * w
    closed = th.einsum("abk,cbk->ac", dmbar, m)
    assert (mat.grad - closed).abs().max().item() <= 1e-12 * max(1.0, closed.abs().max().item())
    zero = mat.detach() == 0
    assert zero.any() and (mat.grad[zero] != 0).all(), "the gradient is dense: entries where M == 0 carry it too"
