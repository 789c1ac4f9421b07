"""CPU: the float64 references of tests/test_gpu_row_fwd.py checked alone (tests/row_cases.py) - the cell-backward
formulas against float64 autograd from the pre-activations, the conditions under which the offset inputs of the two
norms and the saved row of the explore form are fair to the kernels, the im2col column order, the message mean and
the exploration constants against marlclassification_amd/explore.py."""
import pytest
import torch as th

from tests import row_cases as rc
from tests.parity import FWD_TOL, GRAD_TOL


@pytest.mark.parametrize("n", rc.CELL_N_VEC4 + [rc.CELL_N_SCALAR])
def test_cell_backward_formulas_match_autograd(n):
    rows = 65
    x = rc.CellInputs(rows, n, seed=n)
    pre = x.pre.double().requires_grad_()
    c_prev = x.c_prev.double().requires_grad_()
    gates, c_new, h = rc.cell_forward(pre, c_prev)
    (h * x.dh.double()).sum().backward(retain_graph=True)
    (c_new * x.dc.double()).sum().backward()
    # the formulas on the EXACT activations are the gradient ...
    dg, dcp = rc.cell_bwd_formulas(gates.detach(), c_prev.detach(), c_new.detach(), x.dh, x.dc)
    assert (dg - pre.grad).abs().max().item() <= 1e-12 * pre.grad.abs().max().item()
    assert (dcp - c_prev.grad).abs().max().item() <= 1e-12 * c_prev.grad.abs().max().item()
    # ... and on the fp32-rounded ones (what the kernel is given) they stay far inside the gradient bound
    dg32, dcp32 = rc.cell_bwd_formulas(x.gates, x.c_prev, x.c_new, x.dh, x.dc)
    assert (dg32 - pre.grad).abs().max().item() <= GRAD_TOL / 4 * pre.grad.abs().max().item()
    assert (dcp32 - c_prev.grad).abs().max().item() <= GRAD_TOL / 4 * c_prev.grad.abs().max().item()


def test_saturated_cell_has_bounded_formulas():
    x = rc.CellInputs(65, 20, seed=3, saturated=True)
    dg, dcp = rc.cell_bwd_formulas(x.gates, x.c_prev, x.c_new, x.dh, x.dc)
    assert th.isfinite(dg).all() and th.isfinite(dcp).all()
    assert dg.abs().max().item() <= rc.saturated_bound(x)


def _within(got, ref, tol):
    err = (got.double() - ref).abs().max().item()
    return err, tol * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("form", list(rc.GN_OFFSET))
def test_offset_inputs_are_fair_to_a_group_norm(form):
    """the same op in fp32 torch stays within FWD_TOL / 4 of float64 on the mean-8 inputs"""
    P, C, G = rc.GN_OFFSET[form]
    assert rc.gn_form(P, C) == form
    z = rc.norm_input((67, P, C), seed=P * C, offset=True)
    gamma, beta = rc.affine(C, C)
    act64, st64 = rc.gn_silu(z.double(), gamma.double(), beta.double(), G)
    act32, st32 = rc.gn_silu(z, gamma, beta, G)
    for got, ref in ((act32, act64), (st32[..., 0], st64[..., 0]), (st32[..., 1], st64[..., 1])):
        err, bound = _within(got, ref, FWD_TOL / 4)
        assert err <= bound, (form, err, bound)
    assert abs(z.mean().item() - rc.OFFSET_MEAN) < 0.1 and abs(z.std().item() - rc.OFFSET_STD) < 0.05


@pytest.mark.parametrize("n", rc.LN_OFFSET_N)
def test_offset_inputs_are_fair_to_a_layer_norm(n):
    z = rc.norm_input((67, n), seed=n, offset=True)
    gamma, beta = rc.affine(n, n)
    act64, st64 = rc.ln_silu(z.double(), gamma.double(), beta.double())
    act32, st32 = rc.ln_silu(z, gamma, beta)
    for got, ref in ((act32, act64), (st32[..., 0], st64[..., 0]), (st32[..., 1], st64[..., 1])):
        err, bound = _within(got, ref, FWD_TOL / 4)
        assert err <= bound, (n, err, bound)


def test_gn_forms_are_the_ones_the_cases_name():
    for form, cases in rc.GN_CASES.items():
        for P, C, G in cases:
            assert rc.gn_form(P, C) == form and C % G == 0, (form, P, C, G)


def test_im2col_column_order():
    rows, C, hin = 2, 4, 3
    act = th.arange(rows * C * hin * hin, dtype=th.float64).reshape(rows, C, hin * hin) + 1
    cols = rc.im2col(act, hin)
    hout = (hin - 1) // 2 + 1
    assert cols.shape == (rows * hout * hout, 9 * C)
    img = act.reshape(rows, C, hin, hin)
    for r in range(rows):
        for oy in range(hout):
            for ox in range(hout):
                for kh in range(3):
                    for kw in range(3):
                        y, x = 2 * oy - 1 + kh, 2 * ox - 1 + kw
                        for c in range(C):
                            want = img[r, c, y, x].item() if 0 <= y < hin and 0 <= x < hin else 0.0
                            assert cols[(r * hout + oy) * hout + ox, (kh * 3 + kw) * C + c].item() == want


@pytest.mark.parametrize("tau", rc.EXPLORE_TAU)
@pytest.mark.parametrize("n_actions", rc.POLICY_NA)
def test_explore_formula_on_the_saved_row_matches_autograd(n_actions, tau):
    """the condition of the explore reference: the float64 formula on the fp32-rounded saved row stays within
    GRAD_TOL / 4 of float64 autograd from the logits"""
    x = rc.PolicyInputs(257, n_actions, seed=n_actions, tau=tau, eps=rc.EXPLORE_EPS)
    for dlogp in (None, x.dlogp):
        for dprobs in (None, x.dprobs):
            if dlogp is None and dprobs is None:
                continue
            ref = rc.dlogits_explore_autograd(x.logits, x.actions, dlogp, dprobs, tau, x.keep, x.floor)
            got = rc.dlogits_explore_formula(x.probs, x.actions, dlogp, dprobs, tau, x.keep, x.floor)
            err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
            assert err <= GRAD_TOL / 4 * scale + 1e-12, (n_actions, tau, err, scale)


def test_plain_forms_are_the_softmax_gradient():
    x = rc.PolicyInputs(64, 5, seed=1)
    z = x.logits.clone().requires_grad_()
    p = th.softmax(z, -1)
    ((p * x.dprobs.double()).sum() + (x.dlogp.double() * th.log(p.gather(1, x.actions.long()[:, None])[:, 0])).sum()).backward()
    exact = rc.dlogits_probs(p.detach(), x.actions, x.dlogp, x.dprobs)
    assert (exact - z.grad).abs().max().item() <= 1e-12
    assert th.equal(rc.dlogits_plain(p.detach(), x.actions, x.dlogp),
                    rc.dlogits_probs(p.detach(), x.actions, x.dlogp, th.zeros_like(x.dprobs)))
    # keep = 1, floor = 0, tau = 1: the explore formula is the same gradient
    same = rc.dlogits_explore_formula(p.detach(), x.actions, x.dlogp, x.dprobs, 1.0, 1.0, 0.0)
    assert (same - z.grad).abs().max().item() <= 1e-12


def test_explore_constants_are_those_of_the_package():
    from marlclassification_amd.explore import behaviour_probs

    for n_actions in rc.POLICY_NA:
        keep, floor = rc.explore_keep_floor(n_actions)
        p = th.softmax(th.randn(3, n_actions, dtype=th.float64, generator=th.Generator().manual_seed(n_actions)), -1)
        for tau in rc.EXPLORE_TAU:
            want = behaviour_probs(p, tau, rc.EXPLORE_EPS)
            assert th.allclose(rc.behaviour(th.log(p), tau, keep, floor), want, rtol=1e-13, atol=0)


def test_message_mean_reference():
    m = th.randn(5 * 7, 21, generator=th.Generator().manual_seed(0))
    out = rc.agg_msg(m, 5, 7).reshape(5, 7, 21)
    m3 = m.double().reshape(5, 7, 21)
    for a in range(5):
        others = [b for b in range(5) if b != a]
        assert th.allclose(out[a], m3[others].mean(0), rtol=1e-13, atol=1e-15)
    assert th.equal(rc.agg_msg(m[:7], 1, 7), th.zeros(7, 21, dtype=th.float64))


def test_row_hooks_are_declared_bound_and_outside_the_abi():
    import os
    import re

    from marlclassification_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "marl_hip_rowops.h")).read()
    declared = set(re.findall(r"^int (marl_[a-z0-9_]+)\(", header, re.M))
    assert declared == set(_lib.ROWOP_HOOKS) and len(declared) == 9
    assert set(_lib.ROWOP_HOOKS) <= set(_lib._HOOKS) and not set(_lib.ROWOP_HOOKS) & set(_lib.EXPORTS)
    assert len(_lib.EXPORTS) == 57 and _lib.MARL_ABI_VERSION == 5
    lib = _lib.load()
    assert all(getattr(lib, name).argtypes for name in _lib.ROWOP_HOOKS)
