"""marl_cnn_bwd_plan and marl_cnn_fwd_plan (include/marl_hip_cnnops.h) on the host: the plans of the conv launchers
- backward for a raw layer shape, forward for a model and a row count - from the launchers' own routines.  They must
agree with what marl_plan_query reports for a whole configuration, and the grids of tests/conv_cases.py (the cases of
tests/test_gpu_conv_bwd.py and tests/test_gpu_conv_fwd.py) must witness every instantiation a model can select.  No
GPU: the library loads without one (tests/test_plan_witness_host.py relies on the same)."""
import ctypes as C

import pytest

from tests import conv_cases as fwd
from tests.conv_cases import DG_SHAPES, WG_DEEP, WG_FIRST, assert_wgrad_witness
from tests.conv_cases import bwd_plan as plan
from tests.util import CASES, PLAN_CASES, plan_witness


def _lib():
    from marlclassification_amd import _lib as L

    return L.load()


def _layers(ft_extr, window):
    """(l, cin, cout, hin, groups of the layer below) of every conv layer"""
    from marlclassification_amd.engine import CNN_SPECS

    ch, grp = CNN_SPECS[ft_extr]
    h = window
    for l in range(len(grp)):
        yield l, ch[l], ch[l + 1], h, (grp[l - 1] if l else 1)
        h = (h - 1) // 2 + 1


@pytest.mark.parametrize("cfg,na,nb,ns,shape", [
    (CASES["g4_resisc_b2"], 16, 255, 4, (3, 256, 256)),  # tests/util.py's c3_partial_batch: three layers, bf16x6 on two
    (PLAN_CASES["worldstrat16"][0], 4, 7 * 37, 3, (3, 72, 80)),  # five layers, one without a fused layer backward
    (CASES["g2_mnist_c1"], 3, 1024, 5, (1, 28, 28)),  # layers with 1 and 8 input channels
], ids=["resisc45", "worldstrat", "mnist"])
def test_the_hook_agrees_with_plan_query(cfg, na, nb, ns, shape):
    w = plan_witness(cfg, na, nb, ns, shape)
    some_dgrad = False
    for l, cin, cout, hin, G in _layers(cfg.ft_extr, cfg.window):
        p = plan(w["NR"], cin, cout, hin, G, int(l == 0))
        assert (p["wg_rb"], p["wg_chunks"], p["wg_blocks"]) == tuple(w[f"cnn_wgrad_{f}{l}"] for f in ("rb", "chunks", "blocks")), (l, p, w)
        assert p["wg_form"] in (1, 3) and (p["wg_form"] == 3) <= bool(w["wgrad3"])
        if l:
            assert p["dg_rb"] == w[f"cnn_dgrad_rb{l}"] and p["dg_supported"] == (p["dg_rb"] > 0), (l, p, w)
            some_dgrad |= p["dg_rb"] > 1
        else:
            assert p["dg_supported"] == 0
    assert some_dgrad  # (the row counts are large enough for multi-patch chunks: not only the degenerate answer)


def test_the_grid_witnesses_every_selectable_weight_gradient_instantiation():
    """every (first, sct, skt, pd) of cnn_wgrad_kernel that some CNN_SPECS model selects at a window of 4..32 under the
    default knobs is the asserted witness of a case of tests/test_gpu_conv_bwd.py"""
    from marlclassification_amd.engine import CNN_SPECS

    witnessed = {(1, w["sct"], w["skt"], w["pd"]) for *_, w in WG_FIRST.values()}
    witnessed |= {(0, w["sct"], w["skt"], w["pd"]) for *_, w in WG_DEEP.values()}
    selected = {}
    for name in CNN_SPECS:
        for window in range(4, 33):
            for l, cin, cout, hin, G in _layers(name, window):
                p = plan(1000, cin, cout, hin, G, int(l == 0))
                assert p["wg_form"] in (1, 3), (name, window, l, p)  # (every layer of every model is covered)
                if p["wg_form"] == 1:
                    selected.setdefault((int(l == 0), p["wg_sct"], p["wg_skt"], p["wg_pd"]), (name, window, l))
    missed = {k: v for k, v in selected.items() if k not in witnessed}
    assert not missed, f"cnn_wgrad_kernel<sct, skt, first, pd> selectable but not in the GPU grid: {missed}"
    assert (1, 1, 1, 4) in selected and (0, 2, 9, 2) in selected and (0, 1, 5, 2) in selected  # (the sweep sees them)


def test_the_grid_tables_hold_on_the_host():
    """the witnesses of the GPU grid, without a GPU: a plan rule that moves fails here already"""
    for cin, cout, f, _, rows, *_, w in WG_FIRST.values():
        assert_wgrad_witness(plan(rows, cin, cout, f, 1, 1), w)
    for cin, cout, hin, G, rows, w in WG_DEEP.values():
        assert_wgrad_witness(plan(rows, cin, cout, hin, G, 0), w)
    lib = _lib()
    try:
        for cin, cout, G, hin, w in DG_SHAPES.values():
            assert lib.marl_tune(b"dgrad_min_chunks", 512) == 0
            p = plan(5, cin, cout, hin, G, 0)
            assert (p["dg_supported"], p["dg_rb"], p["dg_mt"], p["dg_nt"], p["dg_blocks"]) == (1, 1, w["mt1"], w["nt"], 5)
            assert lib.marl_tune(b"dgrad_min_chunks", 1) == 0
            p = plan(5, cin, cout, hin, G, 0)
            rb = w["rb_big"]
            assert (p["dg_rb"], p["dg_mt"], p["dg_nt"], p["dg_blocks"]) == (rb, -(-rb * hin * hin // 16), w["nt"], -(-5 // rb))
    finally:
        lib.marl_tune(b"dgrad_min_chunks", 512)
    # the default knob keeps 512 chunks: rb = 2 from 1023 rows (512 chunks, the last one of one patch) on
    assert plan(1022, 8, 16, 3, 2, 0)["dg_rb"] == 1 and plan(1023, 8, 16, 3, 2, 0)["dg_rb"] == 2


def test_refusals_need_no_gpu():
    from marlclassification_amd._lib import CnnBwdPlan

    lib = _lib()
    p = CnnBwdPlan()
    assert lib.marl_cnn_bwd_plan(10, 8, 16, 3, 2, 0, None) == -1
    for bad in ((0, 8, 16, 3, 2, 0), (10, 0, 16, 3, 2, 0), (10, 8, 0, 3, 2, 0), (10, 8, 16, 0, 2, 0), (10, 8, 16, 3, 0, 0)):
        assert lib.marl_cnn_bwd_plan(*bad, C.byref(p)) == -1, bad
    assert lib.marl_cnn_bwd_plan(10, 3, 16, 12, 0, 1, C.byref(p)) == 0  # (the first layer has no groups)
    # not covered: nothing but zeros, and the entry point refuses before it looks at the device
    for cin, cout, hin, G in ((64, 128, 4, 16), (12, 32, 4, 4), (16, 32, 4, 3), (16, 30, 4, 2)):
        d = plan(10, cin, cout, hin, G, 0)
        assert (d["dg_supported"], d["dg_rb"], d["dg_mt"], d["dg_nt"], d["dg_blocks"]) == (0, 0, 0, 0, 0), d
        assert lib.marl_cnn_dgrad_scratch(10, cin, cout, hin, G) == 0
        a = 4096  # (an aligned non-null address: the call must return before it reads anything)
        assert lib.marl_cnn_dgrad(a, a, 128, a, a, a, a, a, a, a, a, 1 << 20, 10, cin, cout, hin, G, None) == -2
        assert b"outside the fused kernel's range" in lib.marl_last_error()
    assert plan(10, 12, 32, 4, 4, 0)["wg_form"] == 0  # (three channels per group: the weight gradient neither)
    assert lib.marl_cnn_dgrad(None, 4096, 32, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 1 << 20, 10, 16, 32, 4, 2,
                              None) == -1
    assert lib.marl_cnn_dgrad_scratch(10, 16, 32, 4, 2) == 10 * 2 * 16 * 4


# ---- forward (tests/test_gpu_conv_fwd.py) ----------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,na,nb,ns,shape", [
    (CASES["g4_resisc_b2"], 16, 255, 4, (3, 256, 256)),  # Fwd2Resisc on its persistent walk
    (PLAN_CASES["worldstrat16"][0], 4, 7 * 37, 3, (3, 72, 80)),  # the general kernel at rb = 4
    (CASES["g2_mnist_c1"], 3, 1024, 5, (1, 28, 28)),  # Fwd2Mnist6; the general kernel under cnn_fwd2 = 0
], ids=["resisc45", "worldstrat", "mnist"])
def test_the_forward_hook_agrees_with_plan_query(cfg, na, nb, ns, shape):
    from tests.util import model_spec

    lib = _lib()
    mc = model_spec(cfg).config(na, nb, ns, *shape)
    seen = set()
    try:
        for knob in (1, 0):
            assert lib.marl_tune(b"cnn_fwd2", knob) == 0
            for train in (0, 1):
                w = plan_witness(cfg, na, nb, ns, shape, train=bool(train))
                p = fwd.fwd_plan(mc, train, na * nb)
                assert p["fused"] == 1
                assert (p["which"], p["rb"], p["blocks"]) == (w["cnn_fwd"], w["cnn_fwd_rb"], w["cnn_fwd_blocks"]), (p, w)
                assert p["writes_image"] == (p["which"] in (1, 2, 4, 5)) and not any(p["keeps_cols"])
                seen.add((knob, p["which"]))
    finally:
        lib.marl_tune(b"cnn_fwd2", 1)
    assert all(which == 6 for knob, which in seen if knob == 0)
    assert {which for knob, which in seen if knob == 1} in ({1}, {2}, {6})


def test_the_forward_grid_witnesses_every_selectable_plan():
    """the (which, keeps_cols) pairs that a CNN_SPECS model - or the custom stack the kept-rows scan adds - selects at a
    window of 4..32 under the default knobs, as a rollout or a training launch, are exactly those the witnesses of
    tests/test_gpu_conv_fwd.py name; and every model is covered by the fused forward"""
    from marlclassification_amd.engine import CNN_SPECS

    selected = {}
    for name, stack in list(CNN_SPECS.items()) + list(fwd.COLS_EXTRA.items()):
        for f in range(4, 33):
            for train in (0, 1):
                p = fwd.fwd_plan(fwd.config(stack, f, f + 8, f + 10), train, 1000)
                assert p["fused"] == 1, (name, f)
                selected.setdefault((p["which"], tuple(p["keeps_cols"])), (name, f, train))
    witnessed = {(w["which"], tuple(w["keeps_cols"])) for rows in fwd.GRID.values() for w in rows.values()}
    witnessed |= {(w["which"], tuple(w["keeps_cols"])) for w in fwd.COLS_GRID.values()}
    assert set(selected) == witnessed, (selected, witnessed)
    assert {k[0] for k in selected} == {1, 2, 3, 4, 5, 6}
    # rows are kept on the fused path by no CNN_SPECS model: only by the custom stack, from its smallest window on
    assert fwd.smallest_cols_config()[:3] == (fwd.COLS_MIN[0], fwd.CUSTOM, fwd.COLS_MIN[1])


def test_the_forward_grid_tables_hold_on_the_host():
    """the witnesses of the GPU grid without a GPU, the shapes its comments promise, and the knobs back at their
    defaults afterwards"""
    lib = _lib()
    for model, rows_w in fwd.GRID.items():
        with fwd.knobs(model):
            for rows, w in rows_w.items():
                assert fwd.fwd_plan(fwd.model_config(model), 1, rows) == w, (model, rows)
                if rows > w["rb"]:
                    assert rows % w["rb"] == 1
                if rows > 1000:
                    assert (w["blocks"] == 256 < -(-rows // w["rb"])) if w["which"] != 6 else w["blocks"] == -(-rows // w["rb"])
        assert lib.marl_tune_get(b"cnn_fwd2", 1) == 1 and lib.marl_tune_get(b"cnn_fwd3", 1) == 1
    for rows, w in fwd.COLS_GRID.items():
        assert fwd.fwd_plan(fwd.model_config(fwd.COLS_MIN[2]), 1, rows) == w
    for model, rows in fwd.FORMS.items():  # the image forms compare launches of one plan
        p1, p0 = (fwd.fwd_plan(fwd.model_config(model), t, rows) for t in (1, 0))
        assert (p1["which"], p1["rb"]) == (p0["which"], p0["rb"]) and rows in fwd.GRID[model]


def test_forward_refusals_need_no_gpu():
    from marlclassification_amd._lib import CnnFwdIo, CnnFwdPlan

    lib = _lib()
    cfg = fwd.model_config("mnist10")
    p = CnnFwdPlan()
    assert lib.marl_cnn_fwd_plan(C.byref(cfg), 1, 10, None) == -1
    assert lib.marl_cnn_fwd_plan(None, 1, 10, C.byref(p)) == -1 and lib.marl_cnn_fwd_plan(C.byref(cfg), 1, 0, C.byref(p)) == -1
    # one channel per group: outside the fused forward - every field 0, and the launch refuses before it reads anything
    refused = fwd.config(([1, 8, 16], [8, 4]), 10, 28, 30)
    assert fwd.fwd_plan(refused, 1, 10) == dict(fused=0, which=0, rb=0, blocks=0, keeps_cols=[0] * 5, writes_image=0)
    io = CnnFwdIo()
    io.img = io.pos = io.u = 4096  # (aligned non-null addresses)
    io.rows, io.ldu = 10, 144
    assert lib.marl_cnn_fwd(C.byref(refused), 4096, 1 << 30, C.byref(io), None) == -2
    assert b"does not cover" in lib.marl_last_error()
    assert lib.marl_cnn_fwd(C.byref(cfg), 4096, 0, C.byref(io), None) == -4
    io.u = None
    assert lib.marl_cnn_fwd(C.byref(cfg), 4096, 1 << 30, C.byref(io), None) == -1
    assert lib.marl_cnn_fwd(C.byref(cfg), 4096, 1 << 30, None, None) == -1
