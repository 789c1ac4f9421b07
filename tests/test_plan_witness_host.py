"""Plan witnesses and the knob table, on the host: marl_plan_query answers from the launchers' own plan routines
(host arithmetic only) and marl_tune refuses a key the library does not read.  No GPU: the library loads without one
(tests/test_ppo_host.py relies on the same)."""
import ctypes as C

import pytest

from tests.util import (CASES, PLAN_CASES, PLAN_INVARIANTS, PLAN_WITNESS, Golden, assert_witness, cdiv, library_knobs,
                        model_spec, plan_witness)


def _lib():
    from marlclassification_amd import _lib as L

    return L.load()


def test_an_unknown_knob_is_refused_and_every_known_one_is_accepted():
    """marl_tune used to create any key: a test or lab that toggled a retired knob compared two identical runs.
    (Each known knob is set to the value it already has, so nothing moves for the tests that follow.)"""
    from tests.test_gpu_round6 import KNOB_DEFAULTS

    lib = _lib()
    found, table = library_knobs()
    assert set(table) == set(KNOB_DEFAULTS) | {"g3_clk", "g3_tn_abl"} == found
    for key in ("sample_maxa4", "panel_bwd_maxc", "panel_ln_narrow", "g3_tn_cell_splits", "g3_tn_cell_teams", "wgrad_rb",
                "G3", "g3 ", ""):
        assert lib.marl_tune(key.encode(), 1) == -1, key  # MARL_EINVAL
        assert b"unknown knob" in lib.marl_last_error()
        assert lib.marl_tune_get(key.encode(), 7) == 7  # (reading any key keeps working: nothing was stored)
    assert lib.marl_tune(None, 1) == -1
    for key in table:
        now = lib.marl_tune_get(key.encode(), KNOB_DEFAULTS.get(key, 0))
        assert lib.marl_tune(key.encode(), now) == 0, key
        assert lib.marl_tune_get(key.encode(), now + 1) == now


def _golden_shape(tag):
    g = Golden(tag)
    return g.cfg, g.na, g.nb, g.ns, tuple(g.img.shape[1:])


@pytest.mark.parametrize("tag", list(CASES))
def test_witness_keys_answer_for_the_goldens(tag):
    w = plan_witness(*_golden_shape(tag))
    assert_witness(w, PLAN_INVARIANTS)
    # the fixtures' row counts (95, 96, 48, 32) only ever reach the degenerate plans: one chunk per workgroup, no walk,
    # single-patch layer backward - which is why tests/test_gpu_plan_coverage.py exists
    assert w["cnn_fwd"] in (1, 2, 3) and w["cnn_fwd_blocks"] == cdiv(w["R"], 8)
    assert all(w[f"cnn_dgrad_rb{l}"] == 1 for l in range(1, w["L"]))
    assert all(w[f"cnn_wgrad_rb{l}"] >= 1 and w[f"cnn_wgrad_blocks{l}"] == w[f"cnn_wgrad_chunks{l}"] for l in range(w["L"]))


def test_gated_keys_report_what_runs_not_the_knob():
    """g3_tn_pipe / wgrad3 used to return the raw knob (1 by default) for every shape."""
    lib = _lib()
    assert lib.marl_tune_get(b"g3_tn_pipe", 1) == 1 and lib.marl_tune_get(b"wgrad3", 1) == 1
    w = plan_witness(*_golden_shape("g2_mnist_c1"))  # MnistCnn: 1 / 8 input channels; 480 contraction rows
    assert w["g3"] == 1 and w["g3_tn"] == 0 and w["g3_tn_pipe"] == 0 and w["wgrad3"] == 0
    w = plan_witness(*_golden_shape("g4_resisc_b2"))  # layers 1 / 2 have 16 / 32 input channels
    assert w["wgrad3"] == 1 and w["g3_tn_pipe"] == 0
    cfg = CASES["g4_resisc_b2"]
    w = plan_witness(cfg, 16, 256, 16, (3, 256, 256))  # the benched shape: both run
    assert w["g3_tn"] == 1 and w["g3_tn_pipe"] == 1 and w["wgrad3"] == 1


@pytest.mark.parametrize("tag", list(PLAN_CASES))
def test_plan_coverage_cases_reach_their_plans(tag):
    """the cases of tests/test_gpu_plan_coverage.py, with the values asserted there"""
    cfg, na, nd, rep, ns, shape = PLAN_CASES[tag]
    w = plan_witness(cfg, na, nd * rep, ns, shape)
    assert_witness(w, PLAN_WITNESS[tag] + PLAN_INVARIANTS)
    # rollout-only sizing keeps no im2col rows either: same forward plan
    w0 = plan_witness(cfg, na, nd * rep, ns, shape, train=False)
    assert [w0[k] for k in ("cnn_fwd", "cnn_fwd_rb", "cnn_fwd_blocks")] == [w[k] for k in ("cnn_fwd", "cnn_fwd_rb", "cnn_fwd_blocks")]


def test_witness_keys_are_parsed_strictly():
    lib = _lib()
    mc = model_spec(CASES["g4_resisc_b2"]).config(16, 4, 2, 3, 64, 64)  # three conv layers
    v = C.c_int(0)
    for key in (b"cnn_fwd_", b"cnn_fwd_rbx", b"cnn_dgrad_rb0", b"cnn_dgrad_rb3", b"cnn_dgrad_rb", b"cnn_dgrad_rb12",
                b"cnn_wgrad_rb3", b"cnn_wgrad_rb", b"cnn_wgrad_grid0", b"cnn_wgrad_blocks"):
        assert lib.marl_plan_query(C.byref(mc), 1, key, C.byref(v)) == -1, key
    for key in (b"cnn_dgrad_rb1", b"cnn_dgrad_rb2", b"cnn_wgrad_rb0", b"cnn_wgrad_chunks2", b"cnn_wgrad_blocks2"):
        assert lib.marl_plan_query(C.byref(mc), 1, key, C.byref(v)) == 0, key


def test_the_knobs_move_the_witnesses():
    """the witnesses follow the launchers under a knob: cnn_fwd2 = 0 hands Fwd2Mnist6's shape to the general kernel
    (rb = 8 at 3072 rows: 384 one-chunk workgroups), dgrad_min_chunks moves the layer backward's rb"""
    lib = _lib()
    cfg, na, nd, rep, ns, shape = PLAN_CASES["mnist6_b1024"]
    try:
        assert lib.marl_tune(b"cnn_fwd2", 0) == 0
        w = plan_witness(cfg, na, nd * rep, ns, shape)
        assert (w["cnn_fwd"], w["cnn_fwd_rb"], w["cnn_fwd_blocks"]) == (6, 8, 384)
        assert lib.marl_tune(b"cnn_fwd2", 1) == 0
        assert lib.marl_tune(b"dgrad_min_chunks", 1 << 30) == 0
        assert plan_witness(cfg, na, nd * rep, ns, shape)["cnn_dgrad_rb1"] == 1
        assert lib.marl_tune(b"wgrad3", 0) == 0
        assert plan_witness(*_golden_shape("g4_resisc_b2"))["wgrad3"] == 0
    finally:
        lib.marl_tune(b"cnn_fwd2", 1)
        lib.marl_tune(b"dgrad_min_chunks", 512)
        lib.marl_tune(b"wgrad3", 1)
