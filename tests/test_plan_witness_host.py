"""Plan witnesses and the knob table, on the host: marl_plan_query answers from the launchers' own plan routines
(host arithmetic only) and marl_tune refuses a key the library does not read.  No GPU: the library loads without one
(tests/test_ppo_host.py relies on the same)."""
import ctypes as C

import pytest

from tests.util import (CASES, KNOB_DEFAULTS, PLAN_CASES, PLAN_INVARIANTS, PLAN_WITNESS, Golden, assert_witness, cdiv,
                        library_knobs, model_spec, plan_witness)


def _lib():
    from marlclassification_amd import _lib as L

    return L.load()


def test_an_unknown_knob_is_refused_and_every_known_one_is_accepted():
    """marl_tune used to create any key: a test or lab that toggled a retired knob compared two identical runs.
    (Each known knob is set to the value it already has, so nothing moves for the tests that follow.)"""
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


# ---- the plan under the installed settings: marl_plan_query reports the Plan object the drivers run ----
_FAKE = 1 << 12  # a "device pointer": the setters only store it, marl_plan_query never follows it
SETTINGS = ("none", "ring", "ring+range", "explore", "greedy", "class_loss")
SETTING_KEYS = ("comm", "comm_range", "comm_form", "explore", "explore_form", "class_loss")


def _clear(lib):
    assert lib.marl_comm_range(-1, 0, 1) == 0 and lib.marl_comm_matrix(None, 0) == 0
    assert lib.marl_policy_explore(1.0, 0.0, 0) == 0 and lib.marl_class_loss(None, 0, 0.0, None, 0, 0) == 0


def _install(lib, setting, na, nc):
    if setting in ("ring", "ring+range"):
        assert lib.marl_comm_matrix(_FAKE, na) == 0
    if setting == "ring+range":
        assert lib.marl_comm_range(8, 0, 1) == 0  # Chebyshev, normalised
    if setting == "explore":
        assert lib.marl_policy_explore(2.0, 0.1, 0) == 0
    if setting == "greedy":
        assert lib.marl_policy_explore(1.0, 0.0, 1) == 0
    if setting == "class_loss":
        assert lib.marl_class_loss(_FAKE, nc, 0.1, None, 0, 1) == 0


def full_witness(cfg, na, nb, ns, shape):
    """every key of plan_witness plus the settings' own keys and marl_workspace_sizes, for train = 0 and 1"""
    lib = _lib()
    mc = model_spec(cfg).config(na, nb, ns, *shape)
    out = {}
    for train in (0, 1):
        w = plan_witness(cfg, na, nb, ns, shape, train=bool(train))
        for k in SETTING_KEYS:
            v = C.c_int(-7)
            assert lib.marl_plan_query(C.byref(mc), train, k.encode(), C.byref(v)) == 0, k
            w[k] = v.value
        wb, eb = C.c_size_t(0), C.c_size_t(0)
        assert lib.marl_workspace_sizes(C.byref(mc), train, C.byref(wb), C.byref(eb)) == 0
        w["weights_bytes"], w["episode_bytes"] = wb.value, eb.value
        out[train] = w
    return out


def _shapes():
    out = {tag: _golden_shape(tag) for tag in CASES}
    for tag, (cfg, na, nd, rep, ns, shape) in PLAN_CASES.items():
        out[tag] = (cfg, na, nd * rep, ns, shape)
    return out


PLAN_RELATIONS = ["panel_sample <= panel_chain", "(comm_form in (0, 1, 2)) == (comm == 0)",
                  "(comm_form == 5) == (comm == 1 and panel_chain == 1)", "(explore_form == 0) == (explore == 0)",
                  "(explore_form == 1) == (explore == 1 and panel_sample == 1)", "small_r == (lstm_plan in (3, 4))",
                  "(lstm_plan == 0) == (g3_lstm == 0)"]


def _is_layout_key(k):
    return k.startswith(("g3", "cnn_")) or k in ("wgrad3", "weights_bytes", "episode_bytes")


@pytest.mark.parametrize("tag", list(CASES) + list(PLAN_CASES))
def test_the_plan_under_every_installed_setting(tag):
    """(a) the relations the plan encodes hold under every setting; (b) no setting moves a layout: both workspace
    sizes and every g3* / cnn_* / wgrad3 key are those of the uninstalled library; (c) clearing a setting restores
    every key."""
    lib = _lib()
    cfg, na, nb, ns, shape = _shapes()[tag]
    _clear(lib)
    base = full_witness(cfg, na, nb, ns, shape)
    try:
        for setting in SETTINGS:
            _install(lib, setting, na, cfg.nb_class)
            got = full_witness(cfg, na, nb, ns, shape)
            _clear(lib)
            for train in (0, 1):
                w = got[train]
                assert_witness(w, PLAN_RELATIONS + PLAN_INVARIANTS)
                moved = {k: (base[train][k], w[k]) for k in w if _is_layout_key(k) and w[k] != base[train][k]}
                assert not moved, (setting, train, moved)
                assert w["comm"] == (setting in ("ring", "ring+range")), (setting, w)
                assert w["comm_range"] == (8 if setting == "ring+range" else -1), (setting, w)
                assert w["explore"] == (setting in ("explore", "greedy")) and w["class_loss"] == (setting == "class_loss")
            assert full_witness(cfg, na, nb, ns, shape) == base, setting
    finally:
        _clear(lib)


def test_a_matrix_takes_a_wide_belief_cell_off_the_chain():
    """belief width above 384 with every message width at or below it: chained without a matrix, and under one the
    unchained panel launches behind mix_msg_kernel (the chained kernels keep the matrix in the LDS the wide input
    panel would need) - the one place where an installed setting changes the kernel family"""
    from oracle import marl_oracle as mo

    lib = _lib()
    cfg = mo.OracleConfig("mnist", 6, 388, 64, 16, 24, 8, 10, 96, 96)
    _clear(lib)
    try:
        w = full_witness(cfg, 3, 4, 3, (1, 28, 28))[1]
        assert (w["panel_chain"], w["comm_form"], w["panel_sample"]) == (1, 0, 1)
        _install(lib, "ring", 3, cfg.nb_class)
        w = full_witness(cfg, 3, 4, 3, (1, 28, 28))[1]
        assert (w["panel_chain"], w["comm_form"], w["panel_sample"]) == (0, 3, 0)
        narrow = mo.OracleConfig("mnist", 6, 384, 64, 16, 24, 8, 10, 96, 96)
        assert full_witness(narrow, 3, 4, 3, (1, 28, 28))[1]["comm_form"] == 5
    finally:
        _clear(lib)


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
