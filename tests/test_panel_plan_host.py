"""marl_panel_plan, marl_panel_scratch_bytes and the refusals of marl_panel_fwd / marl_panel_bwd
(include/marl_hip_panelops.h) on the host: no GPU is touched - every refusal happens before a launch and the plan entry
is the launchers' own host arithmetic.

* the plan against an independent Python restatement (tests/panel_harness.py: py_fwd_plan / py_bwd_plan) of
  panel_waves_for, panel_ksplit, panel_stride and the LDS sums, over a sweep of widths that includes the GPU grid's;
* the witness of every case of tests/test_gpu_panel_kernels.py: a changed threshold fails here, loudly, instead of
  moving the case onto another form;
* the exactness of the known-answer operands in fp32;
* the refusals, with their messages;
* marl_panel_scratch_bytes against frag_floats of tests/panel_harness.py."""
import ctypes as C

import pytest
import torch as th

from tests import panel_harness as H
from tests.util import assert_witness


def _lib():
    from marlclassification_amd import _lib

    return _lib, _lib.load()


SWEEP_K = [1, 7, 15, 16, 17, 23, 40, 63, 64, 65, 96, 128, 129, 256, 257, 384, 400, 780, 1024]
SWEEP_N = [1, 13, 22, 31, 32, 33, 64, 100, 128, 129, 192, 383, 384]


@pytest.mark.parametrize("k", SWEEP_K)
def test_forward_plan_equals_the_restatement(k):
    for n in SWEEP_N:
        case = H.Fwd("sweep", k, (n,), 37)
        got, want = H.fwd_plan([case]), H.py_fwd_plan([(k, (n,), False)])
        assert (got["waves"], got["lds_bytes"]) == (want["waves"], want["lds_bytes"]), (k, n, got, want)
        for key in ("nt", "ks", "kper", "empty", "layer_waves", "ln_slots"):
            assert got[key] == [want["layers"][0][key]], (k, n, key, got, want)
        assert got["blocks"] == 3 and got["nlayers"] == 1


def test_forward_plan_of_chains_and_pairs_equals_the_restatement():
    groups = [[c] for c in H.FWD_CASES if len(c.widths) > 1] + [list(H.FWD_PAIR)]
    for cases in groups:
        got = H.fwd_plan(cases)
        want = H.py_fwd_plan([(c.k0, c.widths, c.mix) for c in cases])
        assert (got["waves"], got["lds_bytes"]) == (want["waves"], want["lds_bytes"]), (cases[0].name, got, want)
        for key in ("nt", "ks", "kper", "empty", "layer_waves", "ln_slots"):
            assert got[key] == [lay[key] for lay in want["layers"]], (cases[0].name, key)


@pytest.mark.parametrize("n", SWEEP_N)
def test_backward_plan_equals_the_restatement(n):
    for k in SWEEP_K:
        for off in (0, 1):
            case = H.Bwd("sweep", ((n, k),), 37, lddx_off=off)
            want = H.py_bwd_plan(case.layers, H.r4(k) + off)
            assert want["ok"]
            got = H.bwd_plan(case)
            for key in ("waves", "lds_bytes", "tail_lds", "retried", "maxc"):
                assert got[key] == want[key], (n, k, off, key, got, want)
            for key in ("nt", "ks", "kper", "empty", "rounds"):
                assert got[key] == [want["layers"][0][key]], (n, k, off, key, got, want)


def test_backward_plan_of_the_grid_equals_the_restatement():
    for case in H.BWD_CASES:
        got = H.bwd_plan(case)
        k_last = case.layers[-1][1]
        cb = None
        if case.cellb:
            ldn, ldg = H.r4(case.cellb.n) + 4, H.r4(4 * case.cellb.n) + 4
            cb = (case.cellb.n, ldg, ldn, ldn)
        want = H.py_bwd_plan(case.layers, H.r4(k_last) + 8 * case.pad + case.lddx_off, case.mix, cb)
        for key in ("waves", "lds_bytes", "tail_lds", "retried", "maxc"):
            assert got[key] == want[key], (case.name, key, got, want)
        for key in ("nt", "ks", "kper", "empty", "rounds"):
            assert got[key] == [lay[key] for lay in want["layers"]], (case.name, key)


def test_smallest_retried_input_width():
    """the retry without the LDS tail (launch_panel_bwd, "plan:") starts where two 16-row panels of the input width no
    longer fit: the grid's k_in = 1024 is past it, and the plan entry and the restatement agree on where it starts"""
    first = None
    for k in range(512, 1100, 4):
        got = H.bwd_plan(H.Bwd("retry", ((32, k),), 16))
        assert got["retried"] == H.py_bwd_plan(((32, k),), k)["retried"]
        assert got["tail_lds"] == 1 - got["retried"]
        if got["retried"] and first is None:
            first = k
    assert first is not None and first <= 1024


@pytest.mark.parametrize("case", H.FWD_CASES, ids=lambda c: c.name)
def test_forward_witness(case):
    assert case.witness, "every case names the mechanism it is there for and proves it engaged"
    assert_witness(H.fwd_plan([case]), case.witness)


def test_forward_pair_witness():
    assert_witness(H.fwd_plan(list(H.FWD_PAIR)), H.FWD_PAIR_WITNESS)


@pytest.mark.parametrize("case", H.BWD_CASES, ids=lambda c: c.name)
def test_backward_witness(case):
    assert_witness(H.bwd_plan(case), case.witness + ("nlayers >= 1",))


def test_grid_names_are_unique_and_the_grid_stays_small():
    names = [c.name for c in H.FWD_CASES] + ["b:" + c.name for c in H.BWD_CASES]
    assert len(set(names)) == len(names)
    assert len(names) <= 300


def test_known_answer_operands_are_exact_in_fp32():
    for tag, (k, n, _) in H.FWD_WIDTHS.items():
        p = H.fwd_plan([H.Fwd(tag, k, (n,), 16)])
        x, want = H.slice_kat(k, p["ks"][0], p["kper"][0])
        assert th.equal(x.double().sum(dim=1), want), tag
        assert th.equal(want.float().double(), want), tag  # the sums are fp32 numbers
        live = [s for s in range(p["ks"][0]) if not p["empty"][0] >> s & 1]
        assert want[0].item() == sum(2.0 ** -s for s in live), tag
        assert (x != 0).sum(dim=1).eq(len(live)).all(), tag
        # ... and so is every partial sum of them, in any order: all are multiples of 2^-(ks-1) below 2
        assert p["ks"][0] <= 24
    oh = H.one_hot_rows(37)
    assert th.equal(oh.sum(dim=0), 2.0 ** (th.arange(37) % 5).float()) and (oh != 0).sum() == 37


def test_scratch_bytes_equal_the_fragment_copies():
    _, lib = _lib()
    for tag, (k, n, _) in H.FWD_WIDTHS.items():
        got = lib.marl_panel_scratch_bytes(0, 1, (C.c_int * 1)(n), (C.c_int * 1)(k))
        assert got == 4 * H.frag_floats(n, k), tag
        got = lib.marl_panel_scratch_bytes(1, 1, (C.c_int * 1)(n), (C.c_int * 1)(k))
        assert got == 4 * (H.frag_floats(k, n) + H.r4(n * k)), tag  # the [k, n] copy + the row-major transpose it is built from
    widths, ks = (64, 32, 64, 48), (40, 64, 32, 64)
    got = lib.marl_panel_scratch_bytes(0, 4, (C.c_int * 4)(*widths), (C.c_int * 4)(*ks))
    assert got == 4 * sum(H.frag_floats(n, k) for n, k in zip(widths, ks))
    assert lib.marl_panel_scratch_bytes(0, 0, None, None) == 0
    assert lib.marl_panel_scratch_bytes(0, 5, (C.c_int * 5)(), (C.c_int * 5)()) == 0


# ---- refusals: on the host, before any launch (a CPU-only machine runs them) ---------------------------------------
def _refused(rc, code, text):
    mod, lib = _lib()
    assert rc == code, (rc, lib.marl_last_error())
    assert text in lib.marl_last_error().decode(), lib.marl_last_error()


def _fwd_call(case, edit=None, scratch_bytes=None, plan=False):
    mod, lib = _lib()
    bufs = H.FwdBufs(case, H.fwd_inputs(case), "cpu")
    d = H.fwd_descs([bufs])
    if edit:
        edit(d[0])
    if plan:
        return lib.marl_panel_plan(d, 1, None, C.byref(mod.PanelPlan()))
    need = H.fwd_scratch_bytes(lib, [case])
    scratch = th.zeros(need // 4 + 4)
    return lib.marl_panel_fwd(d, 1, scratch.data_ptr(), need if scratch_bytes is None else scratch_bytes, None)


def _bwd_call(case, edit=None, scratch_bytes=None):
    mod, lib = _lib()
    bufs = H.BwdBufs(case, H.bwd_inputs(case), "cpu")
    d = bufs.desc()
    if edit:
        edit(d)
    need = H.bwd_scratch_bytes(lib, case)
    scratch = th.zeros(need // 4 + 4)
    return lib.marl_panel_bwd(C.byref(d), scratch.data_ptr(), need if scratch_bytes is None else scratch_bytes, None)


PLAIN = H.Fwd("plain", 40, (64, 32), 37)
CHAIN = H.Fwd("chain", 40, (64, 32, 64, 48), 35, "chain", 5, 7, agg_at=2, mix=True)
BPLAIN = H.Bwd("plain", ((64, 32), (32, 40)), 37)
BCHAIN = H.Bwd("chain", ((48, 64), (64, 32), (32, 64), (64, 40)), 35, "chain", 5, 7, agg_at=2, mix=True)
EINVAL, ELIMIT, ESIZE = -1, -2, -4


def test_error_codes_are_the_headers():
    import re

    from tests.util import ROOT

    hdr = open(f"{ROOT}/include/marl_hip.h").read()
    for name, val in (("MARL_EINVAL", EINVAL), ("MARL_ESIZE", ESIZE), ("MARL_ELIMIT", ELIMIT)):
        assert int(re.search(rf"#define {name} \((-\d+)\)", hdr).group(1)) == val, name


def test_forward_refusals():
    _refused(_fwd_call(H.Fwd("wide", 40, (385,), 16)), ELIMIT, "width 385 outside 1..384")
    _refused(_fwd_call(H.Fwd("wide_inner", 40, (384, 64), 16), lambda d: setattr(d.layer[0], "n", 400)), ELIMIT, "outside 1..384")
    _refused(_fwd_call(PLAIN, lambda d: setattr(d.layer[1], "w", None)), EINVAL, "null fragment source")
    _refused(_fwd_call(CHAIN, lambda d: setattr(d, "agg_at", 0)), ELIMIT, "a mixing matrix needs the in-panel aggregation")
    _refused(_fwd_call(CHAIN, lambda d: setattr(d, "by_batch", 4)), ELIMIT, "by_batch * g_na = 20 > 16")
    _refused(_fwd_call(CHAIN, lambda d: setattr(d, "g_nb", 8)), EINVAL, "m == g_na * g_nb")
    _refused(_fwd_call(CHAIN, lambda d: setattr(d, "agg_at", 4)), EINVAL, "0 < agg_at < nlayers")
    _refused(_fwd_call(PLAIN, scratch_bytes=H.fwd_scratch_bytes(_lib()[1], [PLAIN]) - 4), ESIZE, "scratch too small")
    for field in ("sample", "explore", "gate_pos"):
        _refused(_fwd_call(PLAIN, lambda d, f=field: setattr(d, f, 1)), EINVAL, "not served here")
    _refused(_fwd_call(PLAIN, lambda d: setattr(d, "ldx", 42)), EINVAL, "ldx % 4 == 0")
    _refused(_fwd_call(PLAIN, lambda d: setattr(d, "x", d.x + 4)), EINVAL, "16-byte aligned")
    _refused(_fwd_call(PLAIN, lambda d: setattr(d, "nlayers", 5)), EINVAL, "1..4 layers")
    _refused(_fwd_call(PLAIN, lambda d: setattr(d.layer[0], "a", None)), EINVAL, "null vector or output")
    _refused(_fwd_call(PLAIN, lambda d: setattr(d.layer[1], "lda", 31)), EINVAL, "leading dimension below")
    # the launcher's own range checks, reached through its planning routine before anything is enqueued
    _refused(_fwd_call(H.Fwd("lds", 4000, (32,), 16)), ELIMIT, "shape outside its range")
    _refused(_fwd_call(H.Fwd("msg", 40, (64, 384, 64), 32, "chain", 2, 16, agg_at=2)), ELIMIT,
             "in-panel message mean outside its range")
    # the plan entry refuses the same requests
    _refused(_fwd_call(H.Fwd("wide", 40, (385,), 16), plan=True), ELIMIT, "width 385 outside 1..384")
    mod, lib = _lib()
    _refused(lib.marl_panel_plan(None, 0, None, C.byref(mod.PanelPlan())), EINVAL, "exactly one of")
    _refused(lib.marl_panel_fwd(None, 1, None, 0, None), EINVAL, "one or two problems")


def test_backward_refusals():
    _refused(_bwd_call(H.Bwd("wide", ((385, 32),), 16)), ELIMIT, "width 385 outside 1..384")
    _refused(_bwd_call(BPLAIN, lambda d: setattr(d.layer[1], "w", None)), EINVAL, "null fragment source")
    _refused(_bwd_call(BCHAIN, lambda d: setattr(d, "agg_at", 0)), ELIMIT, "a mixing matrix needs the in-panel aggregation")
    _refused(_bwd_call(BCHAIN, lambda d: setattr(d, "by_batch", 4)), ELIMIT, "by_batch * g_na = 20 > 16")
    _refused(_bwd_call(BPLAIN, lambda d: setattr(d.layer[1], "n", 48)), EINVAL, "is not layer 1's width")
    _refused(_bwd_call(BPLAIN, lambda d: setattr(d, "gate_pos", 1)), EINVAL, "not served here")
    _refused(_bwd_call(BPLAIN, scratch_bytes=H.bwd_scratch_bytes(_lib()[1], BPLAIN) - 4), ESIZE, "scratch too small")
    _refused(_bwd_call(BPLAIN, lambda d: setattr(d, "dx", None)), EINVAL, "dx must be")
    _refused(_bwd_call(BPLAIN, lambda d: setattr(d, "ldda", 62)), EINVAL, "da / da2 must be")
    _refused(_bwd_call(BPLAIN, lambda d: setattr(d.layer[0], "part", None)), EINVAL, "null pointer")
    cb = H.Bwd("cellb", ((48, 64),), 37, cellb=H.Cell(64))
    _refused(_bwd_call(cb, lambda d: setattr(d.cellb, "n", 32)), EINVAL, "cellb.n 32 is not the first layer's input width 64")
    _refused(_bwd_call(cb, lambda d: setattr(d.cellb, "ldg", 255)), EINVAL, "cellb: null pointer or a leading dimension")
    ride = H.Bwd("cell", ((64, 32),), 37, cell=H.Cell(64, rows=77))
    _refused(_bwd_call(ride, lambda d: setattr(d, "cell_rows", 0)), EINVAL, "cell_rows < 1")
    _refused(_bwd_call(ride, lambda d: setattr(d.cell, "dh", None)), EINVAL, "cell: null pointer")
    # the launcher's own range check (no retry left: the panels of the LayerNorm width itself do not fit)
    _refused(_bwd_call(H.Bwd("msg", ((48, 64), (64, 384), (384, 64)), 32, "chain", 2, 16, agg_at=2)), ELIMIT,
             "in-panel message mean outside its range")


def test_panel_hooks_stay_outside_the_versioned_abi():
    import re

    from tests.util import ROOT

    mod, _ = _lib()
    hdr = open(f"{ROOT}/include/marl_hip_panelops.h").read()
    assert set(re.findall(r"\b(marl_panel_[a-z0-9_]+)\(", hdr)) == set(mod.PANELOP_HOOKS)
    assert set(mod.PANELOP_HOOKS) <= set(mod._HOOKS) and not set(mod.PANELOP_HOOKS) & set(mod.EXPORTS)
    assert "marl_panel" not in open(f"{ROOT}/include/marl_hip.h").read()
