"""The panel kernels' fragment-order weight copies (csrc/common.h: panel_frag_index).

Layout: a model whose matrices encode their own index (W[r][k] = 1024 r + k, exact in fp32) is packed and the
copies WPF<idx> / WTF<idx> are read back through marl_debug_buffer and compared, element for element, padding and
slack included, with a numpy construction of the documented layout
    [tile of 32 rows][16-deep K group][half: rows l16 | 16 + l16][lane = quad * 16 + l16][4 floats] + 3 groups of zeros.
The numpy construction itself is checked on the CPU against the scalar index formula first.

Parity: 3 agents, 5 images, 2 steps against the float64 oracle at the widths where the addressing can go wrong (K
tail, partly empty last tile, n % 16 != 0, three K slices, more column tiles than waves in the backward), on the
chained launch and - in one child process - under MARL_PANEL_CHAIN=0.  Bounds are the project's (DESIGN.md section
2): outputs 1e-5, loss 5e-5, gradients 1e-4 of the tensor's scale, positions and actions exact.

Refusal: the step entry with a null weights workspace returns an error and leaves the output buffers alone.

With MARL_PANEL_WFRAG_ERRORS=<file> the achieved errors are written there as JSON (profiles/panel_wfrag_errors.json
is one such run)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import marl_oracle as mo  # noqa: E402
from tests.panel_harness import frag_floats, frag_groups  # noqa: E402

gpu = pytest.mark.gpu

FWD = ["ENC_W0", "ENC_W1", "DEC_W0", "DEC_W1", "POL_W0"]  # streamed from the packed copies (WPF)
BWD = ["ENC_W0", "ENC_W1", "DEC_W0", "DEC_W1"]  # their transposes, from the transposed copies (WTF)

#                          extractor, window, n_b, n_a, n_m, n_m_o, n_d, classes, nlb, nla
LAYOUT_MODELS = {
    "c3": mo.OracleConfig("resisc45", 12, 256, 256, 64, 96, 16, 45, 384, 384),
    "c2": mo.OracleConfig("mnist", 6, 64, 64, 16, 24, 8, 10, 96, 96),  # tiles narrower than 32, n % 16 != 0
    "ktail40": mo.OracleConfig("mnist", 6, 32, 32, 20, 24, 8, 10, 48, 48),  # 2 n_m = 40: K % 16 != 0
}
PARITY_MODELS = {
    "ktail40_nmo24": LAYOUT_MODELS["ktail40"],  # (a) K tail 40, (b) n_m_o = 24
    "nmo100": mo.OracleConfig("mnist", 6, 32, 32, 16, 100, 8, 10, 48, 48),  # (b) last tile partly empty, 100 % 16 = 4
    "kslices3": mo.OracleConfig("mnist", 6, 256, 64, 64, 24, 8, 10, 48, 48),  # (c) n_b 256 -> 128: three slices of 96
    "bwd_rounds": mo.OracleConfig("mnist", 6, 400, 32, 16, 24, 8, 10, 48, 48),  # (d) 400 > 32 x 12 waves
}
NA, NB, NS, SHAPE = 3, 5, 2, (1, 28, 28)
TOL_OUT, TOL_LOSS, TOL_GRAD = 1e-5, 5e-5, 1e-4
_errors = {}


# ---- the documented layout, in numpy --------------------------------------------------------------------------------
def frag_reference(w):
    """w [n, K] -> the fragment-order copy, zero padding and the three groups of slack included"""
    n, k = w.shape
    nt, g = (n + 31) // 32, frag_groups(k)
    pad = np.zeros((nt * 32, g * 16), dtype=w.dtype)
    pad[:n, :k] = w
    a = pad.reshape(nt, 2, 16, g, 4, 4)  # tile, half, l16, group, quad, element
    a = a.transpose(0, 3, 1, 4, 2, 5)  # tile, group, half, quad, l16, element
    return np.concatenate([a.ravel(), np.zeros(3 * 512, dtype=w.dtype)])


def frag_index(r, k, groups):
    return ((((r >> 5) * groups + (k >> 4)) * 2 + ((r >> 4) & 1)) * 64 + ((k >> 2) & 3) * 16 + (r & 15)) * 4 + (k & 3)


def index_matrix(n, k):
    return (1024.0 * np.arange(n)[:, None] + np.arange(k)[None, :]).astype(np.float32)


def matrix_shapes(cfg):
    nm2 = 2 * cfg.n_m
    return {"ENC_W0": (nm2, cfg.n_b), "ENC_W1": (cfg.n_m, nm2), "DEC_W0": (nm2, cfg.n_m), "DEC_W1": (cfg.n_m_o, nm2),
            "POL_W0": (cfg.nla, cfg.n_a)}


@pytest.mark.parametrize("tag", list(LAYOUT_MODELS))
def test_numpy_layout_matches_the_index_formula(tag):
    """(CPU) every real entry sits where the scalar formula says, everything else is zero, a wave's load is 1 KB
    contiguous: lane (l16, quad) of half h of group g of tile j reads rows 32 j + 16 h + l16, columns 16 g + 4 quad .."""
    for name, (n, k) in matrix_shapes(LAYOUT_MODELS[tag]).items():
        for w in (index_matrix(n, k), index_matrix(n, k).T.copy()):  # forward copy, backward (transposed) copy
            rows, cols = w.shape
            ref = frag_reference(w)
            g = frag_groups(cols)
            assert ref.size == frag_floats(rows, cols)
            r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
            idx = frag_index(r, c, g)
            assert np.unique(idx).size == rows * cols and idx.max() < ref.size - 3 * 512
            assert np.array_equal(ref[idx], w), (tag, name)
            rest = np.ones(ref.size, dtype=bool)
            rest[idx.ravel()] = False
            assert not ref[rest].any(), (tag, name)
            # one load instruction: lane l of (tile j, group gg, half h) at float offset ((j g + gg) 2 + h) 256 + 4 l
            j, gg, h, lane = (rows - 1) // 32, g - 1, 0, 17
            off = ((j * g + gg) * 2 + h) * 256 + 4 * lane
            rr, kk = 32 * j + 16 * h + (lane & 15), 16 * gg + 4 * (lane >> 4)
            want = [w[rr, kk + e] if rr < rows and kk + e < cols else 0.0 for e in range(4)]
            assert ref[off: off + 4].tolist() == want


# ---- GPU: the packed copies -----------------------------------------------------------------------------------------
def _engine(cfg, device, na=NA, nb=NB, ns=NS, shape=SHAPE):
    from marlclassification_amd.engine import HipEngine
    from tests.util import model_spec

    eng = HipEngine(model_spec(cfg), device)
    eng.configure(na, nb, ns, shape)
    return eng


def _frag_copy(eng, which, name, n, k):
    from marlclassification_amd import _lib

    off, ld = C.c_int64(0), C.c_int(0)
    _lib.check(eng.lib.marl_debug_buffer(C.byref(eng.cfg), 1, f"W{which}F{_lib.P[name]}".encode(), 0, C.byref(off),
                                         C.byref(ld)))
    assert ld.value == frag_groups(k), (name, ld.value)
    return eng.weights_ws()[off.value: off.value + frag_floats(n, k)].cpu().numpy()


@gpu
@pytest.mark.parametrize("tag", list(LAYOUT_MODELS))
def test_packed_copies_match_the_documented_layout(device, tag):
    from marlclassification_amd import _lib
    from tests.util import uniform_params

    cfg = LAYOUT_MODELS[tag]
    shape = (3, 32, 32) if cfg.ft_extr == "resisc45" else SHAPE
    eng = _engine(cfg, device, shape=shape)
    params = uniform_params(cfg, 3)
    slot_name = {slot: name for name, slot in eng.slots.items()}
    for name, (n, k) in matrix_shapes(cfg).items():
        pname = slot_name[_lib.P[name]]
        assert tuple(params[pname].shape) == (n, k), (name, pname)
        params[pname] = th.from_numpy(index_matrix(n, k))
    eng.pack({k: v.to(device) for k, v in params.items()})
    th.cuda.synchronize()
    for name, (n, k) in matrix_shapes(cfg).items():
        w = index_matrix(n, k)
        got = _frag_copy(eng, "P", name, n, k)
        assert np.array_equal(got, frag_reference(w)), (tag, "WPF", name)
        if name in BWD:
            got = _frag_copy(eng, "T", name, k, n)
            assert np.array_equal(got, frag_reference(w.T.copy())), (tag, "WTF", name)
    # a parameter the panel kernels never stream has no copy
    off, ld = C.c_int64(0), C.c_int(0)
    assert eng.lib.marl_debug_buffer(C.byref(eng.cfg), 1, f"WTF{_lib.P['POL_W0']}".encode(), 0, C.byref(off),
                                     C.byref(ld)) != 0


# ---- GPU: parity with the float64 oracle ----------------------------------------------------------------------------
def _reference(cfg):
    from tests.util import uniform_params

    params = uniform_params(cfg, 7)
    img = th.rand(NB, *SHAPE, generator=th.Generator().manual_seed(11))
    y = th.randint(0, cfg.nb_class, (NB,), generator=th.Generator().manual_seed(12))
    inp = mo.draw_episode_inputs(cfg, NA, NB, NS, list(SHAPE[1:]), 13)
    tr, lo, grads = mo.train_iteration(params, cfg, img, y, inp, NS, 0.99)
    return {"params": params, "img": img, "y": y, "inp": tuple(getattr(inp, k) for k in ("pos0", "h0", "c0", "hc0", "cc0", "q")),
            "tr": {k: getattr(tr, k).detach() for k in ("step_preds", "step_log_probas", "step_values", "step_pos",
                                                        "step_actions")},
            "loss": float(lo.loss.item()), "grads": {k: v.detach() for k, v in grads.items()}}


def _achieved(cfg, ref, device):
    """one training iteration of the fused path against the reference: achieved errors, nothing asserted"""
    from marlclassification_amd.fused import EpisodeDraws, FlatParams, FusedA2C

    eng = _engine(cfg, device)
    flat = FlatParams(mo.param_shapes(cfg), device)
    flat.load(ref["params"])
    fa = FusedA2C(eng, flat, 1e-3, 0.99)
    draws = EpisodeDraws(*(t.to(device) for t in ref["inp"]))
    out, scalars = fa.iteration(ref["img"].to(device), ref["y"].to(device), draws)
    th.cuda.synchronize()
    tr = ref["tr"]
    e = {"positions_equal": bool(th.equal(out.step_pos.cpu(), tr["step_pos"])),
         "actions_equal": bool(th.equal(out.step_actions.cpu(), tr["step_actions"])),
         "loss": abs(scalars[0].item() - ref["loss"]), "loss_scale": max(1.0, abs(ref["loss"]))}
    for k in ("step_preds", "step_log_probas", "step_values"):
        e[k] = (getattr(out, k).cpu().double() - tr[k].double()).abs().max().item()
    gv = flat.grad_views()
    worst = 0.0
    for k, g in ref["grads"].items():
        err = (gv[k].cpu().double() - g.double()).abs().max().item()
        worst = max(worst, (err - 1e-7) / max(g.abs().max().item(), 1e-30))
    e["grad_over_scale"] = worst
    e["panel_chain"] = eng.plan_query("panel_chain", True)
    return e


def _check(tag, form, e):
    _errors[f"{tag} {form}"] = e
    print(f"{tag} {form}: {e}")
    assert e["positions_equal"] and e["actions_equal"], e
    for k in ("step_preds", "step_log_probas", "step_values"):
        assert e[k] <= TOL_OUT, (k, e)
    assert e["loss"] <= TOL_LOSS * e["loss_scale"], e
    assert e["grad_over_scale"] <= TOL_GRAD, e


@pytest.fixture(scope="module")
def references():
    return {tag: _reference(cfg) for tag, cfg in PARITY_MODELS.items()}


@pytest.fixture(scope="module")
def unchained(references, tmp_path_factory):
    """every width once more in ONE child process under MARL_PANEL_CHAIN=0 (the switch is read once per process)"""
    d = tmp_path_factory.mktemp("panel_wfrag")
    th.save(references, str(d / "refs.pt"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(d)], cwd=ROOT, capture_output=True, text=True,
                       env=dict(os.environ, MARL_PANEL_CHAIN="0"), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(d / "achieved.json") as f:
        return json.load(f)


@pytest.fixture(scope="module", autouse=True)
def _error_record():
    yield
    path = os.environ.get("MARL_PANEL_WFRAG_ERRORS")
    if path and _errors:
        with open(path, "w") as f:
            json.dump({"tolerances": {"outputs": TOL_OUT, "loss": TOL_LOSS, "grad_over_scale": TOL_GRAD},
                       "episode": {"agents": NA, "images": NB, "steps": NS}, "cases": _errors}, f, indent=1,
                      sort_keys=True)


@gpu
@pytest.mark.parametrize("tag", list(PARITY_MODELS))
def test_parity_chained(device, references, tag):
    e = _achieved(PARITY_MODELS[tag], references[tag], device)
    assert e["panel_chain"] == 1, e  # (every width is inside the chained plan's range: it must be what ran)
    _check(tag, "chained", e)


@gpu
@pytest.mark.parametrize("tag", list(PARITY_MODELS))
def test_parity_unchained(unchained, tag):
    e = unchained[tag]
    assert e["panel_chain"] == 0, e
    _check(tag, "MARL_PANEL_CHAIN=0", e)


# ---- GPU: refusal ---------------------------------------------------------------------------------------------------
@gpu
def test_step_entry_refuses_a_null_weights_workspace(device):
    from tests.util import uniform_params

    cfg = LAYOUT_MODELS["ktail40"]
    eng = _engine(cfg, device, ns=1)
    eng.pack({k: v.to(device) for k, v in uniform_params(cfg, 3).items()})
    c = eng.cfg
    na, nb = c.nb_agents, c.batch
    f = lambda *s: th.rand(*s, device=device)  # noqa: E731
    ins = [f(na, nb, SHAPE[0], cfg.window, cfg.window), f(na, nb, cfg.n_m), f(na, nb, 2), f(na, nb, cfg.n_b),
           f(na, nb, cfg.n_b), f(na, nb, cfg.n_a), f(na, nb, cfg.n_a)]
    outs = [th.full(s, 7.0, device=device) for s in ((na, nb, c.nb_action), (na, nb), (na, nb, c.nb_class),
                                                      (na, nb, cfg.n_m), (na, nb, cfg.n_b), (na, nb, cfg.n_b),
                                                      (na, nb, cfg.n_a), (na, nb, cfg.n_a))]
    ews = eng.episode_ws(False)
    wws = eng.weights_ws()
    rc = eng.lib.marl_step_forward(C.byref(c), None, wws.numel() * 4, ews.data_ptr(), ews.numel() * 4,
                                   *[t.data_ptr() for t in ins], *[t.data_ptr() for t in outs], None, 0, 0, None, None,
                                   None)
    th.cuda.synchronize()
    assert rc != 0
    for t in outs:
        assert bool((t == 7.0).all()), "a refused call wrote an output"


if __name__ == "__main__":  # the child of `unchained`: achieved errors of every width -> <dir>/achieved.json
    d = sys.argv[1]
    refs = th.load(os.path.join(d, "refs.pt"))
    dev = th.device("cuda:0")
    res = {tag: _achieved(PARITY_MODELS[tag], refs[tag], dev) for tag in PARITY_MODELS}
    with open(os.path.join(d, "achieved.json"), "w") as fh:
        json.dump(res, fh)
