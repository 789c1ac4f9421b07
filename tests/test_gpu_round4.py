"""GPU, round 4: the ABI sees workspace sizes (MARL_ESIZE instead of out-of-bounds writes), a bf16x3 weight image
reaches a product only inside the operand its caller passes, and the image-GEMM path of the episode
(csrc/gemm3.hip) is the one the parity fixtures with R % 32 == 0 run - checked against the fp32-operand path on the
same episode."""
import ctypes as C

import pytest
import torch as th

from tests.util import Golden, model_spec

pytestmark = pytest.mark.gpu


def _engine(g, device):
    from marlclassification_amd.engine import HipEngine

    eng = HipEngine(model_spec(g.cfg), device)
    eng.configure(g.na, g.nb, g.ns, g.img.shape[1:])
    eng.pack({k: v.to(device) for k, v in g.params.items()})
    return eng


def _forward(eng, g, device, train=True):
    i = g.inp
    return eng.episode_forward(g.img.to(device), i.pos0.to(device), i.h0.to(device), i.c0.to(device),
                               i.hc0.to(device), i.cc0.to(device), i.q.to(device), None, train)


def _raw_forward(eng, g, device, wws, wbytes, ews, ebytes, train=1):
    """marl_episode_forward through ctypes with explicit workspace sizes; returns the status code"""
    from marlclassification_amd.engine import _stream

    i = g.inp
    t = [x.to(device).contiguous() for x in (g.img, i.pos0, i.h0, i.c0, i.hc0, i.cc0, i.q)]
    out = eng.new_outputs()
    return eng.lib.marl_episode_forward(
        C.byref(eng.cfg), wws.data_ptr(), wbytes, ews.data_ptr(), ebytes, *[x.data_ptr() for x in t], None, 0, 0, None,
        out.step_preds.data_ptr(), out.step_log_probas.data_ptr(), out.step_values.data_ptr(), out.step_pos.data_ptr(),
        out.step_actions.data_ptr(), train, _stream(device))


def test_workspace_sizes_are_checked_by_the_abi(device):
    """a buffer sized before a layout knob changed is refused with MARL_ESIZE (-4)"""
    from marlclassification_amd import engine as E

    g = Golden("g4_resisc_b2")  # R = 32: the image-GEMM layout (knob g3) adds the operand images
    try:
        E.tune("g3", 0)
        eng = _engine(g, device)
        wws, ews = eng.weights_ws(), eng.episode_ws(True)
        sz_w, sz_e = C.c_size_t(0), C.c_size_t(0)
        E.check(eng.lib.marl_workspace_sizes(C.byref(eng.cfg), 1, C.byref(sz_w), C.byref(sz_e)))
        wb, eb = sz_w.value, sz_e.value  # exactly what the layout needs (the wrapper may allocate more)
        assert wws.numel() * 4 >= wb and ews.numel() * 4 >= eb
        assert _raw_forward(eng, g, device, wws, wb, ews, eb) == 0
        assert _raw_forward(eng, g, device, wws, wb, ews, eb - 4) == -4
        assert _raw_forward(eng, g, device, wws, wb - 4, ews, eb) == -4
        assert b"workspace too small" in eng.lib.marl_last_error()
        eng.lib.marl_tune(b"g3", 1)  # (behind the wrapper's back: buffers of the old sizes are now too small)
        E.check(eng.lib.marl_workspace_sizes(C.byref(eng.cfg), 1, C.byref(sz_w), C.byref(sz_e)))
        assert sz_e.value > eb and sz_w.value > wb
        assert _raw_forward(eng, g, device, wws, wb, ews, eb) == -4
        grads = {k: th.zeros_like(v, device=device) for k, v in g.params.items()}
        rc = eng.lib.marl_episode_backward(C.byref(eng.cfg), wws.data_ptr(), wb, ews.data_ptr(), eb,
                                           g.img.to(device).data_ptr(), None, None, None, eng._table(grads), None)
        assert rc == -4
        rc = eng.lib.marl_a2c_loss_fwd_bwd(C.byref(eng.cfg), ews.data_ptr(), eb, *([ews.data_ptr()] * 4), C.c_float(0.9),
                                           *([ews.data_ptr()] * 5), 0, None)
        assert rc == -4
        rc = eng.lib.marl_pack_weights(C.byref(eng.cfg), eng._table({k: v.to(device) for k, v in g.params.items()}),
                                       wws.data_ptr(), wb, None)
        assert rc == -4
    finally:
        E.tune("g3", 1)


def test_gemm_nt_never_meets_a_stale_weight_image(device):
    """a host-side table fp32 address -> image used to outlive the episode call that filled it; a later
    marl_gemm_nt on the same addresses then multiplied by the OLD weights' image.  Now the image travels inside the
    B operand of the call that owns it, and marl_gemm_nt builds a plain operand: it never takes one."""
    from marlclassification_amd import _lib

    g = Golden("g2_mnist_c1")
    eng = _engine(g, device)
    _forward(eng, g, device)  # multiplies by the images of the weight copies inside weights_ws
    off, ld = C.c_int64(0), C.c_int(0)
    idx = _lib.P["POL_W0"]
    _lib.check(eng.lib.marl_debug_buffer(C.byref(eng.cfg), 1, f"WP{idx}".encode(), 0, C.byref(off), C.byref(ld)))
    n, k = g.cfg.nla, g.cfg.n_a
    w = eng.weights_ws()[off.value: off.value + n * ld.value].view(n, ld.value)
    new = th.randn(n, k, generator=th.Generator().manual_seed(1))
    w[:, :k] = new.to(device)  # the fp32 copy changes; the image next to it still holds the packed weights
    a = th.randn(200, k, generator=th.Generator().manual_seed(2))
    ad = th.zeros(200, ld.value, device=device)
    ad[:, :k] = a.to(device)
    cd = th.zeros(200, n, device=device)
    _lib.check(eng.lib.marl_gemm_nt(ad.data_ptr(), ld.value, w.data_ptr(), ld.value, None, cd.data_ptr(), n, 200, n, k,
                                    0, None))
    assert (cd.cpu().double() - a.double() @ new.double().t()).abs().max().item() < 1e-4


class image_path:
    """forces the image-GEMM path (csrc/gemm3.hip: LSTM, in-loop batch, heads, dU, the four large weight gradients
    incl. the 256 x 256 row-contraction kernel) on shapes whose defaults keep the fp32-operand kernels"""

    KNOBS = (("g3", 1), ("g3_min_units", 1), ("g3_tn", 2))

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        from marlclassification_amd import engine as E

        for k, v in self.KNOBS:
            E.tune(k, v if self.on else 0 if k == "g3" else v)

    def __exit__(self, *exc):
        from marlclassification_amd import engine as E

        E.tune("g3", 1)
        E.tune("g3_min_units", 64)
        E.tune("g3_tn", 1)


def test_reference_parity_on_the_forced_image_path(device):
    """the reference-golden checks of tests/test_gpu_episode.py with every large product on images: G2 (MNIST
    C1, R = 96) and G4 (RESISC45 dims, R = 32) - bit-exact positions / actions, logits 1e-5, gradients 1e-4,
    Adam 1e-3 lr.  (The default knobs switch this path on from 128-unit cells / 32768 rows: the benched-size
    tests of rounds 2 and 3 run it as shipped.)"""
    from marlclassification_amd import _lib
    from tests import episode_checks as E0

    with image_path():
        g = Golden("g2_mnist_c1")
        eng = _engine(g, device)
        sz = [C.c_size_t(0) for _ in range(4)]
        _lib.check(eng.lib.marl_workspace_sizes(C.byref(eng.cfg), 1, C.byref(sz[0]), C.byref(sz[1])))
        eng.lib.marl_tune(b"g3", 0)
        _lib.check(eng.lib.marl_workspace_sizes(C.byref(eng.cfg), 1, C.byref(sz[2]), C.byref(sz[3])))
        eng.lib.marl_tune(b"g3", 1)
        assert sz[0].value > sz[2].value and sz[1].value > sz[3].value, "image layout not selected"
        for train in (True, False):
            E0.rollout_matches_reference(device, "g2_mnist_c1", train)
        E0.backward_and_adam_match_reference(device, "g2_mnist_c1")
        E0.loss_and_output_gradients(device, "g2_mnist_c1")
        E0.backward_resisc_dims_gradient_samples(device)


@pytest.mark.parametrize("tag", ["g2_mnist_c1", "g4_resisc_b2"])
def test_image_gemm_path_equals_the_fp32_operand_path(device, tag):
    """same episode + backward with the knob g3 on (gate-gradient images, gemm3.hip products) and off: the six
    bf16 products are the same products in both kernels, the gradients agree to rounding"""
    from marlclassification_amd import engine as E

    g = Golden(tag)
    res = {}
    try:
        for mode in (0, 1):
            image_path(bool(mode)).__enter__()
            eng = _engine(g, device)
            out = _forward(eng, g, device)
            gp, gl, gv, sc, st = eng.a2c_loss(out, g.y.to(device), g.gamma)
            grads = {k: th.zeros_like(v, device=device) for k, v in g.params.items()}
            eng.episode_backward(gp, gl, gv, grads)
            res[mode] = (out, {k: v.cpu() for k, v in grads.items()})
    finally:
        image_path().__exit__()
    assert th.equal(res[0][0].step_actions, res[1][0].step_actions)
    worst = 0.0
    for k in res[0][1]:
        a, b = res[0][1][k].double(), res[1][1][k].double()
        worst = max(worst, (a - b).abs().max().item() / max(1e-30, a.abs().max().item()))
    assert worst <= 2e-5, worst


def test_persistent_cnn_backward_is_grid_independent(device):
    """cnn_dgrad_kernel walks the chunks of 8 patches with a resident grid: the same gradients whether one
    workgroup walks 17 chunks, a grid of its own size walks one each, or every patch is its own chunk - with
    a ragged last chunk (665 rows = 83 * 8 + 1) that rebuilds the tile tables.  dZ is the same arithmetic in
    every case; the affine partial sums are added in a grid-dependent (fixed per grid) order."""
    from marlclassification_amd import engine as E

    g = Golden("g1_conftest")
    res = {}
    try:
        for name, knobs in (("rb1", {}), ("grid5", {"dgrad_min_chunks": 1, "dgrad_wgs": 5}),
                            ("grid84", {"dgrad_min_chunks": 1, "dgrad_wgs": 100000})):
            E.tune("dgrad_min_chunks", knobs.get("dgrad_min_chunks", 512))
            E.tune("dgrad_wgs", knobs.get("dgrad_wgs", 0))
            eng = _engine(g, device)
            out = _forward(eng, g, device)
            gp, gl, gv, sc, st = eng.a2c_loss(out, g.y.to(device), g.gamma)
            grads = {k: th.zeros_like(v, device=device) for k, v in g.params.items()}
            E.check(eng.lib.marl_profile_begin(5, 64))  # class 5: the fused layer-backward launches
            eng.episode_backward(gp, gl, gv, grads)
            ms, n = C.c_double(0), C.c_int(0)
            E.check(eng.lib.marl_profile_end(C.byref(ms), C.byref(n)))
            assert n.value >= 1, "cnn_dgrad_kernel did not run on this shape"
            res[name] = {k: v.cpu().double() for k, v in grads.items()}
    finally:
        E.tune("dgrad_min_chunks", 512)
        E.tune("dgrad_wgs", 0)
    cnn = [k for k in res["rb1"] if "cnn" in k.lower() or "seq_conv" in k.lower()]
    assert cnn, list(res["rb1"])[:8]
    for other in ("grid5", "grid84"):
        worst = 0.0
        for k in res["rb1"]:
            a, b = res["rb1"][k], res[other][k]
            worst = max(worst, (a - b).abs().max().item() / max(1e-30, a.abs().max().item()))
        assert worst <= 2e-6, (other, worst)


@pytest.mark.parametrize("tag,rep", [("c4_aid", 16), ("c5_synth", 32)])
def test_full_size_c4_c5_replicas_match_the_oracle(device, tag, rep):
    """C4 / C5 had numeric oracle checks at B = 2 / 1 only.  The oracle's small case tiled
    along the batch to BASELINE.json's 32 images per GPU (C5: R = 2048 rows, 64 agents - the two-launch panel
    path, the column-pass row contractions and the split-K slab counts of the benched size): every replica
    reproduces the oracle's positions bit for bit (teacher-forced to its actions) and its logits / log-probs /
    values within 1e-5; with the un-tiled batch's advantage statistics (phase 2 of marl_a2c_loss_fwd_bwd) the
    tiled batch's gradient is the small batch's: every gradient entry within 1e-4 of its tensor's scale."""
    from marlclassification_amd.engine import HipEngine
    from oracle import marl_oracle as mo
    from tests.episode_checks import ATOL, BIG_CASES, _maxerr
    from tests.util import uniform_params

    cfg, na, nb, ns, shape = BIG_CASES[tag]
    params = uniform_params(cfg, 7)
    img = th.rand(nb, *shape, generator=th.Generator().manual_seed(11))
    y = th.randint(0, cfg.nb_class, (nb,), generator=th.Generator().manual_seed(12))
    inp = mo.draw_episode_inputs(cfg, na, nb, ns, shape[1:], 13)
    tr, lo, grads = mo.train_iteration(params, cfg, img, y, inp, ns, 0.99)

    def engine(batch):
        eng = HipEngine(model_spec(cfg), device)
        eng.configure(na, batch, ns, shape)
        eng.pack({k: v.to(device) for k, v in params.items()})
        return eng

    small = [t.to(device) for t in (inp.pos0, inp.h0, inp.c0, inp.hc0, inp.cc0, inp.q)]
    eng1 = engine(nb)
    out1 = eng1.episode_forward(img.to(device), *small, tr.step_actions.to(device), True)
    stats = eng1.a2c_loss(out1, y.to(device), 0.99, phase=1)[4].clone()
    del eng1, out1

    def tile(t, dim):
        return th.cat([t] * rep, dim=dim)

    eng = engine(nb * rep)
    big = [tile(inp.pos0, 1), tile(inp.h0, 1), tile(inp.c0, 1), tile(inp.hc0, 1), tile(inp.cc0, 1), tile(inp.q, 2)]
    out = eng.episode_forward(tile(img, 0).to(device), *[t.to(device) for t in big],
                              tile(tr.step_actions, 2).to(device), True)

    def replicas(t, bdim):  # [.., nb * rep, ..] -> [rep, .., nb, ..]
        s = list(t.shape)
        s[bdim:bdim + 1] = [rep, nb]
        return t.reshape(s).movedim(bdim, 0)

    pos = replicas(out.step_pos.cpu(), 2)
    assert th.equal(pos, tr.step_pos.expand_as(pos)), "positions of a replica differ"
    for name, got, ref in (("preds", out.step_preds, tr.step_preds), ("logp", out.step_log_probas, tr.step_log_probas),
                           ("values", out.step_values, tr.step_values)):
        r = replicas(got.cpu(), 2)
        assert (r.double() - ref.detach().double()).abs().max().item() <= ATOL, name
        assert th.equal(r[0], r[rep - 1]), f"{name}: replicas are not bit-identical"
    yb = tile(y, 0).to(device)
    bufs = eng.a2c_loss(out, yb, 0.99, phase=1)
    assert th.allclose(bufs[4], stats * rep, rtol=1e-9), (bufs[4], stats * rep)
    bufs[4].copy_(stats)  # standardize with the small batch's own n / sum / sum of squares
    gp, gl, gv, sc, _ = eng.a2c_loss(out, yb, 0.99, phase=2, bufs=bufs)
    assert abs(sc[0].item() - lo.loss.item()) <= 5e-5 * max(1.0, abs(lo.loss.item()))
    g_out = {k: th.zeros_like(v, device=device) for k, v in params.items()}
    eng.episode_backward(gp, gl, gv, g_out)
    bad = {}
    for k, ref in grads.items():
        err = _maxerr(g_out[k], ref)
        if not err <= 1e-4 * ref.abs().max().item() + 1e-7:
            bad[k.replace("_ModelsWrapper__", "")] = "%.2e/%.2e" % (err, ref.abs().max().item())
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())


@pytest.mark.parametrize("na,nb,ns,shape", [
    (2, 1, 1, (3, 28, 28)),     # one image, one step: no recurrence, no reverse loop
    (3, 1, 4, (3, 28, 28)),     # a single image: R = 3 rows, every kernel one ragged tile
    (5, 7, 1, (3, 28, 28)),     # one step, R = 35
    (16, 3, 2, (3, 40, 36)),    # 16 agents: the chained panels (all agents of an image per workgroup), ragged
    (17, 2, 2, (3, 40, 36)),    # one agent more than a 16-row panel holds: the unchained panel path
])
def test_edge_sizes_match_the_oracle(device, na, nb, ns, shape):
    """Smallest / ragged episode shapes (empty-ish and ragged inputs): teacher-forced rollout,
    loss and EVERY gradient against the oracle, then the free-running trajectory."""
    from oracle import marl_oracle as mo
    from tests.episode_checks import check_against_oracle, oracle_case, oracle_engine

    cfg = mo.OracleConfig("mnist", 6, 32, 32, 8, 12, 8, 10, 48, 48)
    params, img, y, inp = oracle_case(cfg, na, nb, ns, shape)
    eng = oracle_engine(cfg, device, na, nb, ns, shape, params)
    check_against_oracle(eng, cfg, device, params, img, y, inp, ns)
