"""GPU, round 5: (a) full-size parity on DISTINCT images (the tiled-replica tests of rounds 2-4 are
blind to cross-image indexing - every replica held the same images, states and noise), (b) the weights workspace
layout does not move with the batch, (c) a layout knob invalidates the weights workspace and makes
every packer pack again.  Everything goes through the C ABI."""
import ctypes as C

import pytest
import torch as th

from oracle import marl_oracle as mo
from tests.util import PLAN_INVARIANTS, Golden, assert_witness, distinct_image_parity, model_spec, plan_witness
from tests.util import run_update as _run

pytestmark = pytest.mark.gpu

C3_CFG = mo.OracleConfig("resisc45", 12, 256, 256, 64, 96, 16, 45, 384, 384)
C4_CFG = mo.OracleConfig("aid", 24, 256, 256, 64, 96, 16, 30, 320, 320, actions=[[3, 0], [-3, 0], [0, 3], [0, -3]])
C5_CFG = mo.OracleConfig("aid", 32, 256, 256, 64, 96, 16, 45, 384, 384, actions=[[4, 0], [-4, 0], [0, 4], [0, -4]])

# tag: (config, agents, DISTINCT images, steps, image shape, copies of each image) -> batch = images * copies
DISTINCT = {
    "c3_resisc_b256": (C3_CFG, 16, 16, 16, (3, 256, 256), 16),   # BASELINE configs[2] as benched: R = 4096
    "c4_aid_b32": (C4_CFG, 16, 8, 16, (3, 600, 600), 4),        # configs[3] at 32 images per GPU: R = 512
    "c5_synth_b32": (C5_CFG, 64, 4, 32, (3, 1024, 1024), 8),   # configs[4] at 32 per GPU: R = 2048, 64 agents
    # round 6: configs[3]'s weak-scaling variant, 256 images per GPU: R = 4096, AidCnn, stride 3
    "c4_aid_b256": (C4_CFG, 16, 8, 16, (3, 600, 600), 32),
}


# the plans each tag is there for (marl_plan_query, every value from the launcher's own routine), asserted AHEAD of the
# parity run: a changed threshold fails here instead of quietly moving the tag onto another plan
DISTINCT_WITNESS = {
    # 65 536 contraction rows: image GEMMs, image weight gradients (one launch per cell, phase-pipelined), the 128-row
    # LSTM tile plan, the chained panel launch; Fwd2Resisc walks 512 chunks on 256 workgroups; the layer backward and
    # the weight gradients run their largest chunks, persistent (blocks < chunks)
    "c3_resisc_b256": ["R == 4096", "g3 == 1", "g3_tn == 1", "g3_tn_cell == 1", "g3_tn_pipe == 1", "lstm_plan == 2",
                       "small_r == 0", "panel_chain == 1", "comm_form == 0", "cnn_fwd == 1", "cnn_fwd_blocks == 256",
                       "cnn_fwd_blocks < cdiv(R, cnn_fwd_rb)", "cnn_dgrad_rb1 == 8", "cnn_dgrad_rb2 == 8", "wgrad3 == 1",
                       "cnn_wgrad_rb0 == 4", "cnn_wgrad_rb1 == 7", "cnn_wgrad_rb2 == 8",
                       "all(w[f'cnn_wgrad_blocks{l}'] < w[f'cnn_wgrad_chunks{l}'] for l in range(3))"],
    # 8 192 contraction rows: the smallest batch with the per-cell image weight gradients, the gate-split small-R LSTM
    # plan; Fwd3Aid24 without a walk (128 groups of 4); four-layer backward at rb 2 / 5 / 8
    "c4_aid_b32": ["R == 512", "g3 == 1", "g3_tn == 1", "g3_tn_cell == 1", "lstm_plan == 3", "small_r == 1",
                   "panel_chain == 1", "comm_form == 0", "cnn_fwd == 4", "cnn_fwd_rb == 4",
                   "cnn_fwd_blocks == cdiv(R, 4)", "cnn_dgrad_rb1 == 2", "cnn_dgrad_rb2 == 5", "cnn_dgrad_rb3 == 8",
                   "wgrad3 == 1", "cnn_wgrad_blocks3 == 256", "cnn_wgrad_chunks3 == 1171"],
    # 64 agents: no chained launch (the mean while a panel stages, comm_form 1); Fwd3Aid32 walks 512 groups; window 32:
    # single-patch first layer backward, 65 536 one-patch weight-gradient chunks on 512 workgroups
    "c5_synth_b32": ["R == 2048", "g3 == 1", "g3_tn == 1", "g3_tn_cell == 1", "lstm_plan == 2", "small_r == 0",
                     "panel_chain == 0", "comm_form == 1", "cnn_fwd == 5", "cnn_fwd_blocks == 256",
                     "cnn_fwd_blocks < cdiv(R, cnn_fwd_rb)", "cnn_dgrad_rb1 == 1", "cnn_dgrad_rb2 == 3",
                     "cnn_dgrad_rb3 == 6", "cnn_wgrad_rb1 == 1", "cnn_wgrad_chunks1 == 65536", "cnn_wgrad_blocks1 == 512"],
    # configs[3] at 256 images: Fwd3Aid24 walks 1024 groups, the 128-row LSTM plan at stride 3
    "c4_aid_b256": ["R == 4096", "g3 == 1", "g3_tn == 1", "g3_tn_cell == 1", "lstm_plan == 2", "small_r == 0",
                    "panel_chain == 1", "comm_form == 0", "cnn_fwd == 4", "cnn_fwd_blocks == 256",
                    "cnn_fwd_blocks < cdiv(R, cnn_fwd_rb)", "cnn_dgrad_rb1 == 2", "cnn_dgrad_rb2 == 5",
                    "cnn_dgrad_rb3 == 8", "cnn_wgrad_blocks3 == 256", "cnn_wgrad_chunks3 == 9363"],
}


@pytest.mark.parametrize("tag", list(DISTINCT))
def test_full_size_parity_on_distinct_shuffled_images(device, tag):
    """`nd` DIFFERENT oracle images (own pixels, start positions, initial states, sampling noise, labels) are laid
    out `rep` times each in a SHUFFLED order along the batch, up to the benched batch size.  Every slot must
    reproduce the oracle's trajectory of ITS source image - positions bit for bit (teacher-forced to the oracle's
    actions), logits / log-probs / values within 1e-5 - so a kernel that reads image b +- k, averages the messages
    of a neighbouring image's agents or mixes rows across a tile boundary fails here (its neighbours are other
    images), which the identical-replica tests of rounds 2-4 could not see.  With the oracle batch's advantage
    statistics (loss phase 2) the big batch's gradient is the oracle's: every entry within 1e-4 of its tensor's
    scale.  The size-dependent plans (column-pass / 256 x 256 row contractions, 256 x 128 NT tiles, two-launch
    panels at 64 agents, split-K slab counts, small-R tile plans) all run on this data: DISTINCT_WITNESS says which,
    and the plan query confirms it first.  (The body is tests/util.py::distinct_image_parity.)"""
    cfg, na, nd, ns, shape, rep = DISTINCT[tag]
    w = plan_witness(cfg, na, nd * rep, ns, shape)
    assert_witness(w, DISTINCT_WITNESS[tag] + PLAN_INVARIANTS)
    distinct_image_parity(device, cfg, na, nd, ns, shape, rep, f"distinct_{tag}")


# ---- weights workspace: batch-independent layout, invalidated by layout knobs -------------------------
@pytest.mark.parametrize("order", [(2, 1, 2), (1, 2, 1)])
def test_weights_layout_does_not_move_with_the_batch(device, order):
    """with 16 agents, batch 2 gives R = 32 rows (image GEMMs on), batch 1 gives R = 16 (off).
    The weights workspace used to reserve the k16 weight images only in the first case, so every later parameter's
    packed copy moved with the batch: an epoch's last partial batch read weights packed in the other layout
    (silently wrong), or - in the opposite order - every call failed with MARL_ESIZE.  One engine, ONE pack, batches
    alternating without an optimiser step: each run must equal a fresh engine packed for that batch, bit for bit."""
    from marlclassification_amd import _lib
    from marlclassification_amd.engine import HipEngine

    g = Golden("g4_resisc_b2")
    params = {k: v.to(device) for k, v in g.params.items()}
    offs = {}
    eng = HipEngine(model_spec(g.cfg), device)
    eng.configure(g.na, order[0], g.ns, g.img.shape[1:])
    eng.pack(params)
    for nb in order:
        out, grads = _run(eng, g, device, nb)
        fresh = HipEngine(model_spec(g.cfg), device)
        fresh.configure(g.na, nb, g.ns, g.img.shape[1:])
        fresh.pack(params)
        ref_out, ref_grads = _run(fresh, g, device, nb)
        for name in ("step_pos", "step_actions", "step_preds", "step_log_probas", "step_values"):
            assert th.equal(getattr(out, name), getattr(ref_out, name)), (nb, name)
        for k in grads:
            assert th.equal(grads[k], ref_grads[k]), (nb, k)
        wb, eb = eng._sizes(True)
        o = []
        for idx in (_lib.P["LB_WIH"], _lib.P["POL_W0"], _lib.P["PRE_W1"]):
            off, ld = C.c_int64(0), C.c_int(0)
            _lib.check(eng.lib.marl_debug_buffer(C.byref(eng.cfg), 1, f"WP{idx}".encode(), 0, C.byref(off), C.byref(ld)))
            o.append(off.value)
        offs[nb] = (wb, tuple(o))
        v = C.c_int(0)
        _lib.check(eng.lib.marl_plan_query(C.byref(eng.cfg), 1, b"g3", C.byref(v)))
        assert v.value == (1 if nb == 2 else 0)  # (the two batches really are on different kernel families)
        _lib.check(eng.lib.marl_plan_query(C.byref(eng.cfg), 1, b"g3_model", C.byref(v)))
        assert v.value == 1
    assert offs[1] == offs[2], offs
    assert eng.weights_generation == 1, "the weights workspace was re-allocated between batches"


def test_layout_knob_invalidates_the_weights_workspace(device):
    """engine.tune() of a knob that decides which weight images exist (g3, g3_min_units,
    mfma_split) must drop the cached weights workspace too, and FusedA2C / ModelsWrapper.ensure_packed must pack
    again - the old buffer has the old layout and the old size."""
    from marlclassification_amd import engine as E
    from marlclassification_amd.fused import EpisodeDraws, FlatParams, FusedA2C

    g = Golden("g4_resisc_b2")
    eng = E.HipEngine(model_spec(g.cfg), device)
    eng.configure(g.na, g.nb, g.ns, g.img.shape[1:])
    flat = FlatParams({k: tuple(v.shape) for k, v in g.params.items()}, device)
    flat.load(g.params)
    fa = FusedA2C(eng, flat, g.lr, g.gamma)
    i = g.inp
    draws = EpisodeDraws(*(t.to(device) for t in (i.pos0, i.h0, i.c0, i.hc0, i.cc0, i.q)))
    img = g.img.to(device)
    try:
        ref = fa.rollout(img, draws, False)
        gen0, size0 = eng.weights_generation, eng.weights_ws().numel()
        E.tune("g3", 0)  # no weight images any more: smaller workspace, every later offset moves
        out = fa.rollout(img, draws, False)  # (must re-pack by itself)
        assert eng.weights_generation == gen0 + 1 and eng.weights_ws().numel() < size0
        assert th.equal(out.step_pos, ref.step_pos) and th.equal(out.step_actions, ref.step_actions)
        assert (out.step_preds - ref.step_preds).abs().max().item() <= 2e-5
        E.tune("g3", 1)  # ... and back: the workspace grows again (the old one would be MARL_ESIZE)
        out = fa.rollout(img, draws, False)
        assert eng.weights_generation == gen0 + 2 and eng.weights_ws().numel() == size0
        for name in ("step_pos", "step_actions", "step_preds", "step_log_probas", "step_values"):
            assert th.equal(getattr(out, name), getattr(ref, name)), name
    finally:
        E.tune("g3", 1)


def test_image_entry_points_refuse_empty_shapes(device):
    """ni / nj / rows <= 0 used to reach the split plan's division by the tile count (SIGFPE)."""
    from marlclassification_amd import _lib

    lib = _lib.load()
    assert lib.marl_gemm_tn_images_scratch(0, 16, 64) == 0 and lib.marl_gemm_tn_images_scratch(16, 0, 64) == 0
    assert lib.marl_gemm_tn_images_scratch(16, 16, 0) == 0 and lib.marl_gemm_tn_images_scratch(16, 16, 33) == 0
    buf = th.zeros(1024, device=device)
    p = buf.data_ptr()
    assert lib.marl_gemm_tn_images(p, p, p, 16, 0, 16, 64, None, p, 4096, None) == -1
    assert lib.marl_gemm_tn_images(p, p, p, 16, 16, 16, 0, None, p, 4096, None) == -1
    assert lib.marl_gemm_nt_images(p, p, None, p, 16, 0, 16, 16, 0, 0, None) == -1
    assert lib.marl_gemm_nt_images(p, p, None, p, 16, 32, 0, 16, 0, 0, None) == -1


# ---- conv weight gradient on the bf16 matrix pipe (csrc/cnn.hip, cnn_wgrad3_kernel) --------------------
@pytest.mark.parametrize("cin,cout,hin,G,rows", [(16, 32, 6, 2, 3000), (32, 64, 3, 4, 5000), (16, 32, 12, 2, 700),
                                                 (32, 64, 6, 4, 1500), (64, 128, 3, 8, 2100), (16, 32, 16, 2, 130),
                                                 (64, 128, 4, 8, 1037), (32, 64, 8, 4, 515)])
def test_conv_weight_gradient_bf16x6_matches_float64(device, cin, cout, hin, G, rows):
    """VERDICT r4 item 4 (first part): the 3x3 stride-2 weight gradients of the layers with >= 16 input channels
    (networks/vision.py:33-35 through loss.backward()) as six bf16 MFMA products per fp32 product.  Against the
    float64 convolution gradient of the recomputed layer input SiLU(GroupNorm(Z)): error no larger than 1.5x the
    exact-fp32-MFMA kernel's (knob wgrad3 = 0) on the same data, both within 2e-6 of the gradient's scale."""
    import torch.nn.functional as F

    from marlclassification_amd import _lib

    lib = _lib.load()
    gen = th.Generator().manual_seed(cin * 131 + cout + hin * 7 + rows)
    hout = (hin - 1) // 2 + 1
    P = hout * hout
    dz = th.randn(rows, P, cout, generator=gen)
    zin = th.randn(rows, hin * hin, cin, generator=gen) * 1.5 + 0.3
    zz = zin.view(rows, hin * hin, G, cin // G).double()
    mean = zz.mean(dim=(1, 3))
    rstd = 1.0 / th.sqrt(zz.var(dim=(1, 3), unbiased=False) + 1e-5)
    gst = th.stack([mean, rstd], -1).float().contiguous()
    gamma = 1 + 0.1 * th.randn(cin, generator=gen)
    beta = 0.1 * th.randn(cin, generator=gen)
    xh = (zz - gst[..., 0].double()[:, None, :, None]) * gst[..., 1].double()[:, None, :, None]
    x = F.silu(xh.reshape(rows, hin * hin, cin) * gamma.double() + beta.double()).view(rows, hin, hin, cin).permute(0, 3, 1, 2)
    wt = th.zeros(cout, cin, 3, 3, dtype=th.float64, requires_grad=True)
    y = F.conv2d(x, wt, stride=2, padding=1)
    (y * dz.view(rows, hout, hout, cout).permute(0, 3, 1, 2).double()).sum().backward()
    ref = wt.grad.permute(0, 2, 3, 1).reshape(cout, 9 * cin)  # [co][tap * cin + ci]
    ref_b = dz.double().sum(dim=(0, 1))

    d = lambda t: t.to(device).contiguous()  # noqa: E731
    dzd, zind, gstd, gd, bd = d(dz), d(zin), d(gst), d(gamma), d(beta)
    errs = {}
    try:
        for mode in (1, 0):
            _lib.check(lib.marl_tune(b"wgrad3", mode))
            sb = lib.marl_cnn_wgrad_scratch(rows, cin, cout, hin, G, 0)
            scratch = th.zeros(sb // 4 + 64, device=device)
            dw, db = th.zeros(cout, 9 * cin, device=device), th.zeros(cout, device=device)
            for _ in range(2):  # (run to run bit-identical: fixed-order reductions)
                _lib.check(lib.marl_cnn_wgrad(dzd.data_ptr(), None, 0, None, zind.data_ptr(), gstd.data_ptr(), gd.data_ptr(),
                                              bd.data_ptr(), rows, 1, 3, 64, 64, cin, cout, hin, G, dw.data_ptr(),
                                              db.data_ptr(), scratch.data_ptr(), scratch.numel() * 4, None))
                if _ == 0:
                    first = dw.clone()
            assert th.equal(first, dw)
            errs[mode] = ((dw.cpu().double() - ref).abs().max().item() / ref.abs().max().item(),
                          (db.cpu().double() - ref_b).abs().max().item() / ref_b.abs().max().item())
    finally:
        _lib.check(lib.marl_tune(b"wgrad3", 1))
    assert errs[1][0] <= 2e-6 and errs[0][0] <= 2e-6 and errs[1][1] <= 2e-6, errs
    assert errs[1][0] <= 1.5 * errs[0][0] + 2e-7, errs
