"""Helpers shared by the tests: golden-fixture loading (tests/golden/*.npz, written by
oracle/make_golden.py from the real reference) and the oracle <-> engine glue."""
import os

import numpy as np
import torch as th

from oracle import marl_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUND = "r06"  # prefix of the parity records the GPU tests write (copied into profiles/ after the box run)


def record(name, obj):
    """Achieved-error / margin records of the GPU parity tests -> gpurun_out/<ROUND>_<name>.json (gpurun_out/ is
    what comes back from the GPU box; tools/round_profiles.sh copies these into profiles/)."""
    import json

    path = os.path.join(ROOT, "gpurun_out")
    try:
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, f"{ROUND}_{name}.json"), "w") as f:
            json.dump(obj, f, indent=1)
    except OSError:
        pass

CASES = {
    "g1_conftest": mo.OracleConfig("mnist", 12, 23, 22, 21, 20, 19, 10, 24, 25),
    "g2_mnist_c1": mo.OracleConfig("mnist", 6, 64, 64, 16, 24, 8, 10, 96, 96),
    "g3_mnist_ckpt": mo.OracleConfig(
        "mnist", 6, 80, 80, 16, 24, 8, 10, 112, 112,
        actions=[[1, 0], [-1, 0], [0, 1], [0, -1], [0, 0]],
    ),
    "g4_resisc_b2": mo.OracleConfig("resisc45", 12, 256, 256, 64, 96, 16, 45, 384, 384),
}


def uniform_params(cfg, seed):
    """Same machine-independent init as oracle/make_golden.py::uniform_params."""
    g = th.Generator().manual_seed(seed)
    out = {}
    for name, shape in mo.param_shapes(cfg).items():
        r = th.rand(shape, generator=g) * 2 - 1
        if len(shape) >= 2:
            fan_in = int(np.prod(shape[1:]))
            out[name] = r * (3.0 / fan_in) ** 0.5
        elif name.endswith(".weight"):
            out[name] = 1.0 + 0.1 * r
        else:
            out[name] = 0.1 * r
    return out


class Golden:
    def __init__(self, tag):
        self.tag = tag
        self.cfg = CASES[tag]
        z = np.load(os.path.join(GOLDEN, tag + ".npz"))
        self.z = z
        self.na, self.nb, self.ns, self.seed = (int(v) for v in z["meta_na_nb_ns_seed"])
        self.lr, self.gamma = (float(v) for v in z["meta_lr_gamma"])
        if "img" in z:
            self.img = th.from_numpy(z["img"])
        else:
            s = [int(v) for v in z["img_seed_shape"]]
            self.img = th.rand(*s[1:], generator=th.Generator().manual_seed(s[0]))
        self.y = th.from_numpy(z["y"])
        self.inp = mo.EpisodeInputs(*(th.from_numpy(z[k]) for k in ("pos0", "h0", "c0", "hc0", "cc0", "q")))
        if any(k.startswith("param/") for k in z.files):
            self.params = {k: th.from_numpy(z["param/" + k]) for k in mo.param_shapes(self.cfg)}
        else:
            self.params = uniform_params(self.cfg, int(z["params_uniform_seed"][0]))
        chk = sum(v.double().sum().item() for v in self.params.values())
        assert abs(chk - float(z["params_checksum"][0])) < 1e-6 * max(1.0, abs(chk)), "fixture params drifted"
        self.has_full_grads = any(k.startswith("grad/") for k in z.files)

    def ref(self, key):
        return th.from_numpy(self.z["ref_" + key])

    def grad(self, name):
        return th.from_numpy(self.z["grad/" + name])

    def after(self, name):
        return th.from_numpy(self.z["after/" + name])


def model_spec(cfg):
    from marlclassification_amd.engine import ModelSpec

    return ModelSpec(cfg.ft_extr, cfg.window, cfg.n_b, cfg.n_a, cfg.n_m, cfg.n_m_o, cfg.n_d,
                     cfg.nb_class, cfg.nlb, cfg.nla, [list(a) for a in cfg.actions])


def small_model_config(**kw):
    """The ModelConfig of the host tests of the communication options (MNIST extractor, odd widths)."""
    from marlclassification_amd.config import ModelConfig

    return ModelConfig(ft_extr_str="mnist", window_size=6, hidden_size_belief=12, hidden_size_action=10,
                       hidden_size_msg=8, hidden_size_msg_output=9, hidden_size_state=4, state_dim=2,
                       actions=[[1, 0], [-1, 0], [0, 1], [0, -1]], nb_class=10, hidden_size_linear_belief=16,
                       hidden_size_linear_action=16, **kw)


def slice_case(g, nb):
    """(images, episode inputs) of the first ``nb`` images of a golden case"""
    i = g.inp
    return (g.img[:nb], mo.EpisodeInputs(i.pos0[:, :nb].contiguous(), i.h0[:, :nb].contiguous(),
                                         i.c0[:, :nb].contiguous(), i.hc0[:, :nb].contiguous(),
                                         i.cc0[:, :nb].contiguous(), i.q[:, :, :nb].contiguous()))


def run_update(eng, g, device, nb, train=True):
    """Episode, loss and backward of the first ``nb`` images on ``eng``: (episode outputs, gradients on the host)"""
    img, i = slice_case(g, nb)
    eng.configure(g.na, nb, g.ns, g.img.shape[1:])
    out = eng.episode_forward(img.to(device), i.pos0.to(device), i.h0.to(device), i.c0.to(device), i.hc0.to(device),
                              i.cc0.to(device), i.q.to(device), None, train)
    gp, gl, gv, sc, _ = eng.a2c_loss(out, g.y[:nb].to(device), g.gamma)
    grads = {k: th.zeros_like(v, device=device) for k, v in g.params.items()}
    eng.episode_backward(gp, gl, gv, grads)
    return out, {k: v.cpu() for k, v in grads.items()}


# every tuning knob of the library and its default (tests/test_gpu_round6.py moves each off it; the host test of the
# knob table checks the set against the sources)
KNOB_DEFAULTS = {"g3": 1, "g3_lstm": 1, "g3_tn": 1, "g3_min_units": 64, "g3_safe": 0, "mfma_split": 1, "g3_lstm_variant": 0,
                 "g3_nt_variant": 0, "g3_tn_variant": 0, "g3_tn_cell": 1, "g3_tn_pipe": 1, "g3_tn_wgs": 256, "nt_xcd": 1, "tn_xcd": 1,
                 "panel_chain": 1, "red_defer": 3, "tn_split_waves": 8, "wgrad3": 1, "cnn_fwd2": 1, "cnn_fwd3": 1, "dgrad_wgs": 0,
                 "dgrad_min_chunks": 512}


def library_knobs():
    """(the keys of every tune_get("...") in the library's sources, the table marl_tune accepts keys from)"""
    import glob
    import re

    root = os.path.join(ROOT, "marlclassification_amd", "csrc")
    found = set()
    for f in glob.glob(os.path.join(root, "*.hip")):
        found |= set(re.findall(r'tune_get\("([a-z0-9_]+)"', open(f, encoding="utf-8").read()))
    src = open(os.path.join(root, "rowops.hip"), encoding="utf-8").read()
    table = re.search(r"kKnownKnobs\[\] = \{(.*?)\};", src, re.S).group(1)
    return found, re.findall(r'"([a-z0-9_]+)"', table)


# ---- plan witnesses (marl_plan_query: host arithmetic, answers without a GPU) ---------------------------------------
def cdiv(a, b):
    return -(-a // b)


def plan_witness(cfg, na, nb, ns, shape, train=True):
    """Every marl_plan_query key for this model and batch under the current knobs, plus R = na * nb rows, NR = ns * R
    and L conv layers: what the launchers WILL do (each value from the launcher's own routine)."""
    import ctypes as C

    from marlclassification_amd import _lib

    lib = _lib.load()
    mc = model_spec(cfg).config(na, nb, ns, *shape)
    L = len(cfg_groups(cfg))
    keys = ["g3", "g3_model", "g3_lstm", "g3_tn", "g3_tn_cell", "g3_tn_pipe", "wgrad3", "lstm_plan", "small_r",
            "panel_chain", "panel_sample", "comm_form", "cnn_fwd", "cnn_fwd_rb", "cnn_fwd_blocks"]
    keys += [f"cnn_dgrad_rb{l}" for l in range(1, L)]
    keys += [f"cnn_wgrad_{f}{l}" for l in range(L) for f in ("rb", "chunks", "blocks")]
    out = {"R": na * nb, "NR": ns * na * nb, "L": L}
    for k in keys:
        v = C.c_int(-1)
        _lib.check(lib.marl_plan_query(C.byref(mc), int(train), k.encode(), C.byref(v)))
        out[k] = v.value
    return out


def cfg_groups(cfg):
    from marlclassification_amd.engine import CNN_SPECS

    return CNN_SPECS[cfg.ft_extr][1]


def assert_witness(w, conditions):
    """`conditions`: Python expressions over the keys of plan_witness (and cdiv); each must hold."""
    for cond in conditions:
        assert eval(cond, {**w, "cdiv": cdiv, "w": w}), (cond, w)  # noqa: S307


_STEP2 = [[2, 0], [-2, 0], [0, 2], [0, -2]]
_RESISC16 = mo.OracleConfig("resisc45", 16, 128, 128, 32, 48, 16, 45, 192, 192)
# Distinct-image oracle parity (distinct_image_parity below) at the SMALLEST row counts R = agents * images * copies at
# which the row-gated CNN plans engage - 256 chunks x rb for the general cnn_fwd_kernel, more than 256 chunks for the
# cnn_fwd2 walk, 512 chunks x rb for the layer backward - none of them a workload size.
# tag: (config, agents, DISTINCT images, copies of each, steps, image shape)
PLAN_CASES = {
    "mnist6_b1024": (mo.OracleConfig("mnist", 6, 64, 64, 16, 24, 8, 10, 96, 96), 3, 16, 64, 5, (3, 28, 28)),
    "mnist12_odd_ragged": (CASES["g1_conftest"], 5, 7, 59, 4, (1, 28, 28)),
    "mnist10_general": (mo.OracleConfig("mnist", 10, 64, 64, 16, 24, 8, 10, 96, 96), 7, 5, 59, 3, (3, 28, 28)),
    "resisc16_general": (_RESISC16, 8, 7, 23, 3, (3, 64, 72)),
    # (8 x 21 copies, R = 1344 = 32 * 42: the image GEMMs need R % 32 == 0, and 1280 rows would be whole chunks of 5)
    "resisc16_general_g3": (_RESISC16, 8, 8, 21, 3, (3, 64, 72)),
    "worldstrat16": (mo.OracleConfig("worldstrat", 16, 48, 40, 16, 24, 8, 6, 56, 64, actions=_STEP2),
                     4, 7, 37, 3, (3, 72, 80)),
    "c3_partial_batch": (CASES["g4_resisc_b2"], 16, 15, 17, 4, (3, 256, 256)),
    "ckpt768_b64": (mo.OracleConfig("resisc45", 12, 768, 512, 64, 96, 16, 45, 768, 758), 4, 8, 8, 3, (3, 40, 48)),
}
# what each case is there for.  A changed threshold fails here, loudly, instead of moving the case onto another plan.
PLAN_WITNESS = {
    # BASELINE configs[1] (Fwd2Mnist6 at B = 1024): 384 chunks on 256 workgroups, image GEMMs on
    "mnist6_b1024": ["R == 3072", "cnn_fwd == 2", "cnn_fwd_rb == 8", "cnn_fwd_blocks == 256",
                     "cnn_fwd_blocks < cdiv(R, 8)", "g3 == 1", "cnn_dgrad_rb1 == 8"],
    # Fwd2Mnist12 on G1's odd widths: the walk with a one-row last chunk, fp32-operand GEMMs at scale
    "mnist12_odd_ragged": ["R == 2065", "cnn_fwd == 3", "cnn_fwd_blocks == 256", "cnn_fwd_blocks < cdiv(R, 8)",
                           "R % 8 == 1", "g3 == 0", "cnn_dgrad_rb1 == 8"],
    # a window none of the instantiations covers: the general kernel, 8 patches per workgroup, one-row last chunk
    "mnist10_general": ["R == 2065", "cnn_fwd == 6", "cnn_fwd_rb == 8", "R % cnn_fwd_rb != 0",
                        "cnn_fwd_blocks == cdiv(R, cnn_fwd_rb)", "cnn_dgrad_rb1 == 8"],
    # three layers, window 16: an ODD rb (5), a ragged last chunk, multi-patch layer backward on every layer
    "resisc16_general": ["R == 1288", "cnn_fwd == 6", "cnn_fwd_rb == 5", "R % cnn_fwd_rb != 0", "g3 == 0",
                         "cnn_dgrad_rb1 == 5", "cnn_dgrad_rb2 == 7", "wgrad3 == 1"],
    "resisc16_general_g3": ["R == 1344", "cnn_fwd == 6", "cnn_fwd_rb == 5", "R % cnn_fwd_rb != 0", "g3 == 1",
                            "cnn_dgrad_rb1 == 5", "cnn_dgrad_rb2 == 7", "wgrad3 == 1"],
    # five layers: the general kernel at rb = 4; the layer backward that undoes the 16-group GroupNorm (launch 4:
    # conv layer 4's transposed convolution + layer 3's normalisation) takes the col2im fallback - 16 groups do not
    # divide the kernel's 8 lane groups - while launches 1..3 (2 / 4 / 8 groups) run multi-patch.  (Layer 4's own
    # 32-group normalisation is undone by the row kernel ahead of every plan: there is no launch 5.)
    "worldstrat16": ["R == 1036", "cnn_fwd == 6", "cnn_fwd_rb == 4", "R % cnn_fwd_rb == 0", "cnn_dgrad_rb4 == 0",
                     "cnn_dgrad_rb1 == 5", "cnn_dgrad_rb2 == 6", "cnn_dgrad_rb3 == 6", "cnn_wgrad_rb4 == 12"],
    # a flagship model on an epoch's last partial batch (B = 255): fp32-operand GEMMs at flagship widths
    "c3_partial_batch": ["R == 4080", "R % 32 != 0", "g3 == 0", "cnn_fwd == 1", "cnn_fwd_blocks == 256",
                         "cnn_fwd_blocks < cdiv(R, 8)", "cnn_dgrad_rb1 == 8", "cnn_dgrad_rb2 == 8"],
    # the README checkpoint widths at a batch where the image GEMMs are on but the image weight gradients are not
    "ckpt768_b64": ["R == 256", "g3 == 1", "g3_tn == 0", "g3_tn_pipe == 0", "panel_chain == 0", "comm_form == 2",
                    "cnn_fwd == 1"],
}
# must hold at EVERY shape
PLAN_INVARIANTS = ["cnn_fwd in (0, 1, 2, 3, 4, 5, 6)", "cnn_fwd == 0 or cnn_fwd_rb >= 1",
                   "cnn_fwd_blocks <= cdiv(R, max(cnn_fwd_rb, 1))",
                   "cnn_fwd != 6 or cnn_fwd_blocks == cdiv(R, cnn_fwd_rb)",
                   "all(w[f'cnn_wgrad_blocks{l}'] <= w[f'cnn_wgrad_chunks{l}'] for l in range(L))",
                   "all(w[f'cnn_wgrad_chunks{l}'] == (cdiv(NR, w[f'cnn_wgrad_rb{l}']) if w[f'cnn_wgrad_rb{l}'] else 0)"
                   " for l in range(L))",
                   "g3_tn_pipe <= g3_tn", "g3_tn <= g3", "g3 <= g3_model"]


# ---- distinct-image oracle parity at a full batch ----------------------------------------------------------------
ATOL = 1e-5


def distinct_image_parity(device, cfg, na, nd, ns, shape, rep, record_name, extra=None):
    """`nd` DIFFERENT oracle images (own pixels, start positions, initial states, sampling noise, labels) are laid
    out `rep` times each in a SHUFFLED order along the batch.  Every slot must reproduce the oracle's trajectory of
    ITS source image - positions bit for bit (teacher-forced to the oracle's actions), logits / log-probs / values
    within 1e-5 - and copies of one source image are bit-identical wherever they sit; with the oracle batch's
    advantage statistics (loss phase 2) the big batch's gradient is the oracle's: every entry within 1e-4 of its
    tensor's scale.  Writes the achieved errors and margins (plus `extra`) with record() and returns them."""
    import time

    from marlclassification_amd.engine import HipEngine

    def engine(nb):
        eng = HipEngine(model_spec(cfg), device)
        eng.configure(na, nb, ns, shape)
        eng.pack({k: v.to(device) for k, v in params.items()})
        return eng

    params = uniform_params(cfg, 7)
    img = th.rand(nd, *shape, generator=th.Generator().manual_seed(21))
    y = th.randint(0, cfg.nb_class, (nd,), generator=th.Generator().manual_seed(22))
    inp = mo.draw_episode_inputs(cfg, na, nd, ns, shape[1:], 23)
    tr, lo, grads = mo.train_iteration(params, cfg, img, y, inp, ns, 0.99)

    th.cuda.synchronize()
    t0 = time.perf_counter()
    small = [t.to(device) for t in (inp.pos0, inp.h0, inp.c0, inp.hc0, inp.cc0, inp.q)]
    eng1 = engine(nd)
    out1 = eng1.episode_forward(img.to(device), *small, tr.step_actions.to(device), True)
    stats = eng1.a2c_loss(out1, y.to(device), 0.99, phase=1)[4].clone()
    del eng1, out1

    nb = nd * rep
    src = th.arange(nd).repeat(rep)[th.randperm(nb, generator=th.Generator().manual_seed(24))]  # slot -> source image
    assert all(int((src == s).sum()) == rep for s in range(nd)) and not th.equal(src, th.arange(nd).repeat(rep))
    pick = lambda t, dim: t.index_select(dim, src)  # noqa: E731
    eng = engine(nb)
    big = [pick(inp.pos0, 1), pick(inp.h0, 1), pick(inp.c0, 1), pick(inp.hc0, 1), pick(inp.cc0, 1), pick(inp.q, 2)]
    out = eng.episode_forward(pick(img, 0).to(device), *[t.to(device) for t in big],
                              pick(tr.step_actions, 2).to(device), True)
    pos_equal = th.equal(out.step_pos.cpu(), pick(tr.step_pos, 2))
    errs = {}
    for name, got, ref in (("preds", out.step_preds, tr.step_preds), ("logp", out.step_log_probas, tr.step_log_probas),
                           ("values", out.step_values, tr.step_values)):
        errs[name] = (got.cpu().double() - pick(ref.detach(), 2).double()).abs().max().item()
    print(f"{record_name}: positions equal {pos_equal}, abs err {errs}")
    assert pos_equal, "a slot's positions differ from its source image's"
    for name, err in errs.items():
        assert err <= ATOL, (name, err)
    # copies of one source image are bit-identical wherever they sit in the batch
    first = [int((src == s).nonzero()[0]) for s in range(nd)]
    for name in ("step_preds", "step_log_probas", "step_values"):
        t = getattr(out, name).cpu()
        assert th.equal(t, t.index_select(2, th.tensor(first)).index_select(2, src)), f"{name}: copies differ"
    yb = pick(y, 0).to(device)
    bufs = eng.a2c_loss(out, yb, 0.99, phase=1)
    assert th.allclose(bufs[4], stats * rep, rtol=1e-9), (bufs[4], stats * rep)
    bufs[4].copy_(stats)  # standardize with the oracle batch's own n / sum / sum of squares
    gp, gl, gv, sc, _ = eng.a2c_loss(out, yb, 0.99, phase=2, bufs=bufs)
    loss_err = abs(sc[0].item() - lo.loss.item())
    loss_tol = 5e-5 * max(1.0, abs(lo.loss.item()))
    g_out = {k: th.zeros_like(v, device=device) for k, v in params.items()}
    eng.episode_backward(gp, gl, gv, g_out)
    bad, worst, n = {}, 0.0, 0
    for k, ref in grads.items():
        err = (g_out[k].cpu().double() - ref.double()).abs().max().item()
        scale = ref.abs().max().item()
        n += ref.numel()
        worst = max(worst, err / scale if scale > 1e-12 else 0.0)
        if not err <= 1e-4 * scale + 1e-7:
            bad[k.replace("_ModelsWrapper__", "")] = "%.2e/%.2e" % (err, scale)
    seconds = time.perf_counter() - t0
    print(f"{record_name}: loss err {loss_err:.3e} (tol {loss_tol:.3e}), worst gradient err / tensor scale {worst:.3e}, "
          f"GPU part {seconds:.2f} s")
    assert loss_err <= loss_tol
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())
    rec = {"batch": nb, "distinct_images": nd, "rows": na * nb, "positions_equal": True,
           "abs_err": errs, "abs_tolerance": ATOL, "loss_abs_err": loss_err, "loss_tolerance": loss_tol,
           "gradient_entries": n, "grad_max_err_over_tensor_scale": worst, "grad_tolerance": 1e-4,
           "margin": {"outputs": ATOL / max(errs.values()), "gradient": 1e-4 / max(worst, 1e-30),
                      "loss": loss_tol / max(loss_err, 6e-8 * max(1.0, abs(lo.loss.item())))},  # (floor: half an fp32 ulp)
           "gpu_seconds": seconds}
    rec.update(extra or {})
    record(record_name, rec)
    return rec
