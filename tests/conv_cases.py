"""What the conv kernel tests share: the buffers that surround every tensor with NaN / a sentinel, the relative error,
and the case tables with the plan witnesses of the backward (marl_cnn_bwd_plan) and forward (marl_cnn_fwd_plan)
launchers.  tests/test_conv_plan_host.py checks the tables without a GPU; tools/conv_plan_identity.py reads them too."""
import ctypes as C

import torch as th

PAD = 64  # floats (256 bytes) of NaN / sentinel on either side of every tensor: the kernels' 16-byte alignment holds
SENTINEL = -777.0


# ---- placement ---------------------------------------------------------------------------------------------------
def _embed(t, device):
    """`t` on the device inside a buffer whose surroundings are NaN (255 / a valid position for integer data)"""
    flat = t.reshape(-1)
    fill = float("nan") if t.is_floating_point() else (255 if t.dtype == th.uint8 else 0)
    buf = th.full((flat.numel() + 2 * PAD,), fill, dtype=t.dtype, device=device)
    buf[PAD:PAD + flat.numel()] = flat.to(device)
    return buf, buf[PAD:PAD + flat.numel()]


class _Out:
    """an output tensor inside a sentinel-filled buffer"""

    def __init__(self, shape, device):
        self.shape = shape
        self.n = 1
        for s in shape:
            self.n *= s
        self.buf = th.empty(self.n + 2 * PAD, device=device)
        self.reset()

    def reset(self):
        self.buf.fill_(SENTINEL)

    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def get(self):
        b = self.buf.cpu()
        assert th.all(b[:PAD] == SENTINEL) and th.all(b[PAD + self.n:] == SENTINEL), "wrote outside the tensor"
        inner = b[PAD:PAD + self.n]
        assert not th.any(inner == SENTINEL), "left part of the tensor unwritten"
        return inner.reshape(self.shape).clone()


def _rel(got, ref):
    return (got.double() - ref.double()).abs().max().item() / max(ref.abs().max().item(), 1e-30)


# ---- the backward grid -----------------------------------------------------------------------------------------------
# first-layer weight gradient (zin = NULL): name -> (cin, cout, window f, c_img, rows, nb, H, W, witness).  Every witness
# names the instantiation (sct, skt, pd); rows % rb != 0 wherever rb > 1, but in the one-row case.
WG_FIRST = {
    "mnist6": (1, 8, 6, 1, 37, 5, 28, 30, dict(form=1, sct=1, skt=1, ms=8, rb=16, pd=2, pi=4)),
    # MnistCnn on RGB data reads channel 0 only: channels 1 and 2 are NaN
    "mnist6_cimg3": (1, 8, 6, 3, 37, 5, 28, 30, dict(form=1, sct=1, skt=1, ms=8, rb=16, pd=2, pi=4)),
    "mnist6_one_row": (1, 8, 6, 1, 1, 3, 28, 30, dict(form=1, sct=1, skt=1, ms=8, rb=16, pd=2, pi=4)),
    "resisc12": (3, 16, 12, 3, 11, 3, 40, 44, dict(form=1, sct=1, skt=1, rb=4, tgk=2, ms=4, pd=2, pi=4)),
    "aid24": (3, 16, 24, 3, 5, 3, 50, 56, dict(form=1, sct=1, skt=1, rb=1, pd=2, pi=4)),
    "aid32_lean": (3, 16, 32, 3, 5, 3, 64, 72, dict(form=1, sct=1, skt=1, rb=2, pd=4, pi=14)),  # <1, 1, true, 4, 14>
    "cin4_skt3": (4, 16, 6, 4, 17, 5, 28, 30, dict(form=1, sct=1, skt=3, pd=2, rb=14)),
    "cout32_tgc2": (3, 32, 6, 3, 17, 5, 28, 30, dict(form=1, sct=1, skt=1, tgc=2, pd=2, rb=14)),
    # persistent: more chunks than the bound of workgroups (1024), which the launch trims further to what is resident
    "mnist6_persistent": (1, 8, 6, 1, 16 * 1024 + 16 + 5, 5, 28, 30,
                          dict(form=1, sct=1, skt=1, ms=8, rb=16, pd=2, chunks=1026, blocks=1024)),
}
# fp32 form on deeper layers: name -> (cin, cout, hin, G, rows, witness)
WG_DEEP = {
    "mnist_l1_h3": (8, 16, 3, 2, 37, dict(form=1, sct=1, skt=5, ms=8, pd=2, rb=16)),
    "mnist_l1_h6": (8, 16, 6, 2, 31, dict(form=1, sct=1, skt=5, ms=8, pd=2, rb=14)),
    "c4_c8_h4": (4, 8, 4, 1, 19, dict(form=1, sct=1, skt=3, pd=2, rb=16)),
    # WorldStrat's last layer: too many k tiles for the bf16x6 form's two slabs; 65 chunks (the last one of 3 rows) on
    # 64 workgroups x 8 k-slabs
    "worldstrat_l4": (128, 256, 2, 16, 451, dict(form=1, sct=2, skt=9, slabs=8, rb=7, chunks=65, blocks=64, pd=2)),
}
# layer backward: name -> (cin, cout, G, hin, witness): nt column tiles, mt1 row tiles of a one-patch chunk, rb_big = the
# chunk the launcher takes once dgrad_min_chunks = 1 lets it
DG_SHAPES = {
    "mnist_odd_side": (8, 16, 2, 3, dict(nt=1, mt1=1, rb_big=8)),
    "resisc_l1": (16, 32, 2, 6, dict(nt=1, mt1=3, rb_big=8)),
    "resisc_l2": (32, 64, 4, 3, dict(nt=2, mt1=1, rb_big=8)),
    "aid_l3_nt4": (64, 128, 8, 4, dict(nt=4, mt1=1, rb_big=6)),
    "aid_l1_mt16": (16, 32, 2, 16, dict(nt=1, mt1=16, rb_big=1)),
    "no_odd_positions": (16, 32, 2, 1, dict(nt=1, mt1=1, rb_big=8)),
    "small_edge": (16, 32, 2, 2, dict(nt=1, mt1=1, rb_big=8)),
    "odd_side_unequal_classes": (16, 32, 2, 5, dict(nt=1, mt1=2, rb_big=8)),
}


def bwd_plan(rows, cin, cout, hin, groups, first):
    from marlclassification_amd import _lib

    lib, check = _lib.load(), _lib.check
    p = _lib.CnnBwdPlan()
    check(lib.marl_cnn_bwd_plan(rows, cin, cout, hin, groups, first, C.byref(p)))
    return p.as_dict()


def assert_wgrad_witness(p, witness):
    got = {k: p["wg_" + k] for k in witness}
    assert got == witness, (got, witness, p)


# ---- the forward grid ------------------------------------------------------------------------------------------------
NB = 5  # distinct images of every case
MNIST, RESISC = ([1, 8, 16], [2, 4]), ([3, 16, 32, 64], [2, 4, 8])
AID, WORLDSTRAT = ([3, 16, 32, 64, 128], [2, 4, 8, 16]), ([3, 16, 32, 64, 128, 256], [2, 4, 8, 16, 32])
# no CNN_SPECS model: a half-filled second 16-channel tile (20 = 16 + 4), 12 channels per group, four input channels;
# its weight gradients are outside the activation-based kernel's range (512 % (cout / 4) != 0), so a training launch
# keeps the im2col rows of both layers
CUSTOM = ([4, 12, 20], [1, 5])
# name: (channels, groups), window f, image H x W (non-square; positions 0 .. H - f - 1), knobs
MODELS = {
    "resisc12": (RESISC, 12, 28, 30, {}),
    "mnist6": (MNIST, 6, 20, 22, {}),
    "mnist12": (MNIST, 12, 28, 30, {}),
    "aid24": (AID, 24, 40, 44, {}),
    "aid32": (AID, 32, 44, 48, {}),
    "mnist10": (MNIST, 10, 28, 30, {}),          # odd sides 5 -> 3
    "mnist7": (MNIST, 7, 20, 22, {}),            # odd window
    "resisc16": (RESISC, 16, 28, 30, {}),        # odd rb
    "aid20": (AID, 20, 40, 44, {}),
    "worldstrat16": (WORLDSTRAT, 16, 28, 30, {}),  # five layers, P = 1 in the last two, 32 groups
    "custom9": (CUSTOM, 9, 20, 22, {}),
    "custom4": (CUSTOM, 4, 12, 14, {}),          # the smallest configuration that keeps im2col rows (COLS_MIN)
    "mnist6_general": (MNIST, 6, 20, 22, {"cnn_fwd2": 0}),
    "aid24_general": (AID, 24, 40, 44, {"cnn_fwd3": 0}),
}
KNOB_TWIN = {"mnist6_general": "mnist6", "aid24_general": "aid24"}  # the specialised kernel of the same shape
_K0 = [0, 0, 0, 0, 0]
_KC = [1, 1, 0, 0, 0]  # custom9 in training mode


def _w(which, rb, blocks, image=0, cols=_K0):
    return dict(fused=1, which=which, rb=rb, blocks=blocks, keeps_cols=cols, writes_image=image)


# model -> {rows: witness of the training launch}.  cnn_fwd2 (which 1..3): 2065 rows = 259 chunks of 8 on 256 workgroups,
# workgroups 0..2 walk twice, the last chunk has one row.  cnn_fwd3 (4, 5): 1029 rows = 258 groups of 4 on 256
# workgroups, a one-row last group.  General kernel (6): rb = 1, then 2 with a one-row last chunk (511 = 255 * 2 + 1),
# then the largest rb inside the 52 KB cap that leaves 256 chunks, again with a one-row last chunk (2041 = 1 mod 2, 3,
# 4, 5, 6, 8).
GRID = {
    "resisc12": {1: _w(1, 8, 1, 1), 9: _w(1, 8, 2, 1), 2065: _w(1, 8, 256, 1)},
    "mnist6": {1: _w(2, 8, 1, 1), 9: _w(2, 8, 2, 1), 2065: _w(2, 8, 256, 1)},
    "mnist12": {1: _w(3, 8, 1), 9: _w(3, 8, 2), 2065: _w(3, 8, 256)},
    "aid24": {1: _w(4, 4, 1, 1), 5: _w(4, 4, 2, 1), 1029: _w(4, 4, 256, 1)},
    "aid32": {1: _w(5, 4, 1, 1), 5: _w(5, 4, 2, 1), 1029: _w(5, 4, 256, 1)},
    "mnist10": {1: _w(6, 1, 1), 511: _w(6, 2, 256), 2041: _w(6, 8, 256)},
    "mnist7": {1: _w(6, 1, 1), 511: _w(6, 2, 256), 2041: _w(6, 8, 256)},
    "resisc16": {1: _w(6, 1, 1), 511: _w(6, 2, 256), 2041: _w(6, 5, 409)},
    "aid20": {1: _w(6, 1, 1), 511: _w(6, 2, 256), 2041: _w(6, 3, 681)},
    "worldstrat16": {1: _w(6, 1, 1), 511: _w(6, 2, 256), 2041: _w(6, 4, 511)},
    "custom9": {1: _w(6, 1, 1, cols=_KC), 511: _w(6, 2, 256, cols=_KC), 2041: _w(6, 8, 256, cols=_KC)},
    "mnist6_general": {1: _w(6, 1, 1), 511: _w(6, 2, 256), 2041: _w(6, 8, 256)},
    "aid24_general": {1: _w(6, 1, 1), 511: _w(6, 2, 256), 2041: _w(6, 2, 1021)},
}
# image forms, one model per kernel family (and the MnistCnn instantiation for the RGB-data case): model -> rows
FORMS = {"resisc12": 9, "mnist6": 9, "aid24": 5, "mnist10": 511}
# kept im2col rows: the scan's candidates beyond CNN_SPECS, (channels, groups) - windows 4..32 - what it must find, and
# that configuration's cases {rows: witness} (rb = 1 at these row counts: 1 and rb + 1 rows)
COLS_EXTRA = {"custom": CUSTOM}
COLS_MIN = ("custom", 4, "custom4")
COLS_GRID = {1: _w(6, 1, 1, cols=_KC), 2: _w(6, 1, 2, cols=_KC)}


# ---- configurations and plans (host only) ----------------------------------------------------------------------------
def config(stack, f, H, W, nb=NB, c_img=None, u8=0):
    """marl_config of a conv stack: the rest of the model is as small as the library takes it"""
    from marlclassification_amd._lib import MarlConfig

    (ch, groups) = stack
    cfg = MarlConfig()
    cfg.nb_agents, cfg.batch, cfg.nb_steps = 1, nb, 1
    cfg.img_c, cfg.img_h, cfg.img_w = (c_img or ch[0]), H, W
    cfg.window, cfg.cnn_layers = f, len(groups)
    for i, c in enumerate(ch):
        cfg.cnn_ch[i] = c
    for i, g in enumerate(groups):
        cfg.cnn_groups[i] = g
    cfg.n_b = cfg.n_a = cfg.n_m = cfg.n_m_o = cfg.n_d = cfg.nlb = cfg.nla = 8
    cfg.nb_action, cfg.nb_class = 4, 4
    for j, a in enumerate([[1, 0], [-1, 0], [0, 1], [0, -1]]):
        cfg.actions[j][0], cfg.actions[j][1] = a
    cfg.img_u8 = u8
    return cfg


def model_config(model, **kw):
    stack, f, H, W, _ = MODELS[model]
    return config(stack, f, H, W, **kw)


def fwd_plan(cfg, train, rows):
    from marlclassification_amd import _lib

    p = _lib.CnnFwdPlan()
    _lib.check(_lib.load().marl_cnn_fwd_plan(C.byref(cfg), train, rows, C.byref(p)))
    return p.as_dict()


class knobs:
    """the knobs of a model for the length of a with block; the defaults (1) afterwards, whatever happens inside"""

    def __init__(self, model):
        self.k = MODELS[model][4]

    def __enter__(self):
        from marlclassification_amd import _lib

        for k, v in self.k.items():
            _lib.check(_lib.load().marl_tune(k.encode(), v))

    def __exit__(self, *exc):
        from marlclassification_amd import _lib

        for k in self.k:
            _lib.check(_lib.load().marl_tune(k.encode(), 1))


def smallest_cols_config():
    """the smallest configuration - by window, CNN_SPECS models first - whose fused training forward keeps the im2col
    rows of some layer: (name, stack, window, keeps_cols), or None"""
    from marlclassification_amd.engine import CNN_SPECS

    for f in range(4, 33):
        for name, stack in list(CNN_SPECS.items()) + list(COLS_EXTRA.items()):
            p = fwd_plan(config(stack, f, f + 8, f + 10), 1, 1)
            if p["fused"] and any(p["keeps_cols"]):
                return name, stack, f, p["keeps_cols"]
    return None
