"""The matrix-product launchers' cases shared by tests/test_gpu_kernels.py, tests/test_gpu_gemm_plans.py and
tests/test_gemm_plan_host.py: the variant tables with the planning hook (marl_gemm_plan; no GPU needed), the shapes and
variant ids of the image-product tests, and their bodies - the float64 references and the bounds NT_BOUND, TN_BOUND and
the cell's 1e-5 are stated once, here."""
import ctypes as C

import torch as th

KINDS = ("nt", "lstm", "tn", "nt_images", "lstm_images", "tn_images", "tn_images_cell")
DEFAULTS = {"mfma_split": 1, "g3_tn": 1, "g3_tn_pipe": 1, "nt_xcd": 1, "tn_xcd": 1, "tn_split_waves": 8,
            "g3_nt_variant": 0, "g3_lstm_variant": 0, "g3_tn_variant": 0}
# id -> (BM, BN, WM, WN, NST, pipelined); None: the row every other id takes (ids 4, 5, 6 of NT and 7 of LSTM exist
# in MARL_G3_ABLATE builds only: the default build sends them to that row too)
NT_ROWS = {1: (256, 128, 4, 2, 4, 0), 2: (128, 128, 2, 2, 3, 0), 7: (64, 64, 2, 2, 4, 0), 11: (128, 64, 4, 2, 3, 0),
           12: (64, 64, 2, 2, 3, 0), 21: (256, 256, 2, 4, 3, 1), 22: (256, 128, 4, 2, 4, 1), None: (128, 64, 2, 2, 4, 0)}
LSTM_ROWS = {1: (256, 128, 8, 1, 4, 0), 3: (32, 128, 1, 4, 4, 0), 4: (64, 128, 2, 4, 4, 0), 5: (256, 128, 4, 2, 4, 1),
             6: (256, 128, 2, 2, 4, 1), None: (128, 128, 4, 1, 3, 0)}
# id -> (BI, BJ, threads, ring of (BI + BJ) rows x stages); column passes (4) keep the 256 x 256 ring
TN_ROWS = {1: (256, 128, 512, (384, 4)), 2: (128, 128, 256, (256, 3)), 3: (256, 256, 512, (512, 3)),
           4: (256, 128, 512, (512, 3))}
VARIANT_IDS = {"g3_nt_variant": [1, 2, 4, 5, 6, 7, 11, 12, 21, 22, 3, 99],
               "g3_lstm_variant": [1, 2, 3, 4, 5, 6, 7, 99], "g3_tn_variant": [1, 2, 3, 4, 7]}
KNOB_SETTINGS = ([{}] + [{k: v} for k, v in (("mfma_split", 0), ("g3_tn", 2), ("g3_tn_pipe", 0), ("nt_xcd", 0),
                                              ("tn_xcd", 0), ("tn_split_waves", 4))] +
                 [{k: v} for k, ids in VARIANT_IDS.items() for v in ids])


def _lib():
    from marlclassification_amd import _lib as L

    return L


def hook(kind, m, n, k=None, rows=0, has_images=0, variant=0, rc_only=False):
    L = _lib()
    out, cnt = L.GemmPlan(), len(m)
    arr = lambda v: (C.c_int * cnt)(*v)  # noqa: E731
    rc = L.load().marl_gemm_plan(KINDS.index(kind), cnt, arr(m), arr(n), arr(k) if k else None, rows, has_images,
                                 variant, C.byref(out))
    if rc_only:
        return rc
    L.check(rc)
    return out.as_dict()


class knobs:
    """sets knobs through engine.tune, restores the defaults on exit"""

    def __init__(self, setting):
        self.setting = setting

    def __enter__(self):
        from marlclassification_amd import engine

        for k, v in self.setting.items():
            engine.tune(k, v)
        return {**DEFAULTS, **self.setting}

    def __exit__(self, *exc):
        from marlclassification_amd import engine

        for k in self.setting:
            engine.tune(k, DEFAULTS[k])


# ---- operands and bounds (GPU) ----------------------------------------------------------------------------------------
def _kernels():
    from marlclassification_amd import _lib

    return _lib.load(), _lib.check


def _p4(x):
    return (x + 3) & ~3


def _padded(t, ld):
    out = th.zeros(t.shape[0], ld, device=t.device)
    out[:, : t.shape[1]] = t
    return out


NT_SHAPES = [(96, 256, 160), (665, 92, 183), (37, 45, 24), (1, 4, 25), (4096, 512, 368), (3000, 130, 7),
             (300, 2048, 624), (32768 + 77, 368, 200)]  # last: many row blocks, ragged M and N
# error of a product in units of 2^-24 * max_ij sum_k |a_ik b_jk| (the natural scale of an fp32 dot product).
# Worst ratios measured on MI355X over the shapes below (profiles/r04_gemm_errors.json): NT 4.60 bf16x6 / 4.69
# fp32-MFMA, TN 0.97 / 0.97; the bounds are twice that.  (Round 3 allowed 2e-6 * max|C| * sqrt(k): ~10x the
# achieved error.)
NT_BOUND, TN_BOUND = 9.5, 2.0


def _dot_scale(a, b):
    return (a.abs().double() @ b.abs().double().t()).max().item() * 2.0 ** -24


def _image(lib, check, device, t, k):
    img = th.zeros(lib.marl_image_bytes(t.shape[0], k) + 256, dtype=th.uint8, device=device)
    check(lib.marl_image_build(t.data_ptr(), t.shape[1], t.shape[0], k, img.data_ptr(), None))
    return img


# ---- image GEMMs (csrc/gemm3.hip): shapes, variant ids (with their pytest ids) and the checks ---------------------------
NT_IMAGES_SHAPES = [(96, 256, 160), (665, 92, 183), (37, 45, 24), (4096, 512, 368),
                    (3000, 130, 7), (300, 2048, 624), (8192 + 77, 368, 200),
                    # the shapes of tools/g3_lab.py (a stale lab record showed wrong
                    # results on exactly these, under forced variants, and no test covered them)
                    (4096, 256, 1024), (65536, 384, 256), (4096, 1024, 624)]
NT_IMAGES_VARIANTS = {1: "256x128", 2: "128x128", 3: "128x64", 7: "64x64", 11: "128x64w8", 12: "64x64s3",
                      21: "256x256_pipelined", 22: "256x128_pipelined"}
LSTM_IMAGES_SHAPES = [(4096, 256, 368), (777, 23, 45), (96, 64, 96), (300, 80, 200), (512, 256, 624)]
LSTM_IMAGES_VARIANTS = {1: "256rows", 2: "128rows", 3: "32rows_gate_split", 4: "64rows_gate_split",
                        5: "256rows_pipelined_8waves", 6: "256rows_pipelined_4waves"}
TN_SHAPES = [(665, 92, 183), (5000, 16, 27), (20000, 200, 130), (33, 1, 24), (70000, 8, 9), (4096, 1024, 368),
             (9001, 300, 257), (65536, 384, 256)]
TN_IMAGES_SHAPES = [(4096, 1024, 368), (2048, 96, 80), (4096, 45, 384), (65536, 384, 256), (32, 7, 130), (8192, 512, 624)]
TN_IMAGES_VARIANTS = {1: "256x128", 2: "128x128", 3: "256x256", 4: "passes"}
CELL_IMAGES_SHAPES = [(32768, 256, 368, 256), (32768 + 96, 512, 624, 256), (32768, 256, 300, 200), (65536, 1024, 368, 256),
                      (32768, 768, 368, 192), (40000 - 40000 % 32, 300, 80, 256), (8192, 1024, 624, 256)]


def _within(err, bound, what):
    assert err <= bound, f"{what}: err {err:.3e}, bound {bound:.3e}"


def check_gemm_nt_images(device, m, n, k, variant, acc):
    lib, check = _kernels()
    g = th.Generator().manual_seed(m * 7 + n * 3 + k)
    a, b = th.randn(m, k, generator=g), th.randn(n, k, generator=g)
    bias, c0 = th.randn(n, generator=g), th.randn(m, n, generator=g)
    a3 = _image(lib, check, device, _padded(a.to(device), _p4(k)), k)
    b3 = _image(lib, check, device, _padded(b.to(device), _p4(k)), k)
    bias_d = bias.to(device)
    ldc = _p4(n) + 4
    ref = a.double() @ b.double().t() + bias.double() + (c0.double() if acc else 0)

    def run():
        cd = th.zeros(m, ldc, device=device)
        cd[:, :n] = c0.to(device)
        check(lib.marl_gemm_nt_images(a3.data_ptr(), b3.data_ptr(), bias_d.data_ptr(), cd.data_ptr(), ldc, m, n, k,
                                      acc, variant, None))
        return cd

    try:
        check(lib.marl_tune(b"g3_safe", 1))  # every K step fully waited for: the race-free reference
        safe = run()
    finally:
        check(lib.marl_tune(b"g3_safe", 0))
    for _ in range(3):
        cd = run()
        assert th.equal(cd, safe), "pipelined build differs from the fully-waited one"
    _within((cd[:, :n].cpu().double() - ref).abs().max().item(), NT_BOUND * _dot_scale(a, b), "C against float64")
    assert th.equal(cd[:, n:].cpu(), th.zeros(m, ldc - n)), "wrote outside [M, N]"


def check_lstm_images(device, m, n, nin, variant):
    """fused cell (networks/recurrent.py:19-35) from images against float64, and the image of h' it writes
    against the image of the h' it wrote in fp32"""
    lib, check = _kernels()
    g = th.Generator().manual_seed(m + n + nin)
    u, h, cprev = th.randn(m, nin, generator=g), th.randn(m, n, generator=g), th.randn(m, n, generator=g)
    wih, whh = th.randn(4 * n, nin, generator=g) / nin ** 0.5, th.randn(4 * n, n, generator=g) / n ** 0.5
    bias = th.randn(4 * n, generator=g)
    gates = u.double() @ wih.double().t() + h.double() @ whh.double().t() + bias.double()
    i_, f_, g_, o_ = gates.chunk(4, dim=1)
    c_ref = th.sigmoid(f_) * cprev.double() + th.sigmoid(i_) * th.tanh(g_)
    h_ref = th.sigmoid(o_) * th.tanh(c_ref)
    img = lambda t, k: _image(lib, check, device, _padded(t.to(device), _p4(k)), k)  # noqa: E731
    u3, h3, wih3, whh3 = img(u, nin), img(h, n), img(wih, nin), img(whh, n)
    cpd, bd = _padded(cprev.to(device), _p4(n)), bias.to(device)
    hn, cn = th.zeros(m, _p4(n), device=device), th.zeros(m, _p4(n), device=device)
    gt = th.zeros(m, _p4(4 * n), device=device)
    h3n = th.zeros(lib.marl_image_bytes(m, n) + 256, dtype=th.uint8, device=device)
    check(lib.marl_lstm_images(u3.data_ptr(), nin, h3.data_ptr(), wih3.data_ptr(), whh3.data_ptr(), bd.data_ptr(),
                               cpd.data_ptr(), hn.data_ptr(), cn.data_ptr(), gt.data_ptr(), h3n.data_ptr(), m, n,
                               _p4(n), _p4(4 * n), variant, 1, None))
    _within((hn[:, :n].cpu().double() - h_ref).abs().max().item(), 1e-5, "h'")
    _within((cn[:, :n].cpu().double() - c_ref).abs().max().item(), 1e-5, "c'")
    act = th.cat([th.sigmoid(i_), th.sigmoid(f_), th.tanh(g_), th.sigmoid(o_)], dim=1)
    _within((gt[:, : 4 * n].cpu().double() - act).abs().max().item(), 1e-5, "activated gates")
    assert th.equal(hn[:, n:].cpu(), th.zeros(m, _p4(n) - n)), "wrote the padding columns of h'"
    assert th.equal(gt[:, 4 * n:].cpu(), th.zeros(m, _p4(4 * n) - 4 * n)), "wrote the padding columns of the gates"
    nb = lib.marl_image_bytes(m, n)
    assert th.equal(_image(lib, check, device, hn, n)[:nb], h3n[:nb]), "the image of h' is not the image of the h' written"


def check_gemm_tn_images(device, rows, ni, nj, variant):
    lib, check = _kernels()
    g = th.Generator().manual_seed(rows + ni + nj)
    a, b = th.randn(rows, ni, generator=g), th.randn(rows, nj, generator=g)
    a3 = _image(lib, check, device, _padded(a.to(device), _p4(ni)), ni)
    b3 = _image(lib, check, device, _padded(b.to(device), _p4(nj)), nj)
    ldc = _p4(nj) + 4

    def run():
        sb = lib.marl_gemm_tn_images_scratch(ni, nj, rows)  # (the split plan depends on the tile plan)
        scratch = th.zeros(sb // 4 + 16, device=device)
        cd, cs = th.zeros(ni, ldc, device=device), th.zeros(ni, device=device)
        check(lib.marl_gemm_tn_images(a3.data_ptr(), b3.data_ptr(), cd.data_ptr(), ldc, ni, nj, rows, cs.data_ptr(),
                                      scratch.data_ptr(), sb, None))
        return cd, cs

    try:
        check(lib.marl_tune(b"g3_tn_variant", variant))
        check(lib.marl_tune(b"g3_safe", 1))
        safe, _ = run()
        check(lib.marl_tune(b"g3_safe", 0))
        cd, cs = run()
        assert th.equal(cd, safe) and th.equal(run()[0], safe), "pipelined build differs from the fully-waited one"
    finally:
        check(lib.marl_tune(b"g3_safe", 0))
        check(lib.marl_tune(b"g3_tn_variant", 0))
    unit = _dot_scale(a.t(), b.t())
    _within((cd[:, :nj].cpu().double() - a.double().t() @ b.double()).abs().max().item(), TN_BOUND * unit, "C against float64")
    _within((cs.cpu().double() - a.double().sum(0)).abs().max().item(),
            TN_BOUND * a.abs().double().sum(0).max().item() * 2.0 ** -24 * 4, "column sums")
    assert th.equal(cd[:, nj:].cpu(), th.zeros(ni, ldc - nj)), "wrote outside [NI, NJ]"


def check_gemm_tn_images_cell(device, rows, ni, nih, nhh):
    """both weight gradients of an LSTM cell from ONE launch (G's row slabs shared through the L2 of an XCD): against
    float64 within the row-contraction bound, bit-equal to its fully-waited build, column sums = bias gradient,
    nothing written outside [NI, NJ]"""
    lib, check = _kernels()
    gen = th.Generator().manual_seed(rows + ni + nih + nhh)
    g, u, h = th.randn(rows, ni, generator=gen), th.randn(rows, nih, generator=gen), th.randn(rows, nhh, generator=gen)
    g3 = _image(lib, check, device, _padded(g.to(device), _p4(ni)), ni)
    u3 = _image(lib, check, device, _padded(u.to(device), _p4(nih)), nih)
    h3 = _image(lib, check, device, _padded(h.to(device), _p4(nhh)), nhh)
    ld_ih, ld_hh = _p4(nih) + 4, _p4(nhh) + 8
    sb = lib.marl_gemm_tn_images_cell_scratch(ni, nih, nhh, rows)
    assert sb > 0, "the cell plan refuses this shape"

    def run():
        scratch = th.zeros(sb // 4 + 16, device=device)
        c_ih, c_hh, cs = th.zeros(ni, ld_ih, device=device), th.zeros(ni, ld_hh, device=device), th.zeros(ni, device=device)
        check(lib.marl_gemm_tn_images_cell(g3.data_ptr(), ni, u3.data_ptr(), nih, h3.data_ptr(), nhh, rows, c_ih.data_ptr(),
                                           ld_ih, c_hh.data_ptr(), ld_hh, cs.data_ptr(), scratch.data_ptr(), sb, None))
        return c_ih, c_hh, cs

    try:
        check(lib.marl_tune(b"g3_safe", 1))
        safe = run()
    finally:
        check(lib.marl_tune(b"g3_safe", 0))
    for _ in range(2):
        got = run()
        assert all(th.equal(a, b) for a, b in zip(got, safe)), "pipelined build differs from the fully-waited one"
    c_ih, c_hh, cs = got
    gd = g.double()
    _within((c_ih[:, :nih].cpu().double() - gd.t() @ u.double()).abs().max().item(), TN_BOUND * _dot_scale(g.t(), u.t()), "dW_ih")
    _within((c_hh[:, :nhh].cpu().double() - gd.t() @ h.double()).abs().max().item(), TN_BOUND * _dot_scale(g.t(), h.t()), "dW_hh")
    _within((cs.cpu().double() - gd.sum(0)).abs().max().item(), TN_BOUND * g.abs().double().sum(0).max().item() * 2.0 ** -24 * 4,
            "column sums")
    assert th.equal(c_ih[:, nih:].cpu(), th.zeros(ni, ld_ih - nih)), "wrote outside [NI, NIH]"
    assert th.equal(c_hh[:, nhh:].cpu(), th.zeros(ni, ld_hh - nhh)), "wrote outside [NI, NHH]"
    # (short contractions keep the per-product kernels)
    assert lib.marl_gemm_tn_images_cell_scratch(ni, nih, nhh, 4096) == 0, "a cell plan for a contraction of 4096 rows"
