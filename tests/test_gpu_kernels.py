"""GPU: kernel-level parity of libmarl_hip.so (called through the C ABI) against plain
torch fp32 / the golden known-answer vectors."""
import ctypes as C

import numpy as np
import pytest
import torch as th
import torch.nn.functional as F

from tests import gemm_cases as G
from tests.gemm_cases import NT_BOUND, NT_SHAPES, TN_BOUND, _dot_scale, _image, _p4, _padded
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu


def _lib():
    from marlclassification_amd import _lib

    return _lib.load(), _lib.check


@pytest.fixture(params=[1, 0], ids=["bf16x6", "f32mfma"])
def mfma_split(request):
    """Both forms of the matrix kernels: 1 = fp32 operands split into three bf16 terms, six bf16
    MFMA products (gemm_split.hip, the default); 0 = v_mfma_f32_32x32x2_f32 (gemm.hip)."""
    lib, check = _lib()
    check(lib.marl_tune(b"mfma_split", request.param))
    yield request.param
    check(lib.marl_tune(b"mfma_split", 1))


ERR_LOG = {}


def _run_nt(lib, check, device, a, b, bias, c0, acc, weights, guard):
    """one product through the C ABI; guard: A is followed by NaNs (an over-read would poison C)"""
    m, k = a.shape
    n = b.shape[0]
    lda = _p4(k) + 4
    ws = th.full((m * lda + 256,), float("nan"), device=device) if guard else th.zeros(m * lda + 256, device=device)
    ad = ws[: m * lda].view(m, lda)
    ad.zero_()
    ad[:, :k] = a.to(device)
    bd = _padded(b.to(device), _p4(k))
    ldc = n + 3
    cd = th.zeros(m, ldc, device=device)
    cd[:, :n] = c0.to(device)
    bias_d = bias.to(device)
    if weights:  # B as a weight matrix: pre-split image, the path every product of the episode takes
        img = th.zeros(lib.marl_gemm_weight_image_bytes(n, k) // 4 + 64, device=device)
        check(lib.marl_gemm_nt_weights(ad.data_ptr(), lda, bd.data_ptr(), bd.shape[1], bias_d.data_ptr(),
                                       cd.data_ptr(), ldc, m, n, k, acc, img.data_ptr(), None))
    else:
        check(lib.marl_gemm_nt(ad.data_ptr(), lda, bd.data_ptr(), bd.shape[1], bias_d.data_ptr(), cd.data_ptr(),
                               ldc, m, n, k, acc, None))
    th.cuda.synchronize()
    return cd


@pytest.mark.parametrize("m,n,k", NT_SHAPES)
@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("weights", [0, 1], ids=["plainB", "weightB"])
def test_gemm_nt(device, m, n, k, acc, weights):
    """Both forms of the NT kernels on the same operands (A tightly allocated, NaNs behind it): each within
    NT_BOUND of float64, and the bf16x6 form no worse than 1.5x the exact-fp32 MFMA form."""
    lib, check = _lib()
    g = th.Generator().manual_seed(m * 7 + n * 3 + k)
    a = th.randn(m, k, generator=g)
    b = th.randn(n, k, generator=g)
    bias = th.randn(n, generator=g)
    c0 = th.randn(m, n, generator=g)
    ref = a.double() @ b.double().t() + bias.double() + (c0.double() if acc else 0)
    unit = _dot_scale(a, b)
    err = {}
    try:
        for mode in (0, 1):
            check(lib.marl_tune(b"mfma_split", mode))
            cd = _run_nt(lib, check, device, a, b, bias, c0, acc, weights, guard=True)
            err[mode] = (cd[:, :n].cpu().double() - ref).abs().max().item()
            assert th.equal(cd[:, n:].cpu(), th.zeros(m, 3)), "wrote outside [M, N]"
    finally:
        check(lib.marl_tune(b"mfma_split", 1))
    ERR_LOG[f"nt m{m} n{n} k{k} acc{acc} w{weights}"] = (err[1] / unit, err[0] / unit)
    assert err[0] <= NT_BOUND * unit and err[1] <= NT_BOUND * unit, (err, unit)
    assert err[1] <= 1.5 * err[0] + 1e-3 * unit, f"bf16x6 error {err[1]:.3e} vs fp32-MFMA {err[0]:.3e}"


# x = x0 + x1 + x2 with three non-zero bf16 terms at distinct binary places, y likewise: the six kept
# products x0y0, x0y1, x1y0, x0y2, x1y1, x2y0 are six DIFFERENT powers of two (2^0, 2^-10, 2^-9, 2^-20,
# 2^-19, 2^-18), their sum is exactly representable in fp32, and the three dropped products (<= 2^-28)
# lie below half an ulp of it - so a kernel that loses, duplicates or swaps any product cannot produce
# the expected bits, and the exact-fp32 MFMA form must produce the same bits.
KAT_X = 1.0 + 2.0 ** -9 + 2.0 ** -18
KAT_Y = 1.0 + 2.0 ** -10 + 2.0 ** -20
KAT_XY = 1.0 + 2.0 ** -9 + 2.0 ** -10 + 2.0 ** -18 + 2.0 ** -19 + 2.0 ** -20


def _kat_operands(m, n, k):
    """A[i, i % k] = 2^(i % 5) x, B[j, j % k] = 2^-(j % 7) y, zeros elsewhere (one term per dot product)"""
    a, b = th.zeros(m, k, dtype=th.float64), th.zeros(n, k, dtype=th.float64)
    i, j = th.arange(m), th.arange(n)
    a[i, i % k] = KAT_X * 2.0 ** (i % 5).double()
    b[j, j % k] = KAT_Y * 2.0 ** -(j % 7).double()
    hit = (i[:, None] % k) == (j[None, :] % k)
    want = th.where(hit, KAT_XY * 2.0 ** (i % 5).double()[:, None] * 2.0 ** -(j % 7).double()[None, :],
                    th.zeros((), dtype=th.float64))
    assert th.equal(a.float().double(), a) and th.equal(want.float().double(), want)  # exact in fp32
    return a.float(), b.float(), want


@pytest.mark.parametrize("weights", [0, 1], ids=["plainB", "weightB"])
def test_gemm_nt_six_products_kat(device, mfma_split, weights):
    lib, check = _lib()
    m, n, k = 300, 200, 48
    a, b, want = _kat_operands(m, n, k)
    cd = _run_nt(lib, check, device, a, b, th.zeros(n), th.zeros(m, n), 0, weights, guard=False)
    assert th.equal(cd[:, :n].cpu().double(), want)


def test_gemm_tn_six_products_kat(device, mfma_split):
    lib, check = _lib()
    ni, nj, rows = 160, 136, 4096
    at, bt, want = _kat_operands(ni, nj, rows)  # [ni, rows], [nj, rows]: the contraction runs over rows
    ad, bd = _padded(at.t().contiguous().to(device), _p4(ni)), _padded(bt.t().contiguous().to(device), _p4(nj))
    cd = th.zeros(ni, _p4(nj), device=device)
    sb = lib.marl_gemm_tn_scratch(ni, nj, rows)
    scratch = th.zeros(sb // 4 + 16, device=device)
    check(lib.marl_gemm_tn(ad.data_ptr(), ad.shape[1], bd.data_ptr(), bd.shape[1], cd.data_ptr(), cd.shape[1],
                           ni, nj, rows, scratch.data_ptr(), sb, None))
    assert th.equal(cd[:, :nj].cpu().double(), want)


def test_gemm_nt_is_transpose_detecting(device, mfma_split):
    # asymmetric operands: A = identity-like rows selects rows of B exactly
    lib, check = _lib()
    m, n, k = 64, 96, 64
    a = th.eye(m, k)
    b = th.arange(n * k, dtype=th.float32).view(n, k) / 7.0
    cd = th.zeros(m, n, device=device)
    ad, bd = a.to(device), b.to(device)
    check(lib.marl_gemm_nt(ad.data_ptr(), k, bd.data_ptr(), k, None, cd.data_ptr(), n, m, n, k, 0,
                           None))
    th.cuda.synchronize()
    assert th.equal(cd.cpu(), b.t().contiguous()[:m])


@pytest.mark.parametrize("rows,ni,nj", G.TN_SHAPES)
def test_gemm_tn(device, rows, ni, nj):
    """The fp32-MFMA kernel and both forms of the bf16x6 kernel (knob tn_split_waves: 8 = 512 threads, one
    operand per thread while staging, the default; 4 = 256 threads) on the same operands."""
    lib, check = _lib()
    g = th.Generator().manual_seed(rows + ni + nj)
    a = th.randn(rows, ni, generator=g)
    b = th.randn(rows, nj, generator=g)
    ad, bd = _padded(a.to(device), _p4(ni)), _padded(b.to(device), _p4(nj) + 8)
    ldc = _p4(nj)
    ref = a.double().t() @ b.double()
    unit = _dot_scale(a.t(), b.t())

    def run():
        sb = lib.marl_gemm_tn_scratch(ni, nj, rows)  # (the split plan depends on the kernel form)
        scratch = th.zeros(sb // 4 + 16, device=device)
        cd = th.zeros(ni, ldc, device=device)
        check(lib.marl_gemm_tn(ad.data_ptr(), ad.shape[1], bd.data_ptr(), bd.shape[1], cd.data_ptr(),
                               ldc, ni, nj, rows, scratch.data_ptr(), sb, None))
        return cd

    err = {}
    try:
        for mode, waves in ((0, 8), (1, 8), (1, 4)):
            check(lib.marl_tune(b"mfma_split", mode))
            check(lib.marl_tune(b"tn_split_waves", waves))
            cd = run()
            err[mode, waves] = (cd[:, :nj].cpu().double() - ref).abs().max().item()
            assert th.equal(cd, run()), "not deterministic"
    finally:
        check(lib.marl_tune(b"mfma_split", 1))
        check(lib.marl_tune(b"tn_split_waves", 8))
    ERR_LOG[f"tn rows{rows} ni{ni} nj{nj}"] = (err[1, 8] / unit, err[0, 8] / unit)
    assert all(e <= TN_BOUND * unit for e in err.values()), (err, unit)
    assert max(err[1, 8], err[1, 4]) <= 1.5 * err[0, 8] + 1e-3 * unit, err


def test_record_gemm_errors():
    """(after the two tests above) the achieved error ratios -> gpurun_out/gemm_errors.json; the copy under
    profiles/ is what NT_BOUND / TN_BOUND quote"""
    import json
    import os

    if not ERR_LOG:
        pytest.skip("run together with test_gemm_nt / test_gemm_tn")
    os.makedirs("gpurun_out", exist_ok=True)
    worst = {"nt_bf16x6": max((v[0] for k, v in ERR_LOG.items() if k.startswith("nt")), default=0.0),
             "nt_f32mfma": max((v[1] for k, v in ERR_LOG.items() if k.startswith("nt")), default=0.0),
             "tn_bf16x6": max((v[0] for k, v in ERR_LOG.items() if k.startswith("tn")), default=0.0),
             "tn_f32mfma": max((v[1] for k, v in ERR_LOG.items() if k.startswith("tn")), default=0.0)}
    with open("gpurun_out/gemm_errors.json", "w") as f:
        json.dump({"unit": "max |C - float64| / (2^-24 * max_ij sum_k |a_ik b_jk|); (bf16x6, fp32-MFMA)",
                   "worst": worst, "cases": ERR_LOG}, f, indent=1)


# ---- image GEMMs (csrc/gemm3.hip): shapes, ids and bodies are in tests/gemm_cases.py -----------
@pytest.mark.parametrize("m,n,k", G.NT_IMAGES_SHAPES)
@pytest.mark.parametrize("variant", list(G.NT_IMAGES_VARIANTS), ids=list(G.NT_IMAGES_VARIANTS.values()))
@pytest.mark.parametrize("acc", [0, 1])
def test_gemm_nt_images(device, m, n, k, variant, acc):
    G.check_gemm_nt_images(device, m, n, k, variant, acc)


def test_gemm_nt_images_six_products_kat(device):
    lib, check = _lib()
    m, n, k = 300, 200, 48
    a, b, want = _kat_operands(m, n, k)
    a3 = _image(lib, check, device, a.to(device), k)
    b3 = _image(lib, check, device, b.to(device), k)
    for variant in (1, 2, 3, 7, 11, 12, 21, 22):
        cd = th.zeros(m, n, device=device)
        check(lib.marl_gemm_nt_images(a3.data_ptr(), b3.data_ptr(), None, cd.data_ptr(), n, m, n, k, 0, variant, None))
        assert th.equal(cd.cpu().double(), want)


@pytest.mark.parametrize("m,n,nin", G.LSTM_IMAGES_SHAPES)
@pytest.mark.parametrize("variant", list(G.LSTM_IMAGES_VARIANTS), ids=list(G.LSTM_IMAGES_VARIANTS.values()))
def test_lstm_images(device, m, n, nin, variant):
    G.check_lstm_images(device, m, n, nin, variant)


@pytest.mark.parametrize("m,n,nin", [(512, 256, 624), (2048, 256, 624), (333, 100, 77), (4096, 256, 368)])
def test_lstm_gate_split_equals_the_one_wave_form(device, m, n, nin):
    """the small-batch plans (one gate per wave, 32- / 64-row tiles: BASELINE configs[3], [4] at 32 images per GPU)
    run the same K loop and the same cell arithmetic as the 128-row kernel: h', c', the activated gates and the
    image of h' are BIT-identical"""
    lib, check = _lib()
    g = th.Generator().manual_seed(3 * m + n + nin)
    u, h, cprev = th.randn(m, nin, generator=g), th.randn(m, n, generator=g), th.randn(m, n, generator=g)
    wih, whh = th.randn(4 * n, nin, generator=g) / nin ** 0.5, th.randn(4 * n, n, generator=g) / n ** 0.5
    bias = th.randn(4 * n, generator=g)
    img = lambda t, k: _image(lib, check, device, _padded(t.to(device), _p4(k)), k)  # noqa: E731
    u3, h3, wih3, whh3 = img(u, nin), img(h, n), img(wih, nin), img(whh, n)
    cpd, bd = _padded(cprev.to(device), _p4(n)), bias.to(device)
    res = {}
    for variant in (2, 3, 4, 5, 6):
        hn, cn = th.zeros(m, _p4(n), device=device), th.zeros(m, _p4(n), device=device)
        gt = th.zeros(m, _p4(4 * n), device=device)
        h3n = th.zeros(lib.marl_image_bytes(m, n) + 256, dtype=th.uint8, device=device)
        check(lib.marl_lstm_images(u3.data_ptr(), nin, h3.data_ptr(), wih3.data_ptr(), whh3.data_ptr(), bd.data_ptr(),
                                   cpd.data_ptr(), hn.data_ptr(), cn.data_ptr(), gt.data_ptr(), h3n.data_ptr(), m, n,
                                   _p4(n), _p4(4 * n), variant, 1, None))
        res[variant] = (hn, cn, gt, h3n[: lib.marl_image_bytes(m, n)])
    for variant in (3, 4, 5, 6):  # (5, 6: the phase-pipelined 256-row kernels of round 6)
        for a, b, name in zip(res[2], res[variant], ("h", "c", "gates", "image")):
            assert th.equal(a, b), (variant, name)


@pytest.mark.parametrize("rows,ni,nj", G.TN_IMAGES_SHAPES)
@pytest.mark.parametrize("variant", list(G.TN_IMAGES_VARIANTS), ids=list(G.TN_IMAGES_VARIANTS.values()))
def test_gemm_tn_images(device, rows, ni, nj, variant):
    G.check_gemm_tn_images(device, rows, ni, nj, variant)


@pytest.mark.parametrize("rows,ni,nih,nhh", G.CELL_IMAGES_SHAPES)
def test_gemm_tn_images_cell(device, rows, ni, nih, nhh):
    G.check_gemm_tn_images_cell(device, rows, ni, nih, nhh)


@pytest.mark.parametrize("m,n", [(95, 24), (4096, 384), (7, 1), (300, 1000)])
def test_ln_silu_fwd(device, m, n):
    lib, check = _lib()
    g = th.Generator().manual_seed(m + n)
    z = th.randn(m, n, generator=g) * 3
    gamma = th.randn(n, generator=g)
    beta = th.randn(n, generator=g)
    zd = _padded(z.to(device), _p4(n))
    out = th.zeros(m, _p4(n) + 4, device=device)
    stats = th.zeros(m, 2, device=device)
    gd, bd = gamma.to(device), beta.to(device)
    check(lib.marl_ln_silu_fwd(zd.data_ptr(), zd.shape[1], gd.data_ptr(), bd.data_ptr(),
                               out.data_ptr(), out.shape[1], stats.data_ptr(), m, n, None))
    th.cuda.synchronize()
    ref = F.silu(F.layer_norm(z, (n,), gamma, beta, 1e-5))
    assert th.allclose(out[:, :n].cpu(), ref, rtol=1e-5, atol=2e-6)
    assert th.equal(out[:, n:].cpu(), th.zeros(m, out.shape[1] - n))


def test_patch_gather_and_transition_kats(device):
    from marlclassification_amd.engine import HipEngine
    from tests.util import CASES, model_spec

    z = np.load(GOLDEN + "/g5_unit_kats.npz")
    eng = HipEngine(model_spec(CASES["g1_conftest"]), device)
    img, pos = th.from_numpy(z["crop_img"]), th.from_numpy(z["crop_pos"])
    obs = eng.patch_gather(img.to(device), pos.to(device), 5)
    assert th.equal(obs.cpu(), th.from_numpy(z["crop_obs"]))  # bit-exact copy, non-square image
    table = z["tr_table"].tolist()
    p0 = th.from_numpy(z["tr_pos"])
    acts = th.arange(len(table)).view(-1, 1)
    new = eng.transition(p0.to(device), acts.to(device), table, [10, 10], 5)
    assert th.equal(new.cpu(), th.from_numpy(z["tr_new"]))
