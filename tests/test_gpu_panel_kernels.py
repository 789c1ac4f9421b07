"""GPU: panel_fwd_kernel / panel_bwd_kernel (csrc/panel.hip) through their own entry points marl_panel_fwd /
marl_panel_bwd (include/marl_hip_panelops.h): one or two launches per case, at most a few hundred rows, against a plain
float64 torch-CPU reference - F.linear, F.layer_norm(eps = 1e-5), F.silu per layer, oracle.marl_oracle's
aggregate_messages for the message mean (for one agent too: zeros), M @ msgs for a mixing matrix, autograd for the
backward, and the LSTM cell of test_gpu_kernels.py::test_lstm_images differentiated by autograd.

Stage-wise: every stage the kernels write is compared with float64 applied to the kernel's OWN output of the stage
before it, so that errors do not compound and a failure names its stage (z_l <- a_{l-1}; stats_l, a_l <- z_l; xbar <-
a; dz_l, part_l <- the incoming gradient; dz_{l+1} <- dz_l W_l; dx <- dz_last W; the cells <- dx).  The gradient panel
between two layers lives in LDS only: its product and the next LayerNorm backward are one observed stage.

Every case first asserts its witness over marl_panel_plan (tests/panel_harness.py; tests/test_panel_plan_host.py checks
all of them without a GPU).  Bounds:
* GEMM stages, per element: |err| <= gamma_{K+1} (sum_k |a_k||w_k| + |b|), gamma_n = n 2^-24 / (1 - n 2^-24): holds for
  any summation order of a correct fp32 kernel, nothing measured.  The aggregation sites likewise (gamma_{na+2}).
* LayerNorm / SiLU and cell stages: MULT x max(E32, 2^-23 max|result|) with E32 the error of the plain fp32 torch-CPU
  evaluation of the same stage on the same inputs; the hard ceilings (1e-5 absolute for activations and statistics
  of O(1) rows, 1e-4 of the largest magnitude for every gradient) win where they are tighter.
* The exact checks (one-hot sweeps, slice known-answer rows, row independence, sentinels, images, determinism, NaN
  behind zero coefficients) have no tolerance.
With MARL_PANEL_KERNEL_ERRORS=<file> the achieved errors, E32 and ratios of every case are written there as JSON;
profiles/panel_kernel_errors.json is one such run and the source of LN_MULT / BWD_MULT / CELL_MULT below."""
import ctypes as C
import dataclasses
import json
import os

import pytest
import torch as th
import torch.nn.functional as F

from oracle.marl_oracle import aggregate_messages
from tests import panel_harness as H
from tests.panel_harness import SENT, gamma_n, r4
from tests.util import assert_witness

pytestmark = pytest.mark.gpu

# asserted multiples of max(E32, 2^-23 max|result|): twice the worst ratio of profiles/panel_kernel_errors.json
# ("worst_ratio"), rounded up (the convention of NT_BOUND in tests/test_gpu_kernels.py)
LN_MULT = 5    # forward: statistics and activations; worst ratio 2.38 (mean of k_tail_40-m1; activations at most 1.68)
BWD_MULT = 4   # backward: dz and dgamma | dbeta; worst ratio 1.92 (dz_2 of chain4_mix-na5; the affine sums at most 1.86)
CELL_MULT = 3  # cell gate gradients and dc; worst ratio 1.48 (the epilogue cell's gates without the LDS tail)
ABS_ACT = 1e-5    # activations of O(1) inputs
REL_GRAD = 1e-4   # ... and gradients, of the tensor's largest magnitude (tests/test_gpu_row_bwd.py)
_errors = {}


def _lib():
    from marlclassification_amd import _lib

    return _lib, _lib.load(), _lib.check


@pytest.fixture(scope="module", autouse=True)
def _error_record():
    yield
    path = os.environ.get("MARL_PANEL_KERNEL_ERRORS")
    if path and _errors:
        worst = {}
        for e in _errors.values():
            for k, v in e.items():
                kind = k.split(":")[0]
                worst[kind] = max(worst.get(kind, 0.0), v["ratio"])
        with open(path, "w") as f:
            json.dump({"unit": "err = max |gpu - float64|; e32 = max |fp32 torch-CPU - float64| of the same stage on the "
                               "same inputs; ratio = err / max(e32, 2^-23 max|float64|)",
                       "multiples": {"LN_MULT": LN_MULT, "BWD_MULT": BWD_MULT, "CELL_MULT": CELL_MULT},
                       "worst_ratio": worst, "cases": _errors}, f, indent=1, sort_keys=True)


def _stage(case, kind, stage, got, ref64, ref32, mult, ceiling):
    """one LayerNorm / cell stage: records err, e32 and their ratio, then asserts the multiple and the ceiling"""
    err = (got.double() - ref64).abs().max().item()
    mag = ref64.abs().max().item()
    e32 = (ref32.double() - ref64).abs().max().item()
    scale = max(e32, 2.0 ** -23 * mag)
    ratio = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
    _errors.setdefault(case, {})[f"{kind}:{stage}"] = {"err": err, "e32": e32, "max": mag, "ratio": ratio}
    print(f"{case} {kind}:{stage} err {err:.3e} e32 {e32:.3e} ratio {ratio:.2f}")
    # the project's own bounds: absolute for activations and means of O(1) rows, of the largest magnitude for gradients;
    # rstd is no activation - a row of one column has rstd = 1e-5^-1/2 = 316 - and is held to the same 1e-5 RELATIVE to
    # its size where that exceeds 1
    cap = {"act": ABS_ACT, "rstd": ABS_ACT * max(1.0, mag), "grad": REL_GRAD * mag}[ceiling]
    assert err <= cap + 1e-30, (case, stage, "above the project's bound", err, cap)
    if mult is not None:
        assert err <= mult * scale, (case, stage, err, e32, ratio)


def _gemm_stage(case, stage, got, a, w, bias=None):
    """|got - float64(a w^T + b)| <= gamma_{K+1} (|a| |w|^T + |b|), per element"""
    a64, w64 = a.double(), w.double()
    ref, mag = a64 @ w64.t(), a64.abs() @ w64.abs().t()
    if bias is not None:
        ref, mag = ref + bias.double(), mag + bias.double().abs()
    bound = gamma_n(a.shape[1] + 1) * mag
    over = (got.double() - ref).abs() - bound
    assert got.isfinite().all() and over.max().item() <= 0, (case, stage, over.max().item(), over.argmax().item())
    return ref


# ---- float64 / fp32 references ----------------------------------------------------------------------------------------
def _ln_silu(z, gamma, beta):
    return F.silu(F.layer_norm(z, (z.shape[1],), gamma.to(z.dtype), beta.to(z.dtype), 1e-5))


def _stats(z):
    mean = z.mean(dim=1)
    return mean, 1.0 / th.sqrt(((z - mean[:, None]) ** 2).mean(dim=1) + 1e-5)


def _aggregate(case, rows, mix, transpose=False):
    """rows [na * nb, k] -> the message mean over the other agents (the oracle's function) or the mixed messages"""
    t = rows.reshape(case.na, case.nb, -1)
    if mix is None:
        return aggregate_messages(t).reshape(rows.shape)
    mm = mix.to(rows.dtype)
    return th.einsum("ab,bnk->ank", mm.t() if transpose else mm, t).reshape(rows.shape)


def _agg_stage(case, stage, got, rows, mix, transpose=False):
    """aggregation sites: sums of at most na terms, one subtraction and one division - gamma_{na+2} of the magnitudes"""
    ref = _aggregate(case, rows.double(), mix, transpose)
    t = rows.double().abs().reshape(case.na, case.nb, -1)
    if mix is None:
        mag = ((t.sum(dim=0) + t) / max(case.na - 1, 1)).reshape(rows.shape)
    else:
        mm = mix.double().abs()
        mag = th.einsum("ab,bnk->ank", mm.t() if transpose else mm, t).reshape(rows.shape)
    over = (got.double() - ref).abs() - gamma_n(case.na + 2) * mag
    assert got.isfinite().all() and over.max().item() <= 0, (case.name, stage, over.max().item())


def _only_sentinel_outside(buf, m, n, what):
    b = buf.cpu()
    assert th.equal(b[m:], th.full_like(b[m:], SENT)), f"{what}: rows >= m were written"
    assert th.equal(b[:, n:], th.full_like(b[:, n:], SENT)), f"{what}: columns >= n were written"


# ---- forward ------------------------------------------------------------------------------------------------------------
def _image_of(device, t, k):
    mod, lib, check = _lib()
    img = th.zeros(lib.marl_image_bytes(t.shape[0], k) + 256, dtype=th.uint8, device=device)
    check(lib.marl_image_build(t.data_ptr(), t.shape[1], t.shape[0], k, img.data_ptr(), None))
    return img


def run_fwd(device, cases, inputs, prepare=None):
    """one marl_panel_fwd launch of these problems; returns their buffers"""
    mod, lib, check = _lib()
    bufs = [H.FwdBufs(c, i, device) for c, i in zip(cases, inputs)]
    if prepare:
        prepare(bufs)
    need = H.fwd_scratch_bytes(lib, cases)
    scratch = th.full((need // 4 + 64,), float("nan"), device=device)  # (the entry zeroes what it uses)
    descs = H.fwd_descs(bufs)
    check(lib.marl_panel_fwd(descs, len(bufs), scratch.data_ptr(), need, None))
    th.cuda.synchronize()
    assert scratch[need // 4:].isnan().all(), "scratch written behind its reported size"
    return bufs


def check_fwd(case, bufs, inp):
    m, name = case.m, case.name
    mix = inp.get("mix")
    prev = inp["x"]
    e2e = inp["x"].double()
    kin = case.k0
    for l, n in enumerate(case.widths):
        w, bias, gamma, beta = inp["w"][l], inp["bias"][l], inp["gamma"][l], inp["beta"][l]
        if (case.form == "staged" and l == 0) or (case.agg_at and l == case.agg_at):
            ld = bufs.xbar.shape[1]
            _only_sentinel_outside(bufs.xbar, m, r4(kin), f"xbar before layer {l}")
            xb = bufs.xbar[:m, :kin].cpu()
            assert th.equal(bufs.xbar[:m, kin:r4(kin)].cpu(), th.zeros(m, r4(kin) - kin)), "xbar: pad columns not zero"
            _agg_stage(case, f"xbar before layer {l}", xb, prev, mix)
            prev, e2e = xb, _aggregate(case, e2e, mix)
        a_gpu = bufs.a[l][:m, :n].cpu()
        _only_sentinel_outside(bufs.a[l], m, n, f"a_{l}")
        if case.save:
            z_gpu = bufs.z[l][:m, :n].cpu()
            _only_sentinel_outside(bufs.z[l], m, n, f"z_{l}")
            _only_sentinel_outside(bufs.stats[l], m, 2, f"stats_{l}")
            _gemm_stage(name, f"z_{l}", z_gpu, prev, w, bias)
            z64, z32 = z_gpu.double(), z_gpu
            st = bufs.stats[l][:m].cpu()
            (m64, r64), (m32, r32) = _stats(z64), _stats(z32)
            _stage(name, "ln", f"mean_{l}", st[:, 0], m64, m32, LN_MULT, "act")
            _stage(name, "ln", f"rstd_{l}", st[:, 1], r64, r32, LN_MULT, "rstd")
        else:  # z is not kept: product and LayerNorm are one observed stage
            z64 = prev.double() @ w.double().t() + bias.double()
            z32 = F.linear(prev, w, bias)
        _stage(name, "ln", f"a_{l}", a_gpu, _ln_silu(z64, gamma.double(), beta.double()), _ln_silu(z32, gamma, beta),
               LN_MULT, "act")
        e2e = _ln_silu(e2e @ w.double().t() + bias.double(), gamma.double(), beta.double())
        prev, kin = a_gpu, n
    err = (prev.double() - e2e).abs().max().item()
    _errors.setdefault(name, {})["e2e:a_last"] = {"err": err, "e32": 0.0, "max": e2e.abs().max().item(), "ratio": 0.0}
    assert err <= ABS_ACT, (name, "end to end", err)


@pytest.mark.parametrize("case", H.FWD_CASES, ids=lambda c: c.name)
def test_forward(device, case):
    assert_witness(H.fwd_plan([case]), case.witness)
    mod, lib, check = _lib()
    inp = H.fwd_inputs(case)
    a3_before = None

    def prepare(bufs):
        nonlocal a3_before
        if case.image:
            row0, col0, steps = case.image
            g = th.Generator().manual_seed(5)
            base = th.randn(case.m + row0 + 2, 16 * steps, generator=g).to(device)
            a3_before = base
            bufs[0].a3 = _image_of(device, base, 16 * steps)

    bufs = run_fwd(device, [case], [inp], prepare)[0]
    check_fwd(case, bufs, inp)
    if case.image:  # the image equals marl_image_build of the fp32 result placed into what was there, bit for bit
        row0, col0, steps = case.image
        n = case.widths[-1]
        a3_before[row0:row0 + case.m, col0:col0 + n] = bufs.a[-1][: case.m, :n]
        assert th.equal(bufs.a3.cpu(), _image_of(device, a3_before, 16 * steps).cpu())


def test_forward_two_problems_in_one_launch(device):
    cases = list(H.FWD_PAIR)
    assert_witness(H.fwd_plan(cases), H.FWD_PAIR_WITNESS)
    inputs = [H.fwd_inputs(c) for c in cases]
    both = run_fwd(device, cases, inputs)
    for c, b, i in zip(cases, both, inputs):
        check_fwd(c, b, i)
    # ... and each problem alone writes the same bits (the shared wave count changes no problem's K split here:
    # the plain problem alone has 12 waves too; the chain's layers keep ks == 1 at 4 and at 12 waves)
    for c, b, i in zip(cases, both, inputs):
        alone = run_fwd(device, [c], [i])[0]
        for l in range(len(c.widths)):
            assert th.equal(alone.a[l], b.a[l]) and th.equal(alone.z[l], b.z[l]) and th.equal(alone.stats[l], b.stats[l])


@pytest.mark.parametrize("tag", list(H.FWD_WIDTHS))
def test_forward_one_hot_k_sweep(device, tag):
    """m = K rows, row r = 2^(r % 5) e_r: z[r][j] is fl32(2^(r % 5) W[j][r] + b[j]) bit for bit for every (j, k) - the
    fragment addressing, the K tails, the slice boundaries and the tile tails through the arithmetic"""
    k, n, wit = H.FWD_WIDTHS[tag]
    case = H.Fwd(tag, k, (n,), k, pad=1)
    assert_witness(H.fwd_plan([case]), wit)
    inp = H.fwd_inputs(case)
    inp["x"] = H.one_hot_rows(k)
    bufs = run_fwd(device, [case], [inp])[0]
    want = inp["w"][0].t() * (2.0 ** (th.arange(k) % 5).float())[:, None] + inp["bias"][0]  # one rounding: the add
    assert th.equal(bufs.z[0][:k, :n].cpu(), want)
    _only_sentinel_outside(bufs.z[0], k, n, "z")


@pytest.mark.parametrize("tag", list(H.FWD_WIDTHS))
def test_forward_slice_known_answer(device, tag):
    """one 2^-s in each K slice s of a row, all weights 1, no bias: the sum is exact in fp32 in any order, so a lost,
    doubled or misplaced slice changes the bits (the operands' exactness: tests/test_panel_plan_host.py)"""
    k, n, wit = H.FWD_WIDTHS[tag]
    case = H.Fwd(tag, k, (n,), 16)
    p = H.fwd_plan([case])
    assert_witness(p, wit)
    inp = H.fwd_inputs(case)
    inp["x"], want = H.slice_kat(k, p["ks"][0], p["kper"][0])
    inp["w"][0] = th.ones(n, k)
    inp["bias"][0] = th.zeros(n)
    bufs = run_fwd(device, [case], [inp])[0]
    assert th.equal(bufs.z[0][:16, :n].cpu().double(), want[:, None].expand(16, n))


def _fwd_outputs(case, bufs):
    m = case.m
    out = []
    for l, n in enumerate(case.widths):
        out += [bufs.z[l][:m, :n].cpu(), bufs.stats[l][:m].cpu(), bufs.a[l][:m, :n].cpu()]
    return out


@pytest.mark.parametrize("tag", ["c3_encoder_in", "first_six_slot", "k_not_mult_4", "empty_slices_780"])
def test_forward_rows_are_independent(device, tag):
    """plain form: permuting the input rows permutes z, stats and a bit for bit; a row's result does not depend on the
    other rows of its panel; two runs are equal"""
    k, n, _ = H.FWD_WIDTHS[tag]
    case = H.Fwd(tag, k, (n, 48), 53)
    inp = H.fwd_inputs(case)
    base = _fwd_outputs(case, run_fwd(device, [case], [inp])[0])
    again = _fwd_outputs(case, run_fwd(device, [case], [inp])[0])
    assert all(th.equal(a, b) for a, b in zip(base, again)), "two runs differ"
    perm = th.randperm(case.m, generator=th.Generator().manual_seed(3))
    moved = dict(inp, x=inp["x"][perm])
    got = _fwd_outputs(case, run_fwd(device, [case], [moved])[0])
    assert all(th.equal(g, b[perm]) for g, b in zip(got, base))
    keep = th.arange(case.m) % 5 == 2  # these rows stay, every other row of their panels changes
    other = dict(inp, x=th.where(keep[:, None], inp["x"], 3.0 * inp["x"].flip(0) + 1.0))
    got = _fwd_outputs(case, run_fwd(device, [case], [other])[0])
    assert all(th.equal(g[keep], b[keep]) for g, b in zip(got, base))
    assert not th.equal(got[0], base[0])


@pytest.mark.parametrize("na", H.AGENTS)
@pytest.mark.parametrize("mix", [False, True], ids=["mean", "mix"])
def test_forward_chain_images_are_independent(device, na, mix):
    """chained form: permuting whole images permutes every output bit for bit (the images of a workgroup and the
    padding rows do not leak into each other)"""
    nb = H.NB_OF[na]
    case = H.Fwd("chain", 40, (64, 32, 64, 48), na * nb, "chain", na, nb, agg_at=2, mix=mix)
    inp = H.fwd_inputs(case)
    b0 = run_fwd(device, [case], [inp])[0]
    base = _fwd_outputs(case, b0) + [b0.xbar[: case.m, :32].cpu()]
    b2 = run_fwd(device, [case], [inp])[0]
    again = _fwd_outputs(case, b2) + [b2.xbar[: case.m, :32].cpu()]
    assert all(th.equal(a, b) for a, b in zip(base, again)), "two runs differ"
    perm = th.randperm(nb, generator=th.Generator().manual_seed(4))
    rows = (th.arange(na)[:, None] * nb + perm[None, :]).reshape(-1)
    b1 = run_fwd(device, [case], [dict(inp, x=inp["x"][rows])])[0]
    got = _fwd_outputs(case, b1) + [b1.xbar[: case.m, :32].cpu()]
    assert all(th.equal(g, b[rows]) for g, b in zip(got, base))


def test_forward_zero_coefficient_senders_may_hold_nan(device):
    """under a mixing matrix a sender whose coefficient is exactly 0 is not read: the last agent reaches only itself
    (tests/panel_harness.py::mixing_matrix), so NaN in ITS input rows stays in its own rows"""
    na, nb = 5, 7
    case = H.Fwd("chain_nan", 40, (64, 32, 64, 48), na * nb, "chain", na, nb, agg_at=2, mix=True)
    inp = H.fwd_inputs(case)
    assert (inp["mix"][: na - 1, na - 1] == 0).all() and inp["mix"][na - 1, na - 1] != 0
    base = run_fwd(device, [case], [inp])[0]
    x = inp["x"].clone()
    x[(na - 1) * nb:] = float("nan")
    got = run_fwd(device, [case], [dict(inp, x=x)])[0]
    ok = (na - 1) * nb
    for l in range(4):
        assert th.equal(got.a[l][:ok], base.a[l][:ok]), f"layer {l}: NaN leaked through a zero coefficient"
    assert got.a[3][ok: case.m, :48].isnan().all()


# ---- backward -----------------------------------------------------------------------------------------------------------
def _cell_autograd(t, dh):
    """float64: the cell of test_gpu_kernels.py::test_lstm_images (c' = f c + i g, h' = o tanh(c'), i, f, o sigmoids
    and g a tanh of the pre-activations) differentiated by autograd at the saved activations - the gradients w.r.t. the
    four pre-activations and w.r.t. c.  The saved c' is used where the kernel uses it (c' + (c - c.detach()) carries
    the graph without changing the value)."""
    n = t["c_prev"].shape[1]
    gi, gf, gg, go = (x.double() for x in t["gates"].split(n, dim=1))
    pre = [p.detach().requires_grad_() for p in (th.logit(gi), th.logit(gf), th.atanh(gg), th.logit(go))]
    cp = t["c_prev"].double().requires_grad_()
    i_, f_, g_, o_ = th.sigmoid(pre[0]), th.sigmoid(pre[1]), th.tanh(pre[2]), th.sigmoid(pre[3])
    c = f_ * cp + i_ * g_
    c = t["c_new"].double() + (c - c.detach())
    h = o_ * th.tanh(c)
    ((h * dh.double()).sum() + (c * t["dc"].double()).sum()).backward()
    return th.cat([p.grad for p in pre], dim=1), cp.grad


def _cell_plain(t, dh, dtype):
    """the same derivatives written out (what a plain evaluation in `dtype` computes: E32 for dtype = float32)"""
    n = t["c_prev"].shape[1]
    gi, gf, gg, go = (x.to(dtype) for x in t["gates"].split(n, dim=1))
    tc = th.tanh(t["c_new"].to(dtype))
    dh = dh.to(dtype)
    d = dh * go * (1 - tc * tc) + t["dc"].to(dtype)
    return th.cat([d * gg * gi * (1 - gi), d * t["c_prev"].to(dtype) * gf * (1 - gf), d * gi * (1 - gg * gg),
                   dh * tc * go * (1 - go)], dim=1), d * gf


def _check_cell(case, tag, cb, t, dh, img_done, device):
    c, rows, n = cb.c, cb.rows, cb.c.n
    g64, dc64 = _cell_autograd(t, dh)
    p64 = _cell_plain(t, dh, th.float64)  # (autograd and the written-out derivatives agree to float64 rounding)
    assert (p64[0] - g64).abs().max().item() <= 1e-12 * max(1.0, g64.abs().max().item())
    assert (p64[1] - dc64).abs().max().item() <= 1e-12 * max(1.0, dc64.abs().max().item())
    g32, dc32 = _cell_plain(t, dh, th.float32)
    dc = cb.dc[:rows, :n].cpu()
    _stage(case.name, "cell", f"{tag}_dc", dc, dc64, dc32, CELL_MULT, "grad")
    _only_sentinel_outside(cb.dc, rows, n, f"{tag} dc")
    skipped = bool(c.skip and img_done)
    gates = cb.gates[:rows, : 4 * n].cpu()
    if skipped:  # the fp32 gate gradients keep what was there exactly when the image is reported written
        assert th.equal(gates, t["gates"]), f"{tag}: skip_f32 with the image written, yet the fp32 gates changed"
    else:
        _stage(case.name, "cell", f"{tag}_gates", gates, g64, g32, CELL_MULT, "grad")
    _only_sentinel_outside(cb.gates, rows, 4 * n, f"{tag} gates")
    if c.g3 and not img_done:
        assert th.equal(cb.g3, cb.g3_before), f"{tag}: image reported as not written, yet bytes changed"
    elif c.g3 and not skipped:
        # marl_image_build of the fp32 gradients placed into what the image held (rows from row0, columns < 4 n), bit for bit
        cb.g3_base[cb.row0: cb.row0 + rows, : 4 * n] = cb.gates[:rows, : 4 * n]
        assert th.equal(cb.g3, _image_of(device, cb.g3_base, 16 * cb.steps)), f"{tag}: image differs from marl_image_build"
    # (skipped: no fp32 copy to build from - test_backward compares the image with the twin case that keeps it)


def run_bwd(device, case, inp):
    mod, lib, check = _lib()
    bufs = H.BwdBufs(case, inp, device, lib)
    for cb in (bufs.cell, bufs.cellb):
        if cb is not None and cb.g3 is not None:  # the image starts as the image of other values, not as zeros
            g = th.Generator().manual_seed(11)
            cb.g3_base = th.randn(cb.rows + cb.row0 + 2, 16 * cb.steps, generator=g).to(device)
            cb.g3_before = _image_of(device, cb.g3_base, 16 * cb.steps)
            assert cb.g3_before.shape == cb.g3.shape
            cb.g3.copy_(cb.g3_before)
    need = H.bwd_scratch_bytes(lib, case)
    scratch = th.full((need // 4 + 64,), float("nan"), device=device)
    d = bufs.desc()
    check(lib.marl_panel_bwd(C.byref(d), scratch.data_ptr(), need, None))
    th.cuda.synchronize()
    assert scratch[need // 4:].isnan().all(), "scratch written behind its reported size"
    return bufs, d


def _ln_bwd(z, gamma, beta, g_in):
    z = z.detach().clone().requires_grad_()
    gamma = gamma.detach().clone().to(z.dtype).requires_grad_()
    beta = beta.detach().clone().to(z.dtype).requires_grad_()
    _ln_silu(z, gamma, beta).backward(g_in.to(z.dtype))
    return z.grad, th.cat([gamma.grad, beta.grad])


def check_bwd(case, bufs, d, inp, device):
    m, name = case.m, case.name
    mix = inp.get("mix")
    # the gradient entering the first listed layer
    g64 = inp["da"].double() + (inp["da2"].double() if case.da2 else 0)
    g32 = inp["da"] + (inp["da2"] if case.da2 else 0)
    if case.form == "staged":
        g64, g32 = _aggregate(case, g64, None), _aggregate(case, g32, None)
    e2e = g64
    for l, (n, k) in enumerate(case.layers):
        z, gamma, beta, w = inp["z"][l], inp["gamma"][l], inp["beta"][l], inp["w"][l]
        if l > 0 and l == case.agg_at:
            g64, g32, e2e = (_aggregate(case, t, mix, True) for t in (g64, g32, e2e))
        dz64, aff64 = _ln_bwd(z.double(), gamma, beta, g64)
        dz32, aff32 = _ln_bwd(z, gamma, beta, g32)
        dz = bufs.dz[l][:m, :n].cpu()
        _stage(name, "bwd", f"dz_{l}", dz, dz64, dz32, BWD_MULT, "grad")
        _only_sentinel_outside(bufs.dz[l], m, n, f"dz_{l}")
        part = bufs.part[l].cpu()
        assert th.equal(part[bufs.blocks:], th.full_like(part[bufs.blocks:], SENT)), f"part_{l}: written past the workgroups"
        _stage(name, "bwd", f"dgamma_dbeta_{l}", part[: bufs.blocks].double().sum(dim=0).float(), aff64, aff32,
               BWD_MULT, "grad")
        e2e = _ln_bwd(z.double(), gamma, beta, e2e)[0] @ w.double()
        g64, g32 = dz.double() @ w.double(), dz @ w  # the next panel, from the kernel's own dz
        last_dz, last_w = dz, w
    k = case.layers[-1][1]
    dx = bufs.dx[:m, :k].cpu()
    pre = inp["dx0"] if case.accumulate else th.zeros(m, k)
    assert dx.isfinite().all(), "dx: a NaN prefill survived (accumulate == 0) or the kernel wrote one"
    _only_sentinel_outside(bufs.dx, m, k, "dx")
    # dx = prefill + dz_last W: the product per element within gamma_{n+1}, the sum one more rounding
    ref = last_dz.double() @ last_w.double()
    mag = last_dz.double().abs() @ last_w.double().abs()
    over = (dx.double() - (ref + pre.double())).abs() - (gamma_n(last_dz.shape[1] + 1) * mag + 2.0 ** -24 * (ref + pre.double()).abs())
    assert over.max().item() <= 0, (name, "dx", over.max().item())
    e2e = e2e + pre.double()
    err, mag = (dx.double() - e2e).abs().max().item(), e2e.abs().max().item()
    _errors.setdefault(name, {})["e2e:dx"] = {"err": err, "e32": 0.0, "max": mag, "ratio": 0.0}
    assert err <= REL_GRAD * mag, (name, "end to end dx", err, mag)
    if case.cellb:
        assert d.cellb_img_done == H.bwd_plan(case)["cellb_img_done"]
        _check_cell(case, "cellb", bufs.cellb, inp["cellb"], dx, d.cellb_img_done, device)
    if case.cell:
        assert d.cell_img_done == H.bwd_plan(case)["cell_img_done"]
        _check_cell(case, "cell", bufs.cell, inp["cell"], inp["cell"]["dh"], d.cell_img_done, device)


@pytest.mark.parametrize("case", H.BWD_CASES, ids=lambda c: c.name)
def test_backward(device, case):
    assert_witness(H.bwd_plan(case), case.witness)
    inp = H.bwd_inputs(case)
    bufs, d = run_bwd(device, case, inp)
    check_bwd(case, bufs, d, inp, device)
    for which in ("cell", "cellb"):
        c = getattr(case, which)
        if c and c.skip and getattr(d, f"{which}_img_done"):
            # skip_f32 changes what is stored, not what is computed: the image and dc equal those of the twin case
            # that keeps the fp32 gradients (whose image is checked against marl_image_build of them)
            twin = dataclasses.replace(case, **{which: dataclasses.replace(c, skip=0)})
            tb, td = run_bwd(device, twin, inp)
            assert getattr(td, f"{which}_img_done") == 1
            assert th.equal(getattr(tb, which).g3, getattr(bufs, which).g3), f"{which}: skip_f32 changed the image"
            assert th.equal(getattr(tb, which).dc, getattr(bufs, which).dc), f"{which}: skip_f32 changed dc"


@pytest.mark.parametrize("tag", list(H.BWD_WIDTHS))
@pytest.mark.parametrize("shift", [0, 1, 17])
def test_backward_dx_through_one_hot_weights(device, tag, shift):
    """The kernel offers no way to feed dz, and a LayerNorm backward cannot produce a one-hot row (its rows sum to 0
    against gamma), so the one-hot half of the K sweep is carried by the WEIGHT: W[j][k] = 2^(k % 5) where
    j == (k + shift) % n, else 0.  Then dx[r][k] is dz_gpu[r][(k + shift) % n] 2^(k % 5) bit for bit (every other term
    is an exact zero): the transposed fragment copy, the tile rounds and the K slices of the dX product through the
    arithmetic, for every output column k."""
    n, k, wit = H.BWD_WIDTHS[tag]
    case = H.Bwd(tag, ((n, k),), 37, pad=1)
    assert_witness(H.bwd_plan(case), wit)
    inp = H.bwd_inputs(case)
    cols = th.arange(k)
    w = th.zeros(n, k)
    w[(cols + shift) % n, cols] = 2.0 ** (cols % 5).float()
    inp["w"][0] = w
    bufs, _ = run_bwd(device, case, inp)
    dz = bufs.dz[0][:37, :n].cpu()
    assert th.equal(bufs.dx[:37, :k].cpu(), dz[:, (cols + shift) % n] * 2.0 ** (cols % 5).float())


@pytest.mark.parametrize("tag", ["two_slots", "widest_row", "tail_off_by_alignment", "tile_rounds"])
def test_backward_rows_are_independent(device, tag):
    n, k, _ = H.BWD_WIDTHS[tag]
    case = H.Bwd(tag, ((n, k), (k, 40)), 53, da2=1)
    if k > 384:
        case = H.Bwd(tag, ((64, n), (n, k)), 53, da2=1)
    inp = H.bwd_inputs(case)

    def outputs(i):
        b, _ = run_bwd(device, case, i)
        return [b.dz[l][:53, :nn].cpu() for l, (nn, _) in enumerate(case.layers)] + [b.dx[:53, : case.layers[-1][1]].cpu()]

    def rows(i, fn):
        out = dict(i)
        for key in ("da", "da2"):
            out[key] = fn(i[key])
        out["z"] = [fn(z) for z in i["z"]]
        return out

    base, again = outputs(inp), outputs(inp)
    assert all(th.equal(a, b) for a, b in zip(base, again)), "two runs differ"
    perm = th.randperm(53, generator=th.Generator().manual_seed(3))
    got = outputs(rows(inp, lambda t: t[perm]))
    assert all(th.equal(g, b[perm]) for g, b in zip(got, base))
    keep = th.arange(53) % 5 == 2
    got = outputs(rows(inp, lambda t: th.where(keep[:, None], t, 2.0 * t.flip(0) - 0.5)))
    assert all(th.equal(g[keep], b[keep]) for g, b in zip(got, base))
    assert not th.equal(got[0], base[0])


@pytest.mark.parametrize("na", H.AGENTS)
@pytest.mark.parametrize("mix", [False, True], ids=["mean", "mix"])
def test_backward_chain_images_are_independent(device, na, mix):
    nb = H.NB_OF[na]
    case = H.Bwd("chain", ((48, 64), (64, 32), (32, 64), (64, 40)), na * nb, "chain", na, nb, agg_at=2, mix=mix)
    inp = H.bwd_inputs(case)
    perm = th.randperm(nb, generator=th.Generator().manual_seed(4))
    rows = (th.arange(na)[:, None] * nb + perm[None, :]).reshape(-1)
    moved = dict(inp, da=inp["da"][rows], z=[z[rows] for z in inp["z"]])
    b0, _ = run_bwd(device, case, inp)
    b1, _ = run_bwd(device, case, moved)
    b2, _ = run_bwd(device, case, inp)
    m = case.m
    for l, (n, _) in enumerate(case.layers):
        assert th.equal(b2.dz[l], b0.dz[l]) and th.equal(b2.part[l], b0.part[l]), f"two runs differ in layer {l}"
        assert th.equal(b1.dz[l][:m, :n].cpu(), b0.dz[l][:m, :n].cpu()[rows]), f"dz_{l}"
    assert th.equal(b1.dx[:m, :40].cpu(), b0.dx[:m, :40].cpu()[rows])


def test_fast_tanh_of_the_cell_backward_for_small_c(device):
    """the cell backward takes tanh(c') from a fast form, 1 - 2 / (1 + exp(2 c')), which cancels for small |c'|: its
    ABSOLUTE error for c' in [-1e-3, 1e-3] must stay inside the gradient bound of the tensor it feeds - 1e-4 of the
    largest magnitude, here of tanh over rows that also hold c' up to 3.  The o gate's gradient is dh tanh(c') o (1 - o):
    with dh = 1 and o = 1/2 the kernel's output is tanh_fast(c') / 4 exactly, so the kernel's tanh is read off it"""
    n, rows = 64, 256
    case = H.Bwd("tanh", ((64, 32),), 16, cell=H.Cell(n, rows=rows))
    assert_witness(H.bwd_plan(case), ("cell_vec4 == 1",))
    inp = H.bwd_inputs(case)
    t = inp["cell"]
    small = th.linspace(-1e-3, 1e-3, rows * n // 2).reshape(rows // 2, n)
    t["c_new"] = th.cat([small, th.linspace(-3, 3, rows * n // 2).reshape(rows // 2, n)]).contiguous()
    t["gates"] = th.full((rows, 4 * n), 0.5)
    t["dh"] = th.ones(rows, n)
    t["dc"] = th.zeros(rows, n)
    bufs, _ = run_bwd(device, case, inp)
    tanh_gpu = 4.0 * bufs.cell.gates[:rows, 3 * n: 4 * n].cpu().double()
    ref = th.tanh(t["c_new"].double())
    err_small = (tanh_gpu - ref)[: rows // 2].abs().max().item()
    err_all = (tanh_gpu - ref).abs().max().item()
    _errors.setdefault("fast_tanh", {})["tanh:small_c"] = {"err": err_small, "e32": 0.0, "max": 1e-3, "ratio": 0.0}
    _errors["fast_tanh"]["tanh:all_c"] = {"err": err_all, "e32": 0.0, "max": ref.abs().max().item(), "ratio": 0.0}
    print("fast tanh: max abs error", err_small, "for |c| <= 1e-3,", err_all, "for |c| <= 3")
    assert err_small <= REL_GRAD * ref.abs().max().item() and err_all <= REL_GRAD * ref.abs().max().item()
