"""GPU: the conv backward kernels of csrc/cnn.hip through their own entry points - cnn_wgrad_kernel's first-layer and
fp32 forms through marl_cnn_wgrad, cnn_dgrad_kernel through marl_cnn_dgrad (include/marl_hip_cnnops.h) - against
float64 torch-CPU autograd of conv2d(silu(group_norm(x)), w, stride 2, pad 1) (conv2d(patch, w, ...) for the first
layer).

Every case first asserts its witness from marl_cnn_bwd_plan (what the launcher chooses, from the launcher's own
routines), so a change of a plan rule fails here instead of turning a case into a copy of another; the tables below are
also what tests/test_conv_plan_host.py checks the selectable instantiations against.  Inputs sit inside larger buffers
whose surroundings are NaN (255 for uint8 images), outputs inside buffers pre-filled with a sentinel that must survive
outside the tensor and be gone inside; every call runs twice and must repeat bit for bit; knobs are restored.  The
GroupNorm statistics handed to the kernels are float64, rounded once.

Bounds, relative to the reference tensor's largest magnitude: 2e-6 for dW / db (what the bf16x6 test holds both weight
gradient forms to), 1e-4 for the layer backward's outputs.  On top, the kernel's error must not
exceed max(MULT * e32, floor) where e32 is the error of the same computation by torch on the CPU in float32 on the same
data; floor = 2e-6 for the weight gradient and, for the layer backward, the worst e32 of the whole grid for that output
(dzin, dgamma, dbeta each have their own summation length).  MULT = 4: the kernels sum in another order (tiles of four
along K, per-workgroup slabs) and use the hardware exp / rcp.  With MARL_CONV_BWD_ERRORS=<file> in the environment the
achieved errors, e32 and ratios of every case are written there as JSON (profiles/conv_bwd_errors.json is one such
run)."""
import json
import os

import pytest
import torch as th
import torch.nn.functional as F

from tests.conv_cases import DG_SHAPES, SENTINEL, WG_DEEP, WG_FIRST, _embed, _Out, _rel, assert_wgrad_witness
from tests.conv_cases import bwd_plan as plan

pytestmark = pytest.mark.gpu

WG_BOUND = 2e-6
DG_BOUND = 1e-4
MULT = 4
_errors = {}

DG_KNOBS = [512, 1]  # dgrad_min_chunks: the default (rb = 1 at these row counts), and 1 (the largest rb that fits)
DG_ROWS = ["1", "rb+1", "3rb+2"]
# persistent + ragged: rows -> (dgrad_wgs, witness); 551 chunks of two patches, the last one of one - on what is
# resident (dgrad_wgs = 0), and on 48 workgroups, where every workgroup walks 11 or 12 chunks
DG_PERSISTENT = {"resident": (0, dict(rb=2, chunks=551)), "wgs48": (48, dict(rb=2, chunks=551))}
DG_PERSISTENT_ROWS = 1101


def _lib():
    from marlclassification_amd import _lib

    return _lib.load(), _lib.check


@pytest.fixture(scope="module", autouse=True)
def _error_record():
    yield
    path = os.environ.get("MARL_CONV_BWD_ERRORS")
    if path and _errors:
        worst = {}
        for name, e in _errors.items():
            fam = name.split(" ")[0]
            for k, v in e.items():
                if k.startswith("ratio_"):
                    worst[fam] = max(worst.get(fam, 0.0), v)
        with open(path, "w") as f:
            json.dump({"wgrad_bound_rel_to_max": WG_BOUND, "dgrad_bound_rel_to_max": DG_BOUND, "multiple_of_e32": MULT,
                       "worst_ratio_err_over_max_of_e32_and_floor": worst, "cases": _errors}, f, indent=1,
                      sort_keys=True)


def _twice(run, outs):
    """runs `run` twice on freshly sentinel-filled outputs; the results must be bit-identical"""
    res = []
    for _ in range(2):
        for o in outs:
            o.reset()
        run()
        th.cuda.synchronize()
        res.append([o.get() for o in outs])
    for a, b in zip(*res):
        assert th.equal(a, b), "two runs differ"
    return res[0]


# ---- weight gradient -------------------------------------------------------------------------------------------
def _conv_wgrad(x, dz_nchw, cout, cin):
    """dW [co][tap * cin + ci] of conv2d(x, w, stride 2, pad 1) under the upstream gradient dz, in x's precision"""
    w = th.zeros(cout, cin, 3, 3, dtype=x.dtype, requires_grad=True)
    (F.conv2d(x, w, stride=2, padding=1) * dz_nchw).sum().backward()
    return w.grad.permute(0, 2, 3, 1).reshape(cout, 9 * cin)


def _check_wgrad(name, dw, db, ref, ref_b, dw32, db32):
    e = {"dw": _rel(dw, ref), "db": _rel(db, ref_b), "e32_dw": _rel(dw32, ref), "e32_db": _rel(db32, ref_b)}
    e["ratio_dw"] = e["dw"] / max(MULT * e["e32_dw"], WG_BOUND) * MULT
    e["ratio_db"] = e["db"] / max(MULT * e["e32_db"], WG_BOUND) * MULT
    _errors[name] = e
    print(name, e)
    assert e["dw"] <= WG_BOUND and e["db"] <= WG_BOUND, e
    assert e["dw"] <= max(MULT * e["e32_dw"], WG_BOUND) and e["db"] <= max(MULT * e["e32_db"], WG_BOUND), e


@pytest.mark.parametrize("u8", [0, 1], ids=["fp32", "uint8"])
@pytest.mark.parametrize("case", list(WG_FIRST))
def test_first_layer_weight_gradient(device, case, u8):
    lib, check = _lib()
    cin, cout, f, c_img, rows, nb, H, W, witness = WG_FIRST[case]
    p = plan(rows, cin, cout, f, 1, 1)
    assert_wgrad_witness(p, witness)
    assert rows == 1 or p["wg_rb"] == 1 or rows % p["wg_rb"] != 0  # a ragged last chunk wherever a chunk has > 1 patch
    if "blocks" in witness:
        assert p["wg_chunks"] > p["wg_blocks"]  # persistent workgroups
    assert H != W and nb in (3, 5)
    hout = (f - 1) // 2 + 1
    gen = th.Generator().manual_seed(17 * rows + 3 * f + cout + u8)
    dz = th.randn(rows, hout * hout, cout, generator=gen)
    if u8:
        img = th.randint(0, 256, (nb, c_img, H, W), generator=gen, dtype=th.uint8)
        img64 = img.double() / 255
        img32 = img.float() / 255
    else:
        img = th.rand(nb, c_img, H, W, generator=gen)
        img[:, cin:] = float("nan")  # (only the first cin channels are read)
        img64, img32 = img.double(), img
    # both ends of the environment's range (randint(size - f): 0 .. size - f - 1) in each dimension
    pos = th.stack([th.randint(0, H - f, (rows,), generator=gen), th.randint(0, W - f, (rows,), generator=gen)], 1)
    ends = th.tensor([[H - f - 1, W - f - 1], [0, 0], [0, W - f - 1], [H - f - 1, 0]])
    pos[:min(rows, 4)] = ends[:min(rows, 4)]
    pos = pos.to(th.int32)
    if rows >= 2:
        assert {0, H - f - 1} <= set(pos[:, 0].tolist()) and {0, W - f - 1} <= set(pos[:, 1].tolist())

    def patches(src):
        return th.stack([src[r % nb, :cin, pos[r, 0]:pos[r, 0] + f, pos[r, 1]:pos[r, 1] + f] for r in range(rows)])

    dzn = dz.view(rows, hout, hout, cout).permute(0, 3, 1, 2)
    ref = _conv_wgrad(patches(img64), dzn.double(), cout, cin)
    ref_b = dz.double().sum(dim=(0, 1))
    dw32, db32 = _conv_wgrad(patches(img32), dzn, cout, cin), dz.sum(dim=(0, 1))

    (_, dzd), (_, imgd), (_, posd) = _embed(dz, device), _embed(img, device), _embed(pos, device)
    sb = lib.marl_cnn_wgrad_scratch(rows, cin, cout, f, 1, 1)
    scratch = th.zeros(sb // 4 + 64, device=device)
    dw, db = _Out((cout, 9 * cin), device), _Out((cout,), device)

    def run():
        check(lib.marl_cnn_wgrad(dzd.data_ptr(), imgd.data_ptr(), u8, posd.data_ptr(), None, None, None, None, rows,
                                 nb, c_img, H, W, cin, cout, f, 1, dw.ptr(), db.ptr(), scratch.data_ptr(),
                                 scratch.numel() * 4, None))

    gw, gb = _twice(run, [dw, db])
    _check_wgrad(f"wgrad_first {case} {'uint8' if u8 else 'fp32'}", gw, gb, ref, ref_b, dw32, db32)


def _layer_data(rows, cin, cout, hin, G, seed):
    """dz, zin (NHWC), the float64 statistics rounded once, the affine, and a weight"""
    gen = th.Generator().manual_seed(seed)
    hout = (hin - 1) // 2 + 1
    dz = th.randn(rows, hout * hout, cout, generator=gen)
    zin = th.randn(rows, hin * hin, cin, generator=gen) * 1.5 + 0.3
    gamma = 1 + 0.1 * th.randn(cin, generator=gen)
    beta = 0.1 * th.randn(cin, generator=gen)
    w = th.randn(cout, cin, 3, 3, generator=gen) * (2.0 / (9 * cin)) ** 0.5
    zz = zin.view(rows, hin * hin, G, cin // G).double()
    gst = th.stack([zz.mean(dim=(1, 3)), 1.0 / th.sqrt(zz.var(dim=(1, 3), unbiased=False) + 1e-5)], -1).float()
    return dz, zin, gst.contiguous(), gamma, beta, w


def _nchw(t, rows, h, c):
    return t.view(rows, h, h, c).permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", list(WG_DEEP))
def test_deep_layer_weight_gradient_fp32_form(device, case):
    lib, check = _lib()
    cin, cout, hin, G, rows, witness = WG_DEEP[case]
    p = plan(rows, cin, cout, hin, G, 0)
    assert_wgrad_witness(p, witness)
    assert rows % p["wg_rb"] != 0
    if "blocks" in witness:
        assert p["wg_chunks"] > p["wg_blocks"]
    hout = (hin - 1) // 2 + 1
    dz, zin, gst, gamma, beta, _ = _layer_data(rows, cin, cout, hin, G, 131 * cin + cout + 7 * hin + rows)
    dzn = _nchw(dz, rows, hout, cout)

    def grads(dt):
        x = F.silu(F.group_norm(_nchw(zin, rows, hin, cin).to(dt), G, gamma.to(dt), beta.to(dt), 1e-5))
        return _conv_wgrad(x, dzn.to(dt), cout, cin), dz.to(dt).sum(dim=(0, 1))

    (ref, ref_b), (dw32, db32) = grads(th.float64), grads(th.float32)
    emb = [_embed(t, device) for t in (dz, zin, gst, gamma, beta)]
    dzd, zind, gstd, gd, bd = (v for _, v in emb)
    sb = lib.marl_cnn_wgrad_scratch(rows, cin, cout, hin, G, 0)
    scratch = th.zeros(sb // 4 + 64, device=device)
    dw, db = _Out((cout, 9 * cin), device), _Out((cout,), device)

    def run():
        check(lib.marl_cnn_wgrad(dzd.data_ptr(), None, 0, None, zind.data_ptr(), gstd.data_ptr(), gd.data_ptr(),
                                 bd.data_ptr(), rows, 1, 3, 64, 64, cin, cout, hin, G, dw.ptr(), db.ptr(),
                                 scratch.data_ptr(), scratch.numel() * 4, None))

    gw, gb = _twice(run, [dw, db])
    _check_wgrad(f"wgrad_deep {case}", gw, gb, ref, ref_b, dw32, db32)


# ---- layer backward ----------------------------------------------------------------------------------------------
def _dgrad_cases():
    """(name, shape, dgrad_min_chunks, dgrad_wgs, rows label)"""
    out = [(f"{s} mc={k} rows={r}", s, k, 0, r) for s in DG_SHAPES for k in DG_KNOBS for r in DG_ROWS]
    out += [(f"mnist_odd_side persistent {tag}", "mnist_odd_side", 512, wgs, str(DG_PERSISTENT_ROWS))
            for tag, (wgs, _) in DG_PERSISTENT.items()]
    return out


def _dgrad_rows(shape, knob, label):
    """the row count of a case: `rb` is what the launcher takes under the knob once the rows allow it"""
    cin, cout, G, hin, _ = DG_SHAPES[shape]
    rb = 1 if knob == 512 else plan(1000, cin, cout, hin, G, 0)["dg_rb"]
    return {"1": 1, "rb+1": rb + 1, "3rb+2": 3 * rb + 2}.get(label) or int(label)


def _dgrad_reference(shape, rows):
    cin, cout, G, hin, _ = DG_SHAPES[shape]
    hout = (hin - 1) // 2 + 1
    data = _layer_data(rows, cin, cout, hin, G, 977 * cin + 31 * hin + rows)
    dz, zin, gst, gamma, beta, w = data

    def grads(dt):
        x = _nchw(zin, rows, hin, cin).to(dt).requires_grad_()
        g, b = gamma.to(dt).requires_grad_(), beta.to(dt).requires_grad_()
        y = F.conv2d(F.silu(F.group_norm(x, G, g, b, 1e-5)), w.to(dt), stride=2, padding=1)
        y.backward(_nchw(dz, rows, hout, cout).to(dt))
        return {"dzin": x.grad.permute(0, 2, 3, 1).reshape(rows, hin * hin, cin), "dgamma": g.grad, "dbeta": b.grad}

    r64, r32 = grads(th.float64), grads(th.float32)
    return data, r64, {k: _rel(r32[k], r64[k]) for k in r64}


@pytest.fixture(scope="module")
def dgrad_refs():
    """float64 and float32 references of the whole grid, computed once: {(shape, rows): (data, ref64, e32)}, and the
    worst e32 per output over the grid (the floor of the second assertion)"""
    lib, check = _lib()
    refs = {}
    try:
        for _, shape, knob, _, label in _dgrad_cases():
            check(lib.marl_tune(b"dgrad_min_chunks", knob))
            key = (shape, _dgrad_rows(shape, knob, label))
            if key not in refs:
                refs[key] = _dgrad_reference(*key)
    finally:
        check(lib.marl_tune(b"dgrad_min_chunks", 512))
    floor = {k: max(e32[k] for _, _, e32 in refs.values()) for k in ("dzin", "dgamma", "dbeta")}
    return refs, floor


@pytest.mark.parametrize("name,shape,knob,wgs,label", _dgrad_cases(), ids=[c[0] for c in _dgrad_cases()])
def test_layer_backward(device, dgrad_refs, name, shape, knob, wgs, label):
    lib, check = _lib()
    refs, floor = dgrad_refs
    cin, cout, G, hin, witness = DG_SHAPES[shape]
    hout = (hin - 1) // 2 + 1
    try:
        check(lib.marl_tune(b"dgrad_min_chunks", knob))
        check(lib.marl_tune(b"dgrad_wgs", wgs))
        rows = _dgrad_rows(shape, knob, label)
        p = plan(rows, cin, cout, hin, G, 0)
        # ---- witness
        assert p["dg_supported"] == 1 and p["dg_nt"] == witness["nt"], p
        if label in DG_ROWS:
            rb = 1 if knob == 512 else witness["rb_big"]
            assert p["dg_rb"] == rb and p["dg_mt"] == -(-rb * hin * hin // 16), p
            assert rb > 1 or p["dg_mt"] == witness["mt1"], p
            assert p["dg_blocks"] == -(-rows // rb)
        else:
            w = DG_PERSISTENT["wgs48" if wgs else "resident"][1]
            assert p["dg_rb"] == w["rb"] and p["dg_blocks"] == w["chunks"] and rows % p["dg_rb"] != 0, p
            assert not wgs or w["chunks"] > lib.marl_tune_get(b"dgrad_wgs", 0) == wgs
        (dz, zin, gst, gamma, beta, w4), ref, e32 = refs[(shape, rows)]
        pad = (list(DG_SHAPES).index(shape) + rows) % 2  # alternate a tight and a padded leading dimension of wt
        ldwt = cout + 4 * pad
        wt = th.full((9 * cin, ldwt), float("nan"))
        wt[:, :cout] = w4.permute(2, 3, 1, 0).reshape(9 * cin, cout)  # wt[(kh * 3 + kw) * cin + ci][co]
        emb = [_embed(t, device) for t in (dz, wt, zin, gst, gamma, beta)]
        dzd, wtd, zind, gstd, gd, bd = (v for _, v in emb)
        sb = lib.marl_cnn_dgrad_scratch(rows, cin, cout, hin, G)
        assert sb == p["dg_blocks"] * 2 * cin * 4
        scratch = th.zeros(sb // 4, device=device)
        outs = [_Out((rows, hin * hin, cin), device), _Out((cin,), device), _Out((cin,), device)]

        def run():
            check(lib.marl_cnn_dgrad(dzd.data_ptr(), wtd.data_ptr(), ldwt, zind.data_ptr(), gstd.data_ptr(),
                                     gd.data_ptr(), bd.data_ptr(), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(),
                                     scratch.data_ptr(), sb, rows, cin, cout, hin, G, None))

        got = dict(zip(("dzin", "dgamma", "dbeta"), _twice(run, outs)))
    finally:
        check(lib.marl_tune(b"dgrad_min_chunks", 512))
        check(lib.marl_tune(b"dgrad_wgs", 0))
    e = {k: _rel(got[k], ref[k]) for k in got}
    e.update({"e32_" + k: e32[k] for k in got})
    e.update({"ratio_" + k: e[k] / max(MULT * e32[k], floor[k]) * MULT for k in got})
    e["rows"], e["rb"] = rows, p["dg_rb"]
    _errors["dgrad " + name] = e
    print("dgrad", name, e, "floor", floor)
    assert all(e[k] <= DG_BOUND for k in got), e
    assert all(e[k] <= max(MULT * e32[k], floor[k]) for k in got), (e, floor)


def test_layer_backward_refusals(device):
    """shapes the fused kernel does not cover return MARL_ELIMIT with nothing enqueued; a null pointer MARL_EINVAL; a
    scratch that is too small MARL_ESIZE"""
    lib, _ = _lib()
    buf = th.zeros(1 << 16, device=device)
    out = th.full((1 << 16,), SENTINEL, device=device)
    scratch = th.zeros(4096, device=device)
    b, o = buf.data_ptr(), out.data_ptr()

    def call(cin, cout, hin, G, rows=3, dz=b, scratch_bytes=4096 * 4):
        return lib.marl_cnn_dgrad(dz, b, cout, b, b, b, b, o, o + 4 * 40000, o + 4 * 50000, scratch.data_ptr(), scratch_bytes, rows, cin,
                                  cout, hin, G, None)

    assert call(64, 128, 4, 16) == -2 and lib.marl_cnn_dgrad_scratch(3, 64, 128, 4, 16) == 0  # 8 % G != 0
    assert call(12, 32, 4, 4) == -2  # three channels per group: no power of two
    assert call(16, 32, 4, 2, dz=None) == -1
    assert call(16, 32, 4, 2, dz=b + 4) == -1  # 16-byte alignment
    assert call(16, 32, 4, 2, scratch_bytes=3 * 2 * 16 * 4 - 4) == -4
    th.cuda.synchronize()
    assert th.all(out == SENTINEL), "a refused call wrote"
    assert call(16, 32, 4, 2, scratch_bytes=3 * 2 * 16 * 4) == 0
    th.cuda.synchronize()
    assert not th.any(out[:3 * 16 * 16] == SENTINEL)
