"""GPU: the row passes of the batched backward through their own entry points (marl_ln_silu_bwd,
marl_gn_silu_bwd) against a float64 torch-CPU LayerNorm / GroupNorm + SiLU backward (autograd).

LayerNorm grid: every kernel form of csrc/rowops.hip's register pass - the full 384-wide row with a
compile-time source (plain, kin = 1, kin = 4), the same width through the run-time form (kin = 3), a
predicated U = 6 width (320), the full and a predicated U = 2 width (128, 96), one 16-lane row (16) and its
ragged form (13) - at one row, a ragged wave, a block boundary with a tail and two blocks with a one-row
tail.  The statistics come from the library's own forward entry, as in the episode.  Leading dimensions
alternate over the grid between tight ones with dz written in place of da (what the episode does) and
padded ones with a separate dz.

Bound: 1e-4 of the tensor's largest magnitude for dZ, dgamma and dbeta (the gradient bound of DESIGN.md
section 2).  With MARL_ROW_BWD_ERRORS=<file> in the environment the achieved errors of every case are
written there as JSON (profiles/row_bwd_errors.json is one such run)."""
import json
import os

import pytest
import torch as th
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = 1e-4
LN_M = [1, 67, 16 * 16 + 3, 2 * 16 * 16 + 1]
LN_N = [384, 320, 128, 96, 16, 13]
LN_KIN = [0, 1, 4, 3]  # 0: plain da; 3 has no compile-time form
_errors = {}


def _lib():
    from marlclassification_amd import _lib

    return _lib.load(), _lib.check


@pytest.fixture(scope="module", autouse=True)
def _error_record():
    yield
    path = os.environ.get("MARL_ROW_BWD_ERRORS")
    if path and _errors:
        with open(path, "w") as f:
            json.dump({"bound_rel_to_max": BOUND, "cases": _errors}, f, indent=1, sort_keys=True)


def _padded(t, ld, device):
    out = th.zeros(t.shape[0], ld, device=device)
    out[:, : t.shape[1]] = t.to(device)
    return out


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _scratch(m, n, device):
    return th.empty(max(256, -(-m // 256)) * 2 * n, device=device)


@pytest.mark.parametrize("kin", LN_KIN)
@pytest.mark.parametrize("n", LN_N)
@pytest.mark.parametrize("m", LN_M)
def test_ln_silu_bwd(device, m, n, kin):
    lib, check = _lib()
    pad = (LN_M.index(m) + LN_N.index(n) + LN_KIN.index(kin)) % 2
    gen = th.Generator().manual_seed(1000 * m + 10 * n + kin)
    z = th.randn(m, n, generator=gen) * 2 + 0.5
    gamma = th.randn(n, generator=gen)
    beta = th.randn(n, generator=gen) * 0.5
    if kin:
        g = th.randn(m, kin, generator=gen)
        w1t = th.randn(n, kin, generator=gen)
        da64 = g.double() @ w1t.double().t()
    else:
        da = th.randn(m, n, generator=gen)
        da64 = da.double()

    # float64 reference
    z64 = z.double().requires_grad_()
    g64, b64 = gamma.double().requires_grad_(), beta.double().requires_grad_()
    F.silu(F.layer_norm(z64, (n,), g64, b64, 1e-5)).backward(da64)

    ldz = n + 4 * pad
    zd = _padded(z, ldz, device)
    gd, bd = gamma.to(device), beta.to(device)
    stats = th.zeros(m, 2, device=device)
    act = th.zeros(m, n, device=device)
    check(lib.marl_ln_silu_fwd(zd.data_ptr(), ldz, gd.data_ptr(), bd.data_ptr(), act.data_ptr(), n,
                               stats.data_ptr(), m, n, None))
    dgamma, dbeta = th.full((n,), 7.0, device=device), th.full((n,), 7.0, device=device)  # (overwritten)
    scratch = _scratch(m, n, device)
    if kin:
        ldg, ldw, lddz = 4 + 4 * pad, 4, n + 8 * pad
        gdv, wdv = _padded(g, ldg, device), _padded(w1t, ldw, device)
        dz = th.zeros(m, lddz, device=device)
        check(lib.marl_ln_silu_bwd(None, 0, gdv.data_ptr(), ldg, kin, wdv.data_ptr(), ldw, zd.data_ptr(), ldz,
                                   stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), dz.data_ptr(), lddz,
                                   dgamma.data_ptr(), dbeta.data_ptr(), scratch.data_ptr(),
                                   scratch.numel() * 4, m, n, None))
    else:
        ldda = n + 12 * pad
        dad = _padded(da, ldda, device)
        dz, lddz = (th.zeros(m, n + 8, device=device), n + 8) if pad else (dad, ldda)  # tight: in place
        check(lib.marl_ln_silu_bwd(dad.data_ptr(), ldda, None, 0, 0, None, 0, zd.data_ptr(), ldz,
                                   stats.data_ptr(), gd.data_ptr(), bd.data_ptr(), dz.data_ptr(), lddz,
                                   dgamma.data_ptr(), dbeta.data_ptr(), scratch.data_ptr(),
                                   scratch.numel() * 4, m, n, None))
    th.cuda.synchronize()
    e = {"dz": _rel(dz[:, :n].cpu(), z64.grad), "dgamma": _rel(dgamma.cpu(), g64.grad),
         "dbeta": _rel(dbeta.cpu(), b64.grad)}
    _errors[f"ln m={m} n={n} kin={kin} pad={pad}"] = e
    print(f"ln m={m} n={n} kin={kin} pad={pad}: {e}")
    assert th.equal(dz[:, n:].cpu(), th.zeros(m, dz.shape[1] - n)), "wrote past the row"
    assert e["dz"] <= BOUND and e["dgamma"] <= BOUND and e["dbeta"] <= BOUND, e


# (P, C, G, da_chw): the Resisc45 extractor's last layer (the register-resident row kernel, its gradient
# arriving in the feature layout [C][P] with a row stride larger than C * P); a power-of-two channel count
# whose row is no multiple of 64 (the flat kernel); a channel count that is no power of two (the general one)
GN_SHAPES = [(4, 64, 8, 1), (9, 32, 4, 0), (9, 24, 3, 0)]


@pytest.mark.parametrize("P,C,G,chw", GN_SHAPES)
@pytest.mark.parametrize("rows", [1, 67, 259])
def test_gn_silu_bwd(device, rows, P, C, G, chw):
    lib, check = _lib()
    gen = th.Generator().manual_seed(100 * rows + C)
    z = th.randn(rows, P, C, generator=gen) * 2 + 0.5  # NHWC rows
    gamma = th.randn(C, generator=gen)
    beta = th.randn(C, generator=gen) * 0.5
    da = th.randn(rows, C, P, generator=gen) if chw else th.randn(rows, P, C, generator=gen)
    ldda = C * P + (40 if chw else 0)

    z64 = z.double().requires_grad_()
    g64, b64 = gamma.double().requires_grad_(), beta.double().requires_grad_()
    x = z64.permute(0, 2, 1)  # [rows, C, P]
    F.silu(F.group_norm(x, G, g64, b64, 1e-5)).backward(da.double() if chw else da.double().permute(0, 2, 1))
    # the statistics the forward pass would have kept (there is no GroupNorm forward entry): float64, rounded once
    xg = z.double().permute(0, 2, 1).reshape(rows, G, -1)
    stats = th.stack([xg.mean(-1), 1.0 / th.sqrt(xg.var(-1, unbiased=False) + 1e-5)], -1).float().to(device)

    zd = z.to(device).contiguous()
    dad = _padded(da.reshape(rows, -1), ldda, device)
    gd, bd = gamma.to(device), beta.to(device)
    dz = th.zeros(rows, P, C, device=device)
    dgamma, dbeta = th.full((C,), 7.0, device=device), th.full((C,), 7.0, device=device)
    scratch = _scratch(rows, C, device)
    check(lib.marl_gn_silu_bwd(dad.data_ptr(), ldda, chw, zd.data_ptr(), stats.data_ptr(), gd.data_ptr(),
                               bd.data_ptr(), dz.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                               scratch.data_ptr(), scratch.numel() * 4, rows, P, C, G, None))
    th.cuda.synchronize()
    e = {"dz": _rel(dz.cpu(), z64.grad), "dgamma": _rel(dgamma.cpu(), g64.grad),
         "dbeta": _rel(dbeta.cpu(), b64.grad)}
    _errors[f"gn rows={rows} P={P} C={C} G={G} chw={chw}"] = e
    print(f"gn rows={rows} P={P} C={C} G={G} chw={chw}: {e}")
    assert e["dz"] <= BOUND and e["dgamma"] <= BOUND and e["dbeta"] <= BOUND, e
