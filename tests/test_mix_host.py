"""CPU: CutMix / Mixup and soft targets, everything that needs no GPU - the ``--mix`` grammar, the definition
``mix.reference_apply`` and its sanitising, the label shares (``label_weights`` / ``soft_targets`` / ``primary_labels``),
the torch definitions of the soft vote error and rewards (``class_loss.vote_error(targets=)`` / ``rewards(targets=)``)
against ``F.cross_entropy`` in float64, the statistics of ``Policy.draw``, and the guards of ``marl_soft_targets``."""
import math
import os
import re

import pytest
import torch as th
import torch.nn.functional as F

from marlclassification_amd import _lib, augment, mix
from marlclassification_amd import class_loss as cl
from marlclassification_amd.__main__ import build_parser
from tests.buffers import same_bits as _same_bits
from tests.buffers import source as _source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header):
    with open(os.path.join(ROOT, "include", header), "r", encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(marl_[a-z0-9_]+)\s*\(", text))


ROWS = th.tensor([6, 0, 3, 3, 5])
OPS = th.tensor([[0, 0, 0, 0, 0, 0, 0, 0], [2, 1, -1, 0, 0, 0, 0, 0], [4, 0, 2, 1, 1, 3, 3, 0],
                 [6, -2, 0, 0, 0, 0, 0, 0], [2, 0, 0, 2, 0, 2, 9, 0]], dtype=th.int32)
DTYPES = [th.uint8, th.float32]


# ---- the grammar --------------------------------------------------------------------------------------------------
def test_grammar():
    p = mix.parse("cutmix:1.0,mixup:0.4:0.3")
    assert (p.cutmix_alpha, p.cutmix_p, p.mixup_alpha, p.mixup_p) == (1.0, 0.5, 0.4, 0.3)
    assert p.spec == "cutmix:1.0,mixup:0.4:0.3"
    p = mix.parse("cutmix")
    assert (p.cutmix_alpha, p.cutmix_p, p.mixup_p) == (1.0, 0.5, 0.0)
    p = mix.parse(" mixup:2:1 ")
    assert (p.mixup_alpha, p.mixup_p, p.cutmix_p) == (2.0, 1.0, 0.0)
    assert mix.parse("cutmix:0.5:0.5,mixup:0.5:0.5").cutmix_p == 0.5  # (a sum of exactly 1 is allowed)


@pytest.mark.parametrize("spec,word", [
    ("", "unknown token"), ("cutout", "unknown token"), ("cutmix:1:0.5:3", "unknown token"), ("cutmix:x", "bad token"),
    ("cutmix:0", "alpha"), ("mixup:-1", "alpha"), ("mixup:1:1.5", "probability"), ("mixup:1:nan", "bad token"),
    ("cutmix:1:0.7,mixup:1:0.4", "sum"), ("cutmix,cutmix", "twice"), ("cutmix,,mixup", "unknown token"),
])
def test_grammar_errors_name_the_token(spec, word):
    with pytest.raises(ValueError, match=word):
        mix.parse(spec)
    with pytest.raises(ValueError):
        mix.parse(None)


def test_command_line_takes_mix_for_training_only(capsys):
    parser = build_parser()
    base = "-a 3 --step 3 --run-id x train --ft-extr mnist --f 6 --img-size 28 --res-folder synthetic -o out"
    args = parser.parse_args((base + " --mix cutmix:1.0,mixup:0.4:0.3 --augment hflip").split())
    assert args.mix == "cutmix:1.0,mixup:0.4:0.3" and args.augment == "hflip"
    assert parser.parse_args(base.split()).mix is None
    with pytest.raises(SystemExit):
        parser.parse_args((base + " --mix cutmix:1:0.9,mixup:1:0.9").split())
    assert "sum" in capsys.readouterr().err
    for sub in ("test", "infer"):
        with pytest.raises(SystemExit):
            parser.parse_args(f"-a 3 --step 3 --run-id x {sub} --mix cutmix".split())
    capsys.readouterr()


# ---- the definition -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32"])
@pytest.mark.parametrize("mode", ["reflect", "zero"])
def test_reference_properties(dtype, mode):
    shape = (3, 12, 20)
    c, h, w = shape
    src = _source(shape, dtype, n=7)
    fill = 200 if dtype == th.uint8 else -1.5
    views = augment.reference_apply(src, ROWS, OPS, mode, fill)
    nb = ROWS.shape[0]
    cycle = th.tensor([1, 2, 3, 4, 0])

    def run(partner, m, box=(0, 0, 0, 0), k=256):
        mx = th.zeros(nb, 8, dtype=th.int32)
        mx[:, 0], mx[:, 1], mx[:, 6] = partner, m, k
        mx[:, 2:6] = th.tensor(box, dtype=th.int32)
        return mix.reference_apply(src, ROWS, OPS, mx, mode, fill)

    # mode 0 (and mix=None) is the augmenting gather, whatever the other fields say
    assert _same_bits(mix.reference_apply(src, ROWS, OPS, None, mode, fill), views)
    assert _same_bits(run(cycle, 0, (2, 3, 5, 5), 7), views)
    # partner == self is the identity: CutMix in both types; Mixup in integer arithmetic (k v + (256 - k) v = 256 v) -
    # in fp32 the two rounded products need not add up to v, so there the identity holds at k = 0 and k = 256 only
    me = th.arange(nb)
    assert _same_bits(run(me, 1, (2, 3, 5, 9)), views)
    for k in (0, 256) if dtype == th.float32 else (0, 1, 77, 128, 255, 256):
        assert _same_bits(run(me, 2, k=k), views), k
    # a box covering the image gives the partner's view (under the partner's own row and ops)
    assert _same_bits(run(cycle, 1, (0, 0, h, w)), views[cycle])
    assert _same_bits(run(cycle, 1, (-5, -5, h + 10, w + 10)), views[cycle])
    # an empty box gives view b; a box is [by, by + bh) x [bx, bx + bw)
    assert _same_bits(run(cycle, 1, (2, 3, 0, 5)), views)
    got = run(cycle, 1, (2, 3, 4, 6))
    want = views.clone()
    want[:, :, 2:6, 3:9] = views[cycle][:, :, 2:6, 3:9]
    assert _same_bits(got, want)
    # k = 256 gives view b, k = 0 view p
    assert _same_bits(run(cycle, 2, k=256), views)
    assert _same_bits(run(cycle, 2, k=0), views[cycle])
    # the blend itself
    got = run(cycle, 2, k=77)
    if dtype == th.uint8:
        want = ((77 * views.long() + 179 * views[cycle].long() + 128) >> 8).to(th.uint8)
    else:
        want = th.tensor(77 / 256) * views + th.tensor(179 / 256) * views[cycle]
    assert _same_bits(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "f32"])
def test_hostile_values_stay_in_range(dtype):
    shape = (2, 8, 8)
    src = _source(shape, dtype, n=7)
    nb = 5
    rows, ops = ROWS, OPS
    views = augment.reference_apply(src, rows, ops)
    big = 2**31 - 1
    hostile = th.tensor([[-5, 1, 0, 0, 8, 8, 256, 0],            # partner below 0 -> image 0
                         [10**9, 1, 0, 0, 8, 8, 256, 0],         # partner beyond the batch -> the last image
                         [2, 7, 0, 0, 8, 8, 0, 0],               # mode 7 -> 3 -> none
                         [1, 1, -big - 1, -big - 1, big, big, 256, 0],   # a box of +-2^31: by + bh = -1 -> empty
                         [3, 1, -big, -big, big, big, 256, 0],   # by + bh = 0: empty as well
                         ], dtype=th.int32)
    got = mix.reference_apply(src, rows, ops, hostile)
    assert _same_bits(got[0], views[0]) and _same_bits(got[1], views[nb - 1]) and _same_bits(got[2], views[2])
    assert _same_bits(got[3], views[3]) and _same_bits(got[4], views[4])
    wide = th.tensor([[1, 1, -4, -big, big, big, 256, 0]] * nb, dtype=th.int32)  # rows [-4, big - 4) x columns [-big, 0)
    assert _same_bits(mix.reference_apply(src, rows, ops, wide), views)
    wide[:, 3] = -3  # columns [-3, big - 3): the whole image
    assert _same_bits(mix.reference_apply(src, rows, ops, wide), views[th.tensor([1] * nb)])
    for k, same_as in ((-1, 0), (999, 256)):
        a = th.tensor([[1, 2, 0, 0, 0, 0, k, 0]] * nb, dtype=th.int32)
        b = th.tensor([[1, 2, 0, 0, 0, 0, same_as, 0]] * nb, dtype=th.int32)
        assert _same_bits(mix.reference_apply(src, rows, ops, a), mix.reference_apply(src, rows, ops, b))
    lam = mix.label_weights(th.cat([hostile, wide]), 8, 8)
    assert bool(((lam >= 0) & (lam <= 1)).all())
    with pytest.raises(ValueError):
        mix.reference_apply(src, rows, ops, hostile[:3])


# ---- the label shares ---------------------------------------------------------------------------------------------
def _drawn(batch, h, w, seed=5):
    return mix.parse("cutmix:1:0.4,mixup:0.4:0.4").draw(batch, th.Generator().manual_seed(seed), (h, w))


def test_label_weights_and_soft_targets():
    h, w, nc, nb = 12, 20, 7, 512
    m = _drawn(nb, h, w)
    assert set(m[:, 1].tolist()) == {0, 1, 2}
    y = th.randint(0, nc, (nb,), generator=th.Generator().manual_seed(1))
    lam = mix.label_weights(m, h, w)
    assert lam.dtype == th.float32 and lam.shape == (nb,)
    mode, k = m[:, 1], m[:, 6]
    area = (m[:, 4] * m[:, 5]).double()  # (drawn boxes are clipped already)
    want = th.where(mode == 1, (h * w - area) / (h * w), th.where(mode == 2, k.double() / 256, th.ones(nb).double()))
    assert th.equal(lam, want.float())
    q = mix.soft_targets(y, m, h, w, nc)
    assert q.dtype == th.float32 and q.shape == (nb, nc)
    ulp = th.finfo(th.float32).eps
    assert float((q.sum(dim=1).double() - 1.0).abs().max()) <= ulp, "rows sum to 1 within one fp32 ulp"
    plain = mode == 0
    assert th.equal(q[plain], F.one_hot(y[plain], nc).float()), "exactly one-hot where nothing is mixed"
    p = m[:, 0].long()
    dense = lam.view(-1, 1).double() * F.one_hot(y, nc) + (1 - want).view(-1, 1) * F.one_hot(y[p], nc)
    assert float((q.double() - dense).abs().max()) <= ulp
    assert bool((q >= 0).all()) and bool(((q > 0).sum(dim=1) <= 2).all())
    # a box clipped by the image counts its clipped area
    one = th.tensor([[0, 1, -3, 15, 6, 10, 256, 0]], dtype=th.int32)  # rows [0, 3) x columns [15, 20)
    assert mix.label_weights(one, h, w).item() == th.tensor((240 - 15) / 240).float().item()
    with pytest.raises(ValueError):
        mix.soft_targets(y[:3], m, h, w, nc)


def test_primary_labels():
    h, w = 8, 8
    m = th.tensor([[1, 0, 0, 0, 0, 0, 256, 0],   # none: own
                   [2, 1, 0, 0, 4, 8, 256, 0],   # half the image: lam = 0.5 -> own
                   [3, 1, 0, 0, 5, 8, 256, 0],   # more than half: the partner's
                   [0, 2, 0, 0, 0, 0, 128, 0],   # k = 128: lam = 0.5 -> own
                   [0, 2, 0, 0, 0, 0, 127, 0],   # below: the partner's
                   [4, 2, 0, 0, 0, 0, 0, 0]], dtype=th.int32)
    y = th.tensor([10, 11, 12, 13, 14, 15])
    assert mix.primary_labels(y, m, h, w).tolist() == [10, 11, 13, 13, 10, 14]


# ---- the soft vote error and rewards in float64 -------------------------------------------------------------------
@pytest.mark.parametrize("nc", [3, 45])
def test_soft_vote_error_is_torch_cross_entropy_with_probabilities(nc):
    g = th.Generator().manual_seed(nc)
    ns, na, nb = 3, 2, 6
    preds = th.randn(ns, na, nb, nc, generator=g, dtype=th.float64) * 4
    q = th.rand(nb, nc, generator=g, dtype=th.float64)
    q[0, 1:] = 0  # a one-hot row and rows with exact zeros
    q[1, ::2] = 0
    q = q / q.sum(dim=1, keepdim=True)
    w = th.rand(nc, generator=g, dtype=th.float64) + 0.25
    s = th.tensor([0.0, 0.5, 2.0], dtype=th.float64)
    y = th.zeros(nb, dtype=th.int64)
    z = preds.mean(dim=1)
    for weight, eps in ((None, 0.0), (w, 0.0), (None, 0.1), (w, 0.1)):
        want = th.stack([F.cross_entropy(z[t], q, weight=weight, label_smoothing=eps, reduction="none")
                         for t in range(ns)])
        got = cl.vote_error(preds, y, weight, eps, targets=q)
        assert float((got - want).abs().max()) <= 1e-13
        got = cl.vote_error(preds, y, weight, eps, s, targets=q)
        assert float((got - want * s.view(ns, 1)).abs().max()) <= 1e-13
    # a one-hot Q is the integer-label form, for the error and for the rewards
    y = th.randint(0, nc, (nb,), generator=g)
    hot = F.one_hot(y, nc).double()
    for weight, eps in ((None, 0.0), (w, 0.1)):
        a, b = cl.vote_error(preds, y, weight, eps, s), cl.vote_error(preds, y, weight, eps, s, targets=hot)
        assert float((a - b).abs().max()) <= 1e-13
        a, b = cl.rewards(preds, y, weight), cl.rewards(preds, y, weight, targets=hot)
        assert float((a - b).abs().max()) <= 1e-13
    # the rewards are linear in Q
    r = cl.rewards(preds, y, w, targets=q)
    parts = sum(q[:, c].view(1, 1, nb) * cl.rewards(preds, th.full((nb,), c), w) for c in range(nc))
    assert float((r - parts).abs().max()) <= 1e-12
    # entries with Q == 0 are skipped: a logit of -inf there stays out of the sums and of the gradient
    p2 = preds.clone()
    p2[:, :, 1, 0] = -math.inf
    p2.requires_grad_()
    e = cl.vote_error(p2, y, None, 0.0, targets=q)
    assert bool(th.isfinite(e).all()) and bool(th.isfinite(cl.rewards(p2, y, targets=q)).all())
    e.sum().backward()
    assert bool(th.isfinite(p2.grad).all())
    with pytest.raises(ValueError):
        cl.vote_error(preds, y, targets=q[:, :-1])


# ---- the draw -----------------------------------------------------------------------------------------------------
def test_draw_statistics():
    n, alpha = 20000, 0.4
    lam = mix.Policy.beta(alpha, n, th.Generator().manual_seed(0)).double()
    assert bool(((lam >= 0) & (lam <= 1)).all())
    assert abs(lam.mean().item() - 0.5) <= 0.02
    var = 1.0 / (4 * (2 * alpha + 1))
    assert abs(lam.var().item() / var - 1.0) <= 0.05
    h, w = 12, 20
    policy = mix.parse(f"cutmix:{alpha}:0.5,mixup:{alpha}:0.3")
    m = policy.draw(n, th.Generator().manual_seed(0), (h, w))
    assert m.dtype == th.int32 and m.shape == (n, 8)
    assert th.equal(m[:, 0].long().sort().values, th.arange(n)), "partner is a permutation"
    by, bx, bh, bw = (m[:, j].long() for j in (2, 3, 4, 5))
    assert bool(((by >= 0) & (bx >= 0) & (bh >= 0) & (bw >= 0) & (by + bh <= h) & (bx + bw <= w)).all())
    mode = m[:, 1]
    frac = [(mode == j).double().mean().item() for j in range(3)]
    assert abs(frac[1] - 0.5) < 0.02 and abs(frac[2] - 0.3) < 0.02 and abs(frac[0] - 0.2) < 0.02
    assert bool((m[mode != 1][:, 2:6] == 0).all()) and bool((m[mode != 2][:, 6] == 256).all())
    k = m[mode == 2][:, 6].double()
    assert bool(((k >= 0) & (k <= 256)).all()) and abs(k.mean().item() / 256 - 0.5) <= 0.03
    assert bool((m[:, 7] == 0).all())
    # the same generator state gives the same draw; the mixed share of CutMix follows Beta too (clipping only shrinks
    # the box: the own share is at least lam')
    again = policy.draw(n, th.Generator().manual_seed(0), (h, w))
    assert th.equal(m, again)
    lam_cut = mix.label_weights(m[mode == 1], h, w)
    assert 0.5 <= lam_cut.mean().item() <= 0.75
    with pytest.raises(ValueError):
        mix.Policy(cutmix_p=0.6, mixup_p=0.6)


# ---- the library entries ------------------------------------------------------------------------------------------
def test_entry_points_live_beside_the_versioned_abi():
    assert _declared("marl_hip_softtargets.h") == {"marl_soft_targets"} == set(_lib.SOFTTARGET_ENTRIES)
    assert _declared("marl_hip_mix.h") == {"marl_batch_mix", "marl_batch_mix_plan"} == set(_lib.MIX_ENTRIES)
    for name in _lib.SOFTTARGET_ENTRIES + _lib.MIX_ENTRIES:
        assert name not in _declared("marl_hip.h") and name not in _lib.EXPORTS
    assert _lib.MARL_ABI_VERSION == 5


def test_library_guards_answer_without_a_device():
    import ctypes as C

    lib = _lib.load()
    with open(os.path.join(ROOT, "include", "marl_hip.h"), "r", encoding="utf-8") as f:
        einval = int(re.search(r"#define MARL_EINVAL \((-?\d+)\)", f.read()).group(1))
    fake = C.c_void_p(4096)  # (never read: the setting only keeps the pointer)
    try:
        for args in ((fake, -1, 10), (fake, 4, -1), (fake, 0, 10), (fake, 4, 0), (None, 4, 10)):
            assert lib.marl_soft_targets(*args) == einval, args
            assert b"soft_targets" in lib.marl_last_error()
        assert lib.marl_soft_targets(fake, 4, 10) == 0
    finally:
        assert lib.marl_soft_targets(None, 0, 0) == 0
    # the mix launcher's guards are those of the augmenting gather
    info = mix.MixPlan()
    assert lib.marl_batch_mix_plan(3, 8, 8, 2, None, None, C.byref(info)) == einval
    assert lib.marl_batch_mix_plan(3, 8, 0, 1, None, None, C.byref(info)) == einval
    assert lib.marl_batch_mix_plan(3, 64, 64, 1, None, C.c_void_p(4096), C.byref(info)) == 0
    assert info.as_dict() == {"store_bytes": 16, "band_vectors": 1024, "blocks_per_image": 1, "lds_bytes": 0}
    assert lib.marl_batch_mix_plan(1, 5, 7, 1, None, C.c_void_p(4096), C.byref(info)) == 0 and info.store_bytes == 1
    assert lib.marl_batch_mix(None, 4, fake, None, None, None, 4, 3, 8, 8, 1, 0, 0, None) == einval
    assert lib.marl_batch_mix(fake, 4, C.c_void_p(1 << 20), None, None, None, 4, 3, 8, 8, 1, 5, 0, None) == einval
    assert lib.marl_batch_mix(fake, 4, fake, None, None, None, 4, 3, 8, 8, 1, 0, 0, None) == einval  # dst overlaps src
    assert b"overlaps" in lib.marl_last_error()


def test_apply_refuses_a_cpu_tensor():
    with pytest.raises(RuntimeError, match="GPU"):
        mix.apply(_source((1, 5, 7), th.uint8, n=7))
