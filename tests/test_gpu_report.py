"""marl_episode_report on the GPU against ``report.reference_counts`` (the definition in float64 torch).

Integer fields must be EQUAL.  That is a fair demand only where no decision of the definition - an argmax, a rank, a
calibration bin, an exit - sits closer to its boundary than fp32 can resolve, so every parity case first asserts, from
the float64 oracle alone, that the top-two gap of every vote and of every agent's row and the gap between the label's
logit and every other class's are >= 1e-5 (fp32 votes differ from float64 by up to 4e-7 at these sizes), and that every
confidence is >= 2e-6 away from every bin edge and threshold (fp32 confidences differ by up to 1.4e-7).  The seeds
below were chosen so that this holds; no case is filtered.  fp64 sums, divided by n, are held to 1e-5 absolute, the
project's logit tolerance.  The largest differences seen go through ``tests.util.record``
(profiles/report_errors.json)."""
import ctypes as C
import json
import os

import pytest
import torch as th

from marlclassification_amd import _lib
from marlclassification_amd import report as R
from marlclassification_amd.report import EpisodeReport, ReportOptions, reference_counts
from tests.cases import _golden_sampler
from tests.dp import run_ranks
from tests.util import record

pytestmark = pytest.mark.gpu

GAP = 1e-5      # every argmax / rank decision is at least this clear in float64
EDGE = 2e-6     # every confidence is at least this far from every bin edge and threshold
SUM_TOL = 1e-5  # fp64 sums / n
_ERRORS = {}

# (Ns, Na, Nb, nC) -> seed: the smallest shapes at which the addressing changes
SHAPES = {
    (4, 3, 37, 45): 0,    # one partly filled wave of classes and an odd batch
    (3, 5, 19, 3): 0,     # the smallest class count in the project's tests
    (2, 1, 130, 10): 0,   # one agent, more images than one pass of a calibration wave
    (2, 2, 7, 130): 0,    # three passes of the class loop
    (3, 33, 5, 45): 0,    # more than 32 agents
    (5, 64, 3, 70): 0,    # 64 agents, the most the kernel must serve
    (2, 2, 300, 4): 0,    # more images than one pass of a sum workgroup's 256 threads
}


def _logits(shape, seed):
    """Seeded normals whose scale grows with the step (and with sqrt(Na): the vote's scale is the same at every Na),
    so that the vote's confidence tends to rise along the episode."""
    ns, na, nb, nc = shape
    g = th.Generator().manual_seed(seed)
    scale = (na ** 0.5) * 3.0 * (th.arange(1, ns + 1, dtype=th.float32) / ns) ** 2
    p = th.randn(ns, na, nb, nc, generator=g) * scale.view(ns, 1, 1, 1)
    y = th.randint(0, nc, (nb,), generator=g)
    return p, y


def _vote64(p):
    """float64 votes z [Ns,Nb,nC] and confidences [Ns,Nb] of fp32 logits, by the definition."""
    p = p.double()
    z = th.zeros_like(p[:, 0])
    for a in range(p.shape[1]):
        z = z + p[:, a]
    z = z / p.shape[1]
    conf = 1.0 / th.exp(z - z.max(dim=2, keepdim=True).values).sum(dim=2)
    return z, conf


def _thresholds(conf):
    """Thresholds from the oracle's confidences [Ns,Nb]: for the image whose confidence sets the most records along
    the steps, one threshold between each record and the one before (so that image exits at every one of those steps),
    and one above every confidence of the batch (nobody exits)."""
    ns = conf.shape[0]
    runmax = th.cummax(conf, dim=0).values
    records = th.cat([th.ones(1, conf.shape[1], dtype=th.bool), conf[1:] > runmax[:-1]], dim=0)
    b = int(records.sum(dim=0).argmax())
    taus = []
    for t in range(ns):
        if records[t, b]:
            below = float(runmax[t - 1, b]) if t else 0.0
            taus.append(0.5 * (below + float(conf[t, b])))
    taus.append(0.5 * (float(conf.max()) + 1.0))
    return tuple(taus[-R.MAX_EXITS:])


def _assert_margins(p, y, opts, exact_conf=None):
    """Every decision of the definition is clear of its boundary, from the float64 oracle alone."""
    z, conf = _vote64(p)
    top2 = z.topk(2, dim=2).values
    assert float((top2[..., 0] - top2[..., 1]).min()) >= GAP, "vote top-two gap"
    if p.shape[3] > 1:
        a2 = p.double().topk(2, dim=3).values
        assert float((a2[..., 0] - a2[..., 1]).min()) >= GAP, "agent top-two gap"
    zy = z.gather(2, y.view(1, -1, 1).expand(z.shape[0], -1, 1))
    d = (z - zy).abs()
    d.scatter_(2, y.view(1, -1, 1).expand(z.shape[0], -1, 1), float("inf"))
    assert float(d.min()) >= GAP, "gap between the label's logit and another class's"
    _assert_conf_margins(conf, opts, exact_conf)
    return conf


def _assert_conf_margins(conf, opts, exact_conf=None):
    c = conf.flatten()
    if exact_conf is not None:  # (confidences that are exact in fp32 and float64 alike may sit ON an edge)
        c = c[c != exact_conf]
    edges = [k / opts.bins for k in range(opts.bins + 1)] + list(opts.exit_thresholds)
    for e in edges:
        if c.numel():
            assert float((c - e).abs().min()) >= EDGE, f"a confidence within {EDGE} of {e}"


def _assert_exit_coverage(conf, opts):
    """Every exit step 0 .. Ns - 1 is reached by meeting some threshold, and some image never meets one."""
    ns = conf.shape[0]
    reached, never = set(), False
    for tau in opts.exit_thresholds:
        ge = conf >= tau
        first = th.where(ge, th.arange(ns).view(ns, 1), ns).min(dim=0).values
        reached |= set(int(v) for v in first if v < ns)
        never = never or bool((first == ns).any())
    assert reached == set(range(ns)), f"exit steps reached: {sorted(reached)}"
    assert never, "no image stays under every threshold"


def _compare(tag, got, want, lay, n=None):
    """(int, f64) buffers: integers equal, sums / n within SUM_TOL; returns and records the differences."""
    gi, gf = got[0].cpu(), got[1].cpu()
    wi, wf = want[0].cpu(), want[1].cpu()
    g, w = R.split_fields(gi, gf, lay), R.split_fields(wi, wf, lay)
    for name in R.INT_FIELDS:
        assert th.equal(g[name], w[name]), f"{tag}: {name}\n got {g[name].tolist()}\nwant {w[name].tolist()}"
    n = max(int(w["n"][0]) if n is None else n, 1)
    errs = {}
    for name in R.F64_FIELDS:
        errs[name] = float((g[name] - w[name]).abs().max()) / n
        assert errs[name] <= SUM_TOL, f"{tag}: {name} / n differs by {errs[name]:.3e}"
    print(f"[report] {tag}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    _ERRORS[tag] = dict(errs, tol=SUM_TOL, integer_fields="equal")
    record("report_errors", _ERRORS)


def _report_of(p, y, opts, device, **kw):
    ns, na, _, nc = p.shape
    rep = EpisodeReport(ns, na, nc, opts, device, **kw)
    rep.add(p.to(device), y.to(device))
    return rep


def _case(shape):
    p, y = _logits(shape, SHAPES[shape])
    _, conf = _vote64(p)
    opts = ReportOptions(topk=min(5, shape[3]), bins=15, exit_thresholds=_thresholds(conf))
    return p, y, opts


# ---- 1: exact parity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_float64_definition(shape, device):
    p, y, opts = _case(shape)
    conf = _assert_margins(p, y, opts)
    _assert_exit_coverage(conf, opts)
    rep = _report_of(p, y, opts, device)
    _compare("parity/" + "x".join(map(str, shape)), rep.buffers(), reference_counts(p, y, opts), rep.layout)


# ---- 2: ties and exact arithmetic -----------------------------------------------------------------------------------
def test_ties_resolve_as_the_definition_says(device):
    # small integers and Na a power of two: every vote is exact in fp32, so equal values are equal in both precisions
    g = th.Generator().manual_seed(1)
    ns, na, nb, nc = 3, 4, 64, 5
    p = th.randint(-2, 3, (ns, na, nb, nc), generator=g).float()
    y = th.randint(0, nc, (nb,), generator=g)
    p[:, :, 0] = 0.0                       # every class equal, for the vote and for every agent
    p[:, :, 1] = th.tensor([1.0, 0, 1, 0, 1])
    y[0], y[1] = 3, 4                      # a label equal to the maximum at a higher index
    z, conf = _vote64(p)
    top = z.max(dim=2, keepdim=True).values
    assert int(((z == top).sum(dim=2) > 1).sum()) > 10, "the case must hold tied votes"
    opts = ReportOptions(topk=3, bins=7, exit_thresholds=(0.3, 0.45))
    _assert_conf_margins(conf, opts)
    rep = _report_of(p, y, opts, device)
    _compare("ties/int5", rep.buffers(), reference_counts(p, y, opts), rep.layout)

    # nC = 2: equal logits give conf = 0.5 exactly, ON an edge of 2 and of 4 bins, and a threshold of 0.5 must exit
    ns, na, nb, nc = 2, 2, 40, 2
    p = th.randint(-3, 4, (ns, na, nb, nc), generator=g).float()
    p[:, :, :8] = 1.0
    p[0, :, 8:12] = 2.0                    # on the edge at step 0 only
    y = th.randint(0, nc, (nb,), generator=g)
    _, conf = _vote64(p)
    assert int((conf[-1] == 0.5).sum()) >= 8 and int((conf[0] == 0.5).sum()) >= 12
    for bins in (2, 4):
        opts = ReportOptions(topk=1, bins=bins, exit_thresholds=(0.5, 0.6))
        _assert_conf_margins(conf, opts, exact_conf=0.5)
        rep = _report_of(p, y, opts, device)
        want = reference_counts(p, y, opts)
        _compare(f"ties/edge_bins{bins}", rep.buffers(), want, rep.layout)
        f = rep.fields()
        assert int(f["cal_count"][bins // 2]) >= 8           # 0.5 * bins truncates to bins / 2
        assert int(f["exit_hist"][0][0]) >= 12               # conf == threshold exits


# ---- 3: skipped images ----------------------------------------------------------------------------------------------
def test_skipped_images_add_to_skipped_and_to_nothing_else(device):
    shape = (4, 3, 37, 45)
    p, y, opts = _case(shape)
    keep = th.ones(shape[2], dtype=th.bool)
    p_bad, y_bad = p.clone(), y.clone()
    p_bad[0, 1, 3, 7] = float("nan")
    p_bad[0, 2, 11, 44] = float("inf")
    p_bad[0, 0, 20, 0] = float("-inf")
    y_bad[5], y_bad[36] = -1, shape[3]
    keep[[3, 11, 20, 5, 36]] = False
    _assert_margins(p[:, :, keep], y[keep], opts)
    rep = _report_of(p_bad, y_bad, opts, device)
    wi, wf = reference_counts(p[:, :, keep], y[keep], opts)
    wi[rep.layout["skipped"][0]] = 5
    _compare("skipped", rep.buffers(), (wi, wf), rep.layout)
    assert int(rep.fields()["skipped"][0]) == 5 and int(rep.fields()["n"][0]) == 32
    # the oracle skips the same images
    oi, of = reference_counts(p_bad, y_bad, opts)
    assert th.equal(oi, wi) and th.equal(of, wf)


# ---- 4: accumulation ------------------------------------------------------------------------------------------------
def test_accumulation_window_overwrite_and_determinism(device):
    shape = (3, 5, 21, 3)
    p, y = _logits(shape, 2)
    _, conf = _vote64(p)
    opts = ReportOptions(topk=2, bins=15, exit_thresholds=_thresholds(conf))
    _assert_margins(p, y, opts)
    pd, yd = p.to(device), y.to(device)
    whole = _report_of(p, y, opts, device)
    thirds = EpisodeReport(*shape[:2], shape[3], opts, device)
    for k in range(3):
        thirds.add(pd[:, :, 7 * k: 7 * k + 7].contiguous(), yd[7 * k: 7 * k + 7])
    _compare("accumulate/thirds", thirds.buffers(), tuple(t.cpu() for t in whole.buffers()), whole.layout)
    # a window of 2 after three adds holds the last two batches
    win = EpisodeReport(*shape[:2], shape[3], opts, device, window_size=2)
    for k in range(3):
        win.add(pd[:, :, 7 * k: 7 * k + 7].contiguous(), yd[7 * k: 7 * k + 7])
    _compare("accumulate/window", win.buffers(), reference_counts(p[:, :, 7:], y[7:], opts), whole.layout)
    # accumulate = 0 over garbage equals a fresh buffer; two identical calls give identical bytes
    lib = _lib.load()
    words = whole.layout["words"]
    outs = []
    for fill in (0, 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A5A5A5A5A):
        buf = th.full((words,), fill, dtype=th.int64, device=device)
        _call(lib, pd, yd, opts, 0, buf, words * 8, device=device)
        outs.append(buf.cpu())
    assert th.equal(outs[0], outs[1]) and th.equal(outs[1], outs[2])
    gi, gf = whole.buffers()
    assert th.equal(outs[0][: whole.layout["int_words"]], gi.cpu())
    assert th.equal(outs[0][whole.layout["int_words"]:].view(th.float64), gf.cpu())


def _call(lib, pd, yd, opts, accumulate, report, report_bytes, scratch=None, scratch_bytes=None, device=None, **over):
    ns, na, nb, nc = pd.shape
    a = dict(ns=ns, na=na, nb=nb, nc=nc, topk=opts.topk, bins=opts.bins, n_exit=len(opts.exit_thresholds),
             preds=pd.data_ptr(), y=yd.data_ptr(), report_ptr=report if isinstance(report, int) else report.data_ptr(),
             taus=(C.c_float * 8)(*opts.exit_thresholds))
    a.update(over)
    if scratch is None:
        need = lib.marl_report_scratch_bytes(ns, na, nb, nc, opts.topk, opts.bins, len(opts.exit_thresholds))
        keep = th.empty(need // 8 + 1, dtype=th.int64, device=device)
        scratch, scratch_bytes = keep.data_ptr(), keep.numel() * 8
    rc = lib.marl_episode_report(a["preds"], a["y"], a["ns"], a["na"], a["nb"], a["nc"], a["topk"], a["bins"],
                                 a["taus"], a["n_exit"], accumulate, a["report_ptr"], report_bytes, scratch,
                                 scratch_bytes,
                                 th.cuda.current_stream(device).cuda_stream)
    th.cuda.synchronize()
    return rc


# ---- 5: memory safety -----------------------------------------------------------------------------------------------
def test_sentinels_around_exactly_sized_buffers_and_the_c_guards(device):
    lib = _lib.load()
    shape = (4, 3, 37, 45)
    p, y, opts = _case(shape)
    pd, yd = p.to(device), y.to(device)
    lay = R.layout(shape[0], shape[1], shape[3], opts)
    ne = len(opts.exit_thresholds)
    rbytes = lay["words"] * 8
    sbytes = lib.marl_report_scratch_bytes(*shape, opts.topk, opts.bins, ne)
    assert sbytes > 0
    G = 64  # guard bytes on either side (the interiors stay 8-byte aligned)
    rep_buf = th.full((rbytes + 2 * G,), 0xA5, dtype=th.uint8, device=device)
    scr_buf = th.full(((sbytes + 7) // 8 * 8 + 2 * G,), 0xA5, dtype=th.uint8, device=device)
    rc = _call(lib, pd, yd, opts, 0, rep_buf.data_ptr() + G, rbytes, scr_buf.data_ptr() + G, sbytes, device=device)
    assert rc == 0, lib.marl_last_error()
    for buf, n in ((rep_buf, rbytes), (scr_buf, sbytes)):
        assert bool((buf[:G] == 0xA5).all()) and bool((buf[G + n:] == 0xA5).all()), "a sentinel was overwritten"
    got = rep_buf[G: G + rbytes].cpu().view(th.int64)
    wi, wf = reference_counts(p, y, opts)
    _compare("sentinels", (got[: lay["int_words"]], got[lay["int_words"]:].view(th.float64)), (wi, wf), lay)

    # every guard returns its code and enqueues nothing: the report keeps its fill
    EINVAL, ELIMIT, ESIZE = -1, -2, -4
    fill = th.full((lay["words"],), 0x5A5A5A5A5A5A5A5A, dtype=th.int64, device=device)
    nan_tau = (C.c_float * 8)(0.5, float("nan"))
    big_tau = (C.c_float * 8)(1.5)
    cases = [
        (EINVAL, dict(preds=None)), (EINVAL, dict(y=None)), (EINVAL, dict(report_ptr=None)),
        (EINVAL, dict(topk=0)), (EINVAL, dict(bins=0)), (EINVAL, dict(taus=nan_tau, n_exit=2)),
        (EINVAL, dict(taus=big_tau, n_exit=1)), (EINVAL, dict(taus=None, n_exit=1)),
        (ELIMIT, dict(nc=1025)), (ELIMIT, dict(topk=17)), (ELIMIT, dict(bins=65)), (ELIMIT, dict(n_exit=9)),
        (ELIMIT, dict(na=65)),
    ]
    for code, over in cases:
        assert _call(lib, pd, yd, opts, 0, fill, rbytes, device=device, **over) == code, over
    assert _call(lib, pd, yd, opts, 0, fill, rbytes - 8, device=device) == ESIZE
    keep = th.empty(sbytes // 8 + 1, dtype=th.int64, device=device)
    assert _call(lib, pd, yd, opts, 0, fill, rbytes, keep.data_ptr(), sbytes - 4, device=device) == ESIZE
    assert _call(lib, pd, yd, opts, 0, fill, rbytes, 0, sbytes, device=device) == EINVAL  # (a null scratch)
    assert bool((fill == 0x5A5A5A5A5A5A5A5A).all()), "a refused call wrote to the report"
    # 64 agents are served
    assert lib.marl_report_scratch_bytes(5, 64, 3, 70, 5, 15, 0) > 0


# ---- 6: standing in for the meter, a side stream ----------------------------------------------------------------------
def test_conf_mat_equals_the_confusion_meter(device):
    from marlclassification_amd.metrics import ConfusionMeter

    shape = (4, 3, 37, 45)
    p, y, opts = _case(shape)
    _assert_margins(p, y, opts)
    pd, yd = p.to(device), y.to(device)
    for window in (None, 2):
        rep = EpisodeReport(shape[0], shape[1], shape[3], opts, device, window_size=window)
        meter = ConfusionMeter(shape[3], window_size=window)
        for lo, hi in ((0, 10), (10, 25), (25, 37)):
            part = pd[:, :, lo:hi].contiguous()
            rep.add(part, yd[lo:hi])
            meter.add(part[-1].mean(dim=0), yd[lo:hi])
        assert th.equal(rep.conf_mat(), meter.conf_mat())
        assert th.equal(rep.precision(), meter.precision()) and th.equal(rep.recall(), meter.recall())


def test_add_on_a_side_stream(device):
    shape = (4, 3, 37, 45)
    p, y, opts = _case(shape)
    want = _report_of(p, y, opts, device).buffers()
    side = th.cuda.Stream(device)
    rep = EpisodeReport(shape[0], shape[1], shape[3], opts, device)
    with th.cuda.stream(side):
        pd = p.to(device, non_blocking=True) * 1.0  # produced on the side stream: only stream order protects it
        rep.add(pd, y.to(device))
    side.synchronize()
    got = rep.buffers()
    assert th.equal(got[0], want[0]) and th.equal(got[1], want[1])


# ---- 7: trainer -------------------------------------------------------------------------------------------------------
def test_trainer_metrics_come_from_the_report(device):
    from marlclassification_amd.training import Trainer
    from tests.util import Golden

    g = Golden("g1_conftest")
    opts = ReportOptions(topk=3, bins=15, exit_thresholds=(0.5,))
    model, sampler = _golden_sampler(g, device)
    trainer = Trainer(model, g.cfg.nb_class, g.lr, g.gamma, report=opts)
    preds = []
    for _ in range(2):
        out, _ = trainer.train_step(g.img, g.y, sampler)
        preds.append(out.step_preds.detach().cpu().clone())
    m = trainer.metrics()
    assert preds[0].shape == (g.ns, g.na, g.nb, g.cfg.nb_class) and not th.equal(preds[0], preds[1])
    wi = wf = None
    for pr in preds:
        _assert_margins(pr, g.y, opts)
        i, f = reference_counts(pr, g.y, opts)
        wi, wf = (i, f) if wi is None else (wi + i, wf + f)
    lay = R.layout(g.ns, g.na, g.cfg.nb_class, opts)
    _compare("trainer/two_steps", trainer.report.buffers(), (wi, wf), lay)
    res = R.result_from_fields(R.split_fields(wi, wf, lay), opts, g.na)
    cm = th.tensor(res["confusion"], dtype=th.float)
    want = dict(R.summary_metrics(res, opts, "train"),
                train_prec=(cm.diagonal() / (cm.sum(0) + 1e-8)).mean().item(),
                train_rec=(cm.diagonal() / (cm.sum(1) + 1e-8)).mean().item())
    assert set(want) == {"train_acc", "train_top3", "train_nll", "train_ece", "train_prec", "train_rec"}
    for k, v in want.items():
        assert m[k] == pytest.approx(v, abs=SUM_TOL), k

    # without `report`: the keys of before, and the confusion meter behind them
    model2, sampler2 = _golden_sampler(g, device)
    plain = Trainer(model2, g.cfg.nb_class, g.lr, g.gamma)
    plain.train_epoch([(g.img, g.y)], 0, sampler2)
    assert set(plain.metrics()) == {"error", "path_loss", "loss", "critic_loss", "train_prec", "train_rec"}
    assert plain.report is None


def test_eval_epoch_fills_a_report(device):
    from marlclassification_amd.training import Trainer
    from tests.util import Golden

    g = Golden("g1_conftest")
    opts = ReportOptions(topk=3, bins=15, exit_thresholds=(0.5,))
    model, sampler = _golden_sampler(g, device)
    trainer = Trainer(model, g.cfg.nb_class, g.lr, g.gamma)
    loader = [(g.img, g.y), (g.img, g.y)]  # (the sampler's fixed draws fit the fixture's batch size)
    rep = EpisodeReport(g.ns, g.na, g.cfg.nb_class, opts, device)
    got = trainer.eval_epoch(loader, 0, sampler, report=rep)
    assert got is rep
    meter = trainer.eval_epoch(loader, 0, sampler)
    assert th.equal(rep.conf_mat(), meter.conf_mat().to(rep.conf_mat().device))
    with th.no_grad():
        pr = sampler.run_episode(g.img).step_preds.cpu()
    _assert_margins(pr, g.y, opts)
    i, f = reference_counts(pr, g.y, opts)
    _compare("trainer/eval_epoch", rep.buffers(), (2 * i, 2 * f), rep.layout)
    r = rep.result()
    assert r["n"] == 2 * g.nb and len(r["accuracy"]) == g.ns and len(r["agent_accuracy"][0]) == g.na


# ---- 8: command line --------------------------------------------------------------------------------------------------
def test_command_line_test_mode_writes_the_report(device, tmp_path, capsys):
    import numpy as np
    from PIL import Image

    from marlclassification_amd.__main__ import main
    from marlclassification_amd.config import ModelConfig

    root = tmp_path / "images"
    rng = np.random.default_rng(0)
    for c in range(3):
        (root / f"class{c}").mkdir(parents=True)
        for k in range(7):
            arr = rng.integers(0, 256, (28, 28), dtype=np.uint8)
            arr[4 * c: 4 * c + 8] = 255
            Image.fromarray(arr).save(root / f"class{c}" / f"img{k}.png")
    mc = ModelConfig(ft_extr_str="mnist", window_size=6, hidden_size_belief=32, hidden_size_action=32,
                     hidden_size_msg=8, hidden_size_msg_output=12, hidden_size_state=8, state_dim=2,
                     actions=[[1, 0], [-1, 0], [0, 1], [0, -1]], nb_class=3, hidden_size_linear_belief=48,
                     hidden_size_linear_action=48)
    mc.save_marl_config(str(tmp_path / "marl.json"))
    th.manual_seed(11)
    th.save(mc.build_marl(3)[0].state_dict(), tmp_path / "sd.pt")
    out = tmp_path / "out"
    main((f"-a 3 --step 4 --cuda --run-id rep test --dataset-path {root} --json-path {tmp_path / 'marl.json'} "
          f"--state-dict-path {tmp_path / 'sd.pt'} --img-size 28 --batch-size 8 -o {out} --report --report-topk 2 "
          f"--exit-at 0.5,0.9").split())
    printed = capsys.readouterr().out
    assert "Precision mean" in printed and "exit at confidence >= 0.5" in printed
    r = json.loads((out / "report.json").read_text())
    assert r["n"] == 21 and r["skipped"] == 0
    for k in ("accuracy", "topk", "agent_accuracy", "agreement", "nll"):
        assert len(r[k]) == 4, k
    assert len(r["exits"]) == 2 and sum(r["exits"][0]["exit_hist"]) == 21
    assert sum(map(sum, r["confusion"])) == 21
    assert (out / "accuracy_per_step.png").stat().st_size > 0
    # --tta: the views are stacked along the agent axis
    out2 = tmp_path / "out_tta"
    main((f"-a 3 --step 4 --cuda --run-id rep test --dataset-path {root} --json-path {tmp_path / 'marl.json'} "
          f"--state-dict-path {tmp_path / 'sd.pt'} --img-size 28 --batch-size 8 -o {out2} --report --tta hflip").split())
    r2 = json.loads((out2 / "report.json").read_text())
    assert r2["n"] == 21 and len(r2["agent_accuracy"][0]) == 6


# ---- 9: two ranks -----------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from marlclassification_amd.parallel import shard_bounds

    device = th.device("cuda:0")  # both ranks share the one GPU of the test box
    shape = (4, 3, 37, 45)
    p, y, opts = _case(shape)
    lo, hi = shard_bounds(36, rank, world)
    rep = EpisodeReport(shape[0], shape[1], shape[3], opts, device)
    rep.add(p[:, :, lo:hi].contiguous().to(device), y[lo:hi].to(device))
    rep.all_reduce()
    i, f = rep.buffers()
    if rank == 0:
        out_q.put((i.cpu().numpy(), f.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_all_reduce_to_the_report_of_the_whole_set(device):
    (gi, gf), = run_ranks(_dp_worker, 2)
    shape = (4, 3, 37, 45)
    p, y, opts = _case(shape)
    single = _report_of(p[:, :, :36].contiguous(), y[:36], opts, device)
    si, sf = single.buffers()
    assert th.equal(th.from_numpy(gi), si.cpu())
    assert float((th.from_numpy(gf) - sf.cpu()).abs().max()) / 36 <= SUM_TOL
