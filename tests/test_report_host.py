"""CPU: the episode report's host side (marlclassification_amd/report.py) - option guards, the float64 definition
``reference_counts`` against a loop written out by hand, ties, skipped images, the arithmetic of ``result()``, the
two-rank all-reduce, the library's exports and the command-line flags."""
import ctypes as C
import math
import os

import pytest
import torch as th
import torch.distributed as dist

from marlclassification_amd import _lib
from marlclassification_amd import report as R
from marlclassification_amd.report import EpisodeReport, ReportOptions, reference_counts
from tests.dp import run_ranks


def _fields(step_preds, y, opts):
    ns, na, _, nc = step_preds.shape
    i, f = reference_counts(step_preds, y, opts)
    return R.split_fields(i, f, R.layout(ns, na, nc, opts))


# ---- options -----------------------------------------------------------------------------------------------------
def test_options_defaults_and_guards():
    o = ReportOptions()
    assert (o.topk, o.bins, o.exit_thresholds) == (5, 15, ())
    assert ReportOptions(16, 64, (0.0, 1.0)).exit_thresholds == (0.0, 1.0)
    for bad in (dict(topk=0), dict(topk=17), dict(bins=0), dict(bins=65), dict(topk=2.5), dict(topk=True),
                dict(exit_thresholds=(1.5,)), dict(exit_thresholds=(-0.1,)), dict(exit_thresholds=(float("nan"),)),
                dict(exit_thresholds=(float("inf"),)), dict(exit_thresholds=tuple([0.5] * 9)),
                dict(exit_thresholds=5)):
        with pytest.raises(ValueError):
            ReportOptions(**bad)
    # thresholds are the fp32 values the kernel compares with
    assert ReportOptions(exit_thresholds=(0.9,)).exit_thresholds[0] == th.tensor(0.9).item()
    for sizes in ((0, 1, 2), (1025, 1, 2), (1, 65, 2), (1, 0, 2), (1, 1, 1025), (1, 1, 0)):
        with pytest.raises(ValueError):
            R.layout(*sizes, o)
    with pytest.raises(ValueError):
        EpisodeReport(2, 2, 3, o, "cpu", window_size=0)
    with pytest.raises(ValueError):
        R.parse_exit_at("0.5,x")
    assert R.parse_exit_at("0.5, 0.9") == (0.5, 0.9) and R.parse_exit_at(None) == ()


# ---- the definition, by hand ------------------------------------------------------------------------------------
# 2 steps, 2 agents, 3 images, 3 classes; labels 0, 2, 1
_P = th.tensor([
    # step 0
    [[[2.0, 0.0, 0.0], [0.0, 1.0, 3.0], [0.0, 0.0, 0.5]],     # agent 0: argmax 0, 2, 2
     [[0.0, 1.0, 0.0], [0.0, 2.0, 1.0], [1.0, 0.0, 0.5]]],    # agent 1: argmax 1, 1, 0
    # step 1
    [[[4.0, 0.0, 0.0], [0.0, 0.0, 4.0], [0.0, 3.0, 0.0]],     # agent 0: argmax 0, 2, 1
     [[2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 1.0, 2.0]]],    # agent 1: argmax 0, 1, 2
])
_Y = th.tensor([0, 2, 1])


def _lse(z):
    m = max(z)
    return m, sum(math.exp(v - m) for v in z)


def test_reference_counts_against_a_written_out_case():
    opts = ReportOptions(topk=2, bins=4, exit_thresholds=(0.6, 0.99))
    f = _fields(_P, _Y, opts)
    # votes z[t][b] = mean over the two agents
    z = [[[1.0, 0.5, 0.0], [0.0, 1.5, 2.0], [0.5, 0.0, 0.5]],
         [[3.0, 0.0, 0.0], [0.0, 1.0, 2.0], [0.0, 2.0, 1.0]]]
    assert int(f["n"][0]) == 3 and int(f["skipped"][0]) == 0
    # vote predictions: step 0 -> 0, 2, 0 (a tie of classes 0 and 2: the lowest index); step 1 -> 0, 2, 1
    assert f["vote_hit"].tolist() == [2, 3]
    # ranks of the labels: step 0 -> 0, 0, 2 (image 2: z_1 = 0 under both 0.5s); step 1 -> 0, 0, 0
    assert f["rank_hist"].tolist() == [[2, 0, 1], [3, 0, 0]]
    # agents' own hits (argmaxes in the comments of _P)
    assert f["agent_hit"].tolist() == [[2, 0], [3, 1]]
    # agents that agree with the vote: step 0 -> (a0: 0,2,2 vs 0,2,0 = 2) + (a1: 1,1,0 = 1); step 1 -> 3 + 1
    assert f["agree"].tolist() == [3, 4]
    nll = [[0.0] * 3 for _ in range(2)]
    conf = [[0.0] * 3 for _ in range(2)]
    for t in range(2):
        for b in range(3):
            m, s = _lse(z[t][b])
            nll[t][b] = -(z[t][b][int(_Y[b])] - m - math.log(s))
            conf[t][b] = 1.0 / s
    assert f["nll_sum"].tolist() == pytest.approx([sum(nll[0]), sum(nll[1])], abs=1e-12)
    assert f["confusion"].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
    # last step's confidences: 1 / (1 + 2 e^-3) = 0.909, 1 / (1 + e^-1 + e^-2) = 0.665 (twice) -> bins 3, 2, 2 of 4
    assert [int(c * 4) for c in conf[1]] == [3, 2, 2]
    assert f["cal_count"].tolist() == [0, 0, 2, 1] and f["cal_hit"].tolist() == [0, 0, 2, 1]
    assert f["cal_conf"].tolist() == pytest.approx([0.0, 0.0, conf[1][1] + conf[1][2], conf[1][0]], abs=1e-12)
    # step-0 confidences: 0.506, 0.574, 0.384 -> at 0.6 images exit at steps 1, 1, 1; at 0.99 nobody exits: Ns - 1
    assert max(conf[0]) < 0.6 and min(conf[1]) > 0.6 and max(conf[1]) < 0.99
    assert f["exit_hist"].tolist() == [[0, 3], [0, 3]] and f["exit_hit"].tolist() == [3, 3]


def test_reference_counts_exits_at_the_first_confident_step():
    opts = ReportOptions(exit_thresholds=(0.5, 0.55))
    f = _fields(_P, _Y, opts)
    # step-0 confidences 0.506, 0.574, 0.384: at 0.5 images 0 and 1 stop at step 0 (both right), image 2 goes on to
    # step 1 (right there); at 0.55 only image 1 stops at step 0
    assert f["exit_hist"].tolist() == [[2, 1], [1, 2]] and f["exit_hit"].tolist() == [3, 3]


def test_reference_counts_ties():
    # every class equal: the lowest index wins, for the vote and for each agent
    p = th.zeros(1, 2, 3, 4)
    y = th.tensor([0, 2, 3])
    f = _fields(p, y, ReportOptions(topk=3, bins=4, exit_thresholds=(0.25,)))
    assert f["vote_hit"].tolist() == [1] and f["agent_hit"].tolist() == [[1, 1]] and f["agree"].tolist() == [6]
    # the rank counts equal logits at LOWER indices ahead of the label: ranks 0, 2, 3 (= topk: "beyond")
    assert f["rank_hist"].tolist() == [[1, 0, 1, 1]]
    assert f["confusion"][:, 0].tolist() == [1, 0, 1, 1]
    # conf = 1 / 4 exactly: bin 1 of 4, and a threshold equal to it exits
    assert f["cal_count"].tolist() == [0, 3, 0, 0] and f["exit_hist"].tolist() == [[3]]
    # a label that equals the maximum at a higher index: not a hit, rank 1
    p = th.tensor([[[[1.0, 0.0, 1.0]]]])
    f = _fields(p, th.tensor([2]), ReportOptions(topk=2))
    assert f["vote_hit"].tolist() == [0] and f["rank_hist"].tolist() == [[0, 1, 0]]


def test_reference_counts_skips_images():
    g = th.Generator().manual_seed(3)
    p = th.randn(3, 2, 7, 5, generator=g)
    y = th.randint(0, 5, (7,), generator=g)
    opts = ReportOptions(topk=2, bins=5, exit_thresholds=(0.4,))
    p_bad, y_bad = p.clone(), y.clone()
    p_bad[0, 1, 0, 2] = float("nan")
    p_bad[2, 0, 2, 0] = float("inf")
    p_bad[1, 1, 3, 4] = float("-inf")
    y_bad[5] = -1
    y_bad[6] = 5
    keep = th.tensor([1, 4])
    want_i, want_f = reference_counts(p[:, :, keep], y[keep], opts)
    got_i, got_f = reference_counts(p_bad, y_bad, opts)
    lay = R.layout(3, 2, 5, opts)
    assert int(got_i[lay["skipped"][0]]) == 5 and int(got_i[lay["n"][0]]) == 2
    want_i[lay["skipped"][0]] = 5
    assert th.equal(got_i, want_i) and th.equal(got_f, want_f)
    # nothing valid: only `skipped` moves
    i, f = reference_counts(p_bad[:, :, :1], y_bad[:1], opts)
    assert int(i.sum()) == 1 and float(f.abs().sum()) == 0.0


def test_layout_matches_the_library():
    lib = _lib.load()
    slots = ("n skipped vote_hit rank_hist agent_hit agree confusion cal_count cal_hit exit_hist exit_hit nll_sum "
             "cal_conf").split()
    for ns, na, nc, opts in ((4, 3, 45, ReportOptions()), (5, 64, 70, ReportOptions(16, 64, (0.1,) * 8)),
                             (1, 1, 1, ReportOptions(1, 1))):
        out = (C.c_int64 * (len(slots) + 1))()
        assert lib.marl_report_layout(ns, na, nc, opts.topk, opts.bins, len(opts.exit_thresholds), out) == 0
        lay = R.layout(ns, na, nc, opts)
        assert [lay[s][0] for s in slots] + [lay["words"]] == list(out)
        assert lay["int_words"] == lay["nll_sum"][0]
        assert lib.marl_report_scratch_bytes(ns, na, 7, nc, opts.topk, opts.bins, len(opts.exit_thresholds)) > 0
    out = (C.c_int64 * 14)()
    assert lib.marl_report_layout(4, 65, 45, 5, 15, 0, out) == -2      # MARL_ELIMIT
    assert lib.marl_report_layout(4, 3, 1025, 5, 15, 0, out) == -2
    assert lib.marl_report_layout(4, 3, 45, 17, 15, 0, out) == -2
    assert lib.marl_report_layout(4, 3, 45, 5, 65, 0, out) == -2
    assert lib.marl_report_layout(4, 3, 45, 5, 15, 9, out) == -2
    assert lib.marl_report_layout(4, 3, 45, 0, 15, 0, out) == -1       # MARL_EINVAL
    assert lib.marl_report_layout(4, 3, 45, 5, 0, 0, out) == -1
    assert lib.marl_report_layout(4, 3, 45, 5, 15, 0, None) == -1
    assert lib.marl_report_scratch_bytes(4, 65, 7, 45, 5, 15, 0) == 0


def test_exports_and_abi_unchanged():
    assert _lib.REPORT_ENTRIES == ("marl_report_layout", "marl_report_scratch_bytes", "marl_episode_report")
    assert set(_lib.REPORT_ENTRIES) <= set(_lib._HOOKS)
    assert len(_lib.EXPORTS) == 57 and _lib.MARL_ABI_VERSION == 5
    lib = _lib.load()
    assert lib.marl_abi_version() == 5 and all(hasattr(lib, s) for s in _lib.REPORT_ENTRIES)


# ---- result() ----------------------------------------------------------------------------------------------------
def test_result_arithmetic():
    opts = ReportOptions(topk=3, bins=2, exit_thresholds=(0.5,))
    rep = EpisodeReport(2, 2, 3, opts, "cpu")
    lay = rep.layout
    i = th.zeros(lay["int_words"], dtype=th.int64)
    f = th.zeros(lay["words"] - lay["int_words"], dtype=th.float64)
    v = R.split_fields(i, f, lay)
    v["n"][0], v["skipped"][0] = 10, 2
    v["vote_hit"].copy_(th.tensor([4, 7]))
    v["rank_hist"].copy_(th.tensor([[4, 3, 2, 1], [7, 1, 1, 1]]))
    v["agent_hit"].copy_(th.tensor([[3, 5], [6, 8]]))
    v["agree"].copy_(th.tensor([10, 16]))
    v["nll_sum"].copy_(th.tensor([12.0, 5.0]))
    v["cal_count"].copy_(th.tensor([4, 6]))
    v["cal_hit"].copy_(th.tensor([1, 6]))
    v["cal_conf"].copy_(th.tensor([1.6, 5.1]))
    v["exit_hist"].copy_(th.tensor([[3, 7]]))
    v["exit_hit"].copy_(th.tensor([6]))
    v["confusion"].copy_(th.tensor([[3, 1, 0], [0, 2, 1], [1, 0, 2]]))
    rep.merge(i, f)
    r = rep.result()
    assert r["n"] == 10 and r["skipped"] == 2
    assert r["accuracy"] == [0.4, 0.7]
    assert r["topk"] == [[0.4, 0.7, 0.9], [0.7, 0.8, 0.9]]           # cumulative over the ranks
    assert r["agent_accuracy"] == [[0.3, 0.5], [0.6, 0.8]]
    assert r["agreement"] == [0.5, 0.8]                               # agree / (n * Na)
    assert r["nll"] == [1.2, 0.5]
    assert r["ece"] == pytest.approx((abs(1 - 1.6) + abs(6 - 5.1)) / 10)
    assert r["exits"][0]["mean_steps"] == pytest.approx((1 * 3 + 2 * 7) / 10)
    assert r["exits"][0]["exit_accuracy"] == 0.6 and r["exits"][0]["exit_hist"] == [3, 7]
    assert r["confusion"] == [[3, 1, 0], [0, 2, 1], [1, 0, 2]]
    # ConfusionMeter's formulas
    cm = th.tensor(r["confusion"], dtype=th.float)
    assert th.equal(rep.conf_mat(), cm.long())
    assert th.allclose(rep.precision(), cm.diagonal() / (cm.sum(0) + 1e-8))
    assert th.allclose(rep.recall(), cm.diagonal() / (cm.sum(1) + 1e-8))
    m = R.summary_metrics(r, opts, "eval")
    assert m == {"eval_acc": 0.7, "eval_top3": 0.9, "eval_nll": 0.5, "eval_ece": r["ece"]}
    assert len(R.step_table(r, opts)) == 1 + 2 + 1
    rep.merge(i, f)                                                   # merging adds
    assert rep.result()["n"] == 20 and rep.result()["accuracy"] == [0.4, 0.7]
    assert EpisodeReport(2, 2, 3, opts, "cpu").result()["accuracy"] == [0.0, 0.0]  # nothing seen: zeros, no division
    with pytest.raises(ValueError):
        rep.merge(i[:-1], f)
    with pytest.raises(RuntimeError):                                 # no CPU implementation of add
        rep.add(th.zeros(2, 2, 4, 3), th.zeros(4, dtype=th.long))


def test_to_json(tmp_path):
    import json

    opts = ReportOptions(exit_thresholds=(0.5,))
    rep = EpisodeReport(2, 2, 3, opts, "cpu")
    rep.merge(*reference_counts(_P, _Y, opts))
    path = rep.to_json(str(tmp_path / "report.json"))
    with open(path) as fh:
        r = json.load(fh)
    assert r["n"] == 3 and len(r["accuracy"]) == 2 and r == rep.result()


# ---- two ranks ---------------------------------------------------------------------------------------------------
def _case(seed=5):
    g = th.Generator().manual_seed(seed)
    p = th.randn(3, 2, 10, 4, generator=g) * th.tensor([1.0, 2.0, 4.0]).view(3, 1, 1, 1)
    y = th.randint(0, 4, (10,), generator=g)
    return p, y, ReportOptions(topk=2, bins=5, exit_thresholds=(0.5, 0.9))


def _worker(rank, world, port, out_q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    th.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    p, y, opts = _case()
    lo, hi = rank * 5, rank * 5 + 5
    rep = EpisodeReport(3, 2, 4, opts, "cpu")
    rep.merge(*reference_counts(p[:, :, lo:hi], y[lo:hi], opts))
    rep.all_reduce()
    i, f = rep.buffers()
    if rank == 1:
        out_q.put((i.numpy(), f.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_all_reduce():
    (gi, gf), = run_ranks(_worker, 2, get_timeout=300)
    p, y, opts = _case()
    wi, wf = reference_counts(p, y, opts)
    assert th.equal(th.from_numpy(gi), wi)
    assert th.allclose(th.from_numpy(gf), wf, rtol=0, atol=1e-12)


# ---- command line --------------------------------------------------------------------------------------------------
def test_cli_flags():
    from marlclassification_amd.__main__ import build_parser, check_report
    from marlclassification_amd.config import EvalConfig, TrainConfig

    p = build_parser()
    test_argv = "--run-id r --cuda test --dataset-path d --json-path j --state-dict-path s -o o".split()
    a = p.parse_args(test_argv)
    assert (a.report, a.report_topk, a.report_bins, a.exit_at) == (False, 5, 15, None)
    check_report(p, a)
    a = p.parse_args(test_argv + "--report --report-topk 3 --report-bins 10 --exit-at 0.5,0.9".split())
    assert (a.report, a.report_topk, a.report_bins, a.exit_at) == (True, 3, 10, "0.5,0.9")
    check_report(p, a)
    t = p.parse_args("--run-id r train -o o --report --exit-at 0.8".split())
    assert t.report and t.exit_at == "0.8"
    for bad in (["--exit-at", "0.5"], ["--report", "--exit-at", "1.5"], ["--report", "--report-topk", "17"],
                ["--report", "--report-bins", "0"], ["--report-topk", "3"]):
        with pytest.raises(SystemExit):
            check_report(p, p.parse_args(test_argv + bad))
    # their absence leaves the configs as they were
    e = EvalConfig(img_size=28, state_dict_path="s", batch_size=8, json_path="j", dataset_path="d", output_dir="o")
    assert (e.report, e.report_topk, e.report_bins, e.exit_at) == (False, 5, 15, None)
    c = TrainConfig(img_size=28, nb_epoch=1, learning_rate=1e-3, batch_size=8, resources_dir="r", output_dir="o",
                    gamma=0.99)
    assert (c.report, c.report_topk, c.report_bins, c.exit_at) == (False, 5, 15, None)
