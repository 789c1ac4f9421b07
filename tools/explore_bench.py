"""Cost of the exploration controls (``marl_policy_explore``) against ANOTHER checkout (the parent commit, built), every
leg a fresh child process, alternating on one box:

    python tools/explore_bench.py --parent DIR [--rounds 3] [--steps 100] [--warmup 10] [--out profiles/explore_c3.json]

  * the unchanged path: ``rounds`` x (parent, this tree) ``bench.py --gpus 1`` at C3; this tree's median must lie inside
    the parent's own spread; ``--dump-outputs`` of both trees compared array by array (np.array_equal);
  * the exploration path: ``Trainer.train_step`` at C3, B = 256 - the parent's plain step, this tree's plain step, this
    tree under (tau 2, eps 0.1) and this tree greedy - in the same alternation (``--leg`` is the child's entry);
  * one ``rocprofv3 --kernel-trace --stats`` run of its own (plain steps, then steps under (2, 0.1), in one process): the
    durations of the EXPLORE instantiations and of policy_dlogits_explore_kernel next to their plain siblings."""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTIONS = [[1, 0], [-1, 0], [0, 1], [0, -1]]
SETTINGS = {"plain": None, "explore": (2.0, 0.1, False), "greedy": (1.0, 0.0, True)}


def med(v):
    return sorted(v)[len(v) // 2]


# ---- the child: Trainer.train_step at C3 in the tree named by the working directory ---------------------------------
def leg(names, iters, batch):
    sys.path.insert(0, os.getcwd())
    import torch as th

    from bench import C3, IMG, NA, NS
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import CNN_BY_NAME
    from marlclassification_amd.training import Trainer

    dev = th.device("cuda", 0)
    img = th.rand(batch, *IMG, device=dev)
    y = th.randint(C3["nb_class"], (batch,), device=dev)
    out = {}
    for name in names:
        th.manual_seed(0)
        model = ModelsWrapper(CNN_BY_NAME[C3["ft_extr"]](C3["window"]), C3["n_b"], C3["n_a"], C3["n_m"], C3["n_m_o"],
                              C3["n_d"], 2, len(ACTIONS), C3["nb_class"], C3["nlb"], C3["nla"]).to(dev)
        if SETTINGS[name] is not None:
            model.set_exploration(*SETTINGS[name])
        sampler = EpisodeSampler(MultiAgent(NA, model), Environment(ACTIONS, C3["window"]), NS)
        trainer = Trainer(model, C3["nb_class"], 1e-4, 0.99)
        for _ in range(5):
            trainer.train_step(img, y, sampler)
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            trainer.train_step(img, y, sampler)
        th.cuda.synchronize()
        out[name] = round(1e3 * (time.perf_counter() - t0) / iters, 4)
    print(json.dumps(out))


# ---- the parent process -------------------------------------------------------------------------------------------
def run(cmd, tree, prefix=(), timeout=600):
    r = subprocess.run(list(prefix) + [sys.executable] + cmd, cwd=tree, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} in {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-3000:]}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]) if lines else {}


def trace(args):
    import sqlite3

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from rocpd_stats import short

    d = tempfile.mkdtemp(prefix="explore_trace_")
    run([os.path.abspath(__file__), "--leg", "plain,explore", "--iters", "20", "--batch", str(args.batch)], ROOT,
        prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "r", "--"])
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    if not dbs:
        raise SystemExit(f"no trace database under {d}")
    db = sqlite3.connect(dbs[0])
    cols = [row[1] for row in db.execute("pragma table_info(kernels)")]
    namecol = "name" if "name" in cols else "kernel_name"
    agg = {}
    for n, dur in db.execute(f"select {namecol}, (end - start) from kernels"):
        n = short(n)
        if "sample_kernel" in n or "panel_fwd_kernel" in n or "policy_dlogits" in n:
            a = agg.setdefault(n, [0, 0])
            a[0] += 1
            a[1] += dur
    return {k: {"calls": c, "avg_us": round(ns / c / 1e3, 3), "total_ms": round(ns / 1e6, 3)}
            for k, (c, ns) in sorted(agg.items())}


def main():
    import numpy as np

    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="checkout of the parent commit (built)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) comma-separated settings: plain, explore, greedy")
    args = ap.parse_args()
    if args.leg:
        leg(args.leg.split(","), args.iters, args.batch)
        return
    parent = os.path.abspath(args.parent)
    res = {"workload": "bench.py --gpus 1 (C3: RESISC45 dims, 16 agents, 16 steps, 256 images)", "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    bench = ["bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup", str(args.warmup)]
    ms = {"parent": [], "this": []}
    for rnd in range(args.rounds):
        for who, tree in (("parent", parent), ("this", ROOT)):
            ms[who].append(run(bench, tree)["ms_per_step"])
        print(f"round {rnd}: parent {ms['parent'][-1]:.3f} ms, this tree {ms['this'][-1]:.3f} ms", flush=True)
    res["unchanged_path_ms_per_step"] = ms
    res["unchanged_path"] = {
        "parent_median_ms": med(ms["parent"]), "median_ms": med(ms["this"]),
        "parent_min_ms": min(ms["parent"]), "parent_max_ms": max(ms["parent"]),
        "median_inside_parent_spread": min(ms["parent"]) <= med(ms["this"]) <= max(ms["parent"]),
        "median_not_slower_than_parent_max": med(ms["this"]) <= max(ms["parent"])}
    save()

    dumps = {}
    with tempfile.TemporaryDirectory() as dp, tempfile.TemporaryDirectory() as dt:
        run(bench + ["--dump-outputs", dp], parent)
        run(bench + ["--dump-outputs", dt], ROOT)
        names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(dp, "*.npy")))
        assert names == sorted(os.path.basename(f) for f in glob.glob(os.path.join(dt, "*.npy"))), names
        for n in names:
            a, b = np.load(os.path.join(dp, n)), np.load(os.path.join(dt, n))
            dumps[n] = bool(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b))
    res["dump_outputs_equal"] = dumps
    res["dump_outputs_all_equal"] = bool(dumps) and all(dumps.values())
    print(f"dump-outputs: {dumps}", flush=True)
    save()

    me = os.path.abspath(__file__)
    step = {"parent_plain": [], "plain": [], "explore_t2_e0.1": [], "greedy": []}
    for rnd in range(args.rounds):
        child = [me, "--iters", str(args.iters), "--batch", str(args.batch), "--leg"]
        step["parent_plain"].append(run(child + ["plain"], parent)["plain"])
        for key, name in (("plain", "plain"), ("explore_t2_e0.1", "explore"), ("greedy", "greedy")):
            step[key].append(run(child + [name], ROOT)[name])
        print(f"round {rnd}: train_step " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in step.items()), flush=True)
    res["train_step_ms"] = step
    res["train_step"] = {k + "_median_ms": med(v) for k, v in step.items()}
    res["train_step"]["parent_spread_ms"] = max(step["parent_plain"]) - min(step["parent_plain"])
    res["train_step"]["explore_minus_parent_ms"] = med(step["explore_t2_e0.1"]) - med(step["parent_plain"])
    res["train_step"]["greedy_minus_parent_ms"] = med(step["greedy"]) - med(step["parent_plain"])
    save()

    if not args.no_trace:
        res["kernel_trace"] = trace(args)
        print(json.dumps(res["kernel_trace"]), flush=True)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
