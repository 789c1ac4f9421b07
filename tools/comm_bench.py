"""Trainer.train_step at the flagship shape (bench.py's C3: RESISC45 dims, 16 agents, 16 steps, B = 256) under
communication graphs, next to the plain step of ANOTHER checkout (the parent commit) as the yardstick.

    python tools/comm_bench.py --parent DIR [--rounds 3] [--steps 30] [--warmup 5] [--out profiles/comm_c3.json]
    python tools/comm_bench.py --one GRAPH [--tree DIR]       # one leg: plain | full | ring | none (a JSON line)
    python tools/comm_bench.py --grad --parent DIR [--out profiles/comm_grad_c3.json]   # the learnable graph
    python tools/comm_bench.py --range R --parent DIR [--out profiles/comm_range_c3.json]   # range-limited exchange

Every leg is a fresh child process; a round runs parent-plain, plain, full, ring, none in that order, so the legs
alternate with the yardstick on one box.  ``--tree DIR`` imports the package (and bench.py's constants) from DIR.
``--grad``: the cost of learning the matrix (marl_comm_grad + the torch launches of the masked softmax, its backward
and Adam on Na^2 values) - a round runs the PARENT's constant full(16), this tree's constant full(16), then
``learn_full`` and ``learn_ring`` (``comm.LearnableComm`` on that support, ``Trainer(comm_lr=...)``); the yardstick is
the parent's constant-matrix step and its own round-to-round spread.  ``--trace`` (with ``--grad``) then runs the
constant and the ``learn_full`` leg once more under ``rocprofv3 --kernel-trace``, lists every kernel the learnable step
launches beyond the constant one (calls per step, average duration, the new kernels against their 8 us estimate) and
compares the legs' excess with the sum of those durations plus the parent's spread.
``--range R``: the cost of gating the exchange by the agents' positions (``set_comm_range(R)``) - a round runs the
PARENT's constant full(16), this tree's constant full(16), then ``range_full`` and ``range_ring`` (that base under the
range); the yardstick is again the parent's constant-matrix step and its own round-to-round spread."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("plain", "full", "ring", "none")
GRAD_LEGS = ("full", "learn_full", "learn_ring")  # (after the parent's constant full)
RANGE_LEGS = ("full", "range_full", "range_ring")  # (likewise)


def one(graph: str, tree: str, steps: int, warmup: int, batch: int, radius: int = -1) -> None:
    sys.path.insert(0, tree)
    import torch as th

    import bench
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import CNN_BY_NAME
    from marlclassification_amd.training import Trainer

    c, dev = bench.C3, th.device("cuda", 0)
    actions = [[1, 0], [-1, 0], [0, 1], [0, -1]]
    th.manual_seed(0)
    model = ModelsWrapper(CNN_BY_NAME[c["ft_extr"]](c["window"]), c["n_b"], c["n_a"], c["n_m"], c["n_m_o"], c["n_d"],
                          2, len(actions), c["nb_class"], c["nlb"], c["nla"]).to(dev)
    form, kw = None, {}
    if graph.startswith("learn_"):
        from marlclassification_amd import comm

        model.set_comm(comm.LearnableComm(getattr(comm, graph[6:])(bench.NA)).to(dev))
        kw = {"comm_lr": bench.LR}
    elif graph.startswith("range_"):
        from marlclassification_amd import comm

        if radius < 0:
            raise SystemExit("comm_bench: a range_* leg needs --range R")
        model.set_comm(getattr(comm, graph[6:])(bench.NA).to(dev))
        model.set_comm_range(radius)
    elif graph != "plain":
        from marlclassification_amd import comm

        model.set_comm(getattr(comm, graph)(bench.NA).to(dev))
    sampler = EpisodeSampler(MultiAgent(bench.NA, model), Environment(actions, c["window"]), bench.NS)
    trainer = Trainer(model, c["nb_class"], bench.LR, bench.GAMMA, **kw)
    gen = th.Generator(device=dev).manual_seed(0)
    img = th.rand(batch, *bench.IMG, device=dev, generator=gen)
    y = th.randint(0, c["nb_class"], (batch,), device=dev, generator=gen)
    for _ in range(warmup):
        trainer.train_step(img, y, sampler)
    th.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out, scalars = trainer.train_step(img, y, sampler)
    th.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    if not bool(th.isfinite(scalars).all()) or not bool(th.isfinite(out.step_preds).all()):
        raise SystemExit("comm_bench: non-finite outputs")
    if graph != "plain":
        form = model.hip_engine(actions).plan_query("comm_form")
    res = {"graph": graph, "ms_per_step": ms, "steps": steps, "batch": batch, "comm_form": form,
           "loss": scalars[0].item()}
    if graph.startswith("range_"):
        res["comm_range"] = model.hip_engine(actions).plan_query("comm_range")
    print(json.dumps(res))


def leg(graph: str, tree: str, args) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--one", graph, "--tree", tree, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--batch", str(args.batch)]
    if graph.startswith("range_"):
        cmd += ["--range", str(args.range)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree)
    if r.returncode != 0:
        raise SystemExit(f"leg {graph} in {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=LEGS + GRAD_LEGS[1:] + RANGE_LEGS[1:])
    ap.add_argument("--range", type=int, default=None, metavar="R",
                    help="the range-limited legs (radius R, chebyshev, normalised) against the parent's constant full")
    ap.add_argument("--grad", action="store_true", help="the learnable-graph legs against the parent's constant full")
    ap.add_argument("--trace", action="store_true", help="with --grad: kernel traces of the launches a learnable step adds")
    ap.add_argument("--trace-steps", type=int, default=10)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", help="checkout of the parent commit (built): its plain step is the yardstick")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one:
        one(args.one, os.path.abspath(args.tree), args.steps, args.warmup, args.batch,
            -1 if args.range is None else args.range)
        return
    if not args.parent:
        ap.error("--parent DIR (or --one GRAPH)")
    if args.grad:
        grad_rounds(args)
        return
    if args.range is not None:
        range_rounds(args)
        return
    res = {"parent_plain": []}
    res.update({g: [] for g in LEGS})
    forms = {}
    for rnd in range(args.rounds):
        res["parent_plain"].append(leg("plain", os.path.abspath(args.parent), args)["ms_per_step"])
        for g in LEGS:
            r = leg(g, ROOT, args)
            res[g].append(r["ms_per_step"])
            forms[g] = r["comm_form"]
        print(f"round {rnd}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in res.items()), flush=True)
    p = res["parent_plain"]
    summary = {"workload": "Trainer.train_step, bench.py C3 (RESISC45 dims, 16 agents, 16 steps)", "batch": args.batch,
               "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "ms_per_step": res,
               "comm_form": forms, "parent_spread_ms": max(p) - min(p), "parent_median_ms": sorted(p)[len(p) // 2],
               "median_ms": {k: sorted(v)[len(v) // 2] for k, v in res.items()}}
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


def _trace(graph: str, steps: int, warmup: int, batch: int) -> dict:
    """One leg under rocprofv3 --kernel-trace (a run of its own): kernel name -> [calls, total ns]."""
    import glob
    import sqlite3
    import tempfile

    from rocpd_stats import short

    d = tempfile.mkdtemp(prefix=f"comm_bench_{graph}_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "r", "--", sys.executable, os.path.abspath(__file__),
           "--one", graph, "--steps", str(steps), "--warmup", str(warmup), "--batch", str(batch)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, TMPDIR="/tmp"))
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    if r.returncode != 0 or not dbs:
        raise SystemExit(f"trace of {graph} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    db = sqlite3.connect(dbs[0])
    cols = [row[1] for row in db.execute("pragma table_info(kernels)")]
    namecol = "name" if "name" in cols else "kernel_name"
    agg = {}
    for n, dur in db.execute(f"select {namecol}, (end - start) from kernels"):
        a = agg.setdefault(short(n), [0, 0])
        a[0] += 1
        a[1] += dur
    return agg


def added_launches(args) -> dict:
    """What a learnable step launches beyond the constant-matrix step, from two traces of the same number of steps."""
    n = args.trace_steps + 2
    const, learn = (_trace(g, args.trace_steps, 2, args.batch) for g in ("full", "learn_full"))
    added = {}
    for k, (calls, ns) in learn.items():
        c0, n0 = const.get(k, (0, 0))
        if calls != c0:
            added[k] = {"extra_calls_per_step": (calls - c0) / n, "avg_us": ns / calls / 1e3,
                        "extra_us_per_step": (ns - n0) / n / 1e3}
    new = {k: v["avg_us"] for k, v in added.items() if k.startswith("comm_grad")}
    return {"steps_traced": n, "added_kernels": added,
            "added_launches_per_step": sum(v["extra_calls_per_step"] for v in added.values()),
            "added_us_per_step": sum(v["extra_us_per_step"] for v in added.values()),
            "new_kernels_avg_us": new, "new_kernels_estimate_us": 8.0,
            "torch_launches_us_per_step": sum(v["extra_us_per_step"] for k, v in added.items()
                                              if not k.startswith("comm_grad")),
            "kernel_us_per_step": {"const": sum(v[1] for v in const.values()) / n / 1e3,
                                   "learn": sum(v[1] for v in learn.values()) / n / 1e3}}


def grad_rounds(args) -> None:
    res = {"parent_full": []}
    res.update({g: [] for g in GRAD_LEGS})
    for rnd in range(args.rounds):
        res["parent_full"].append(leg("full", os.path.abspath(args.parent), args)["ms_per_step"])
        for g in GRAD_LEGS:
            res[g].append(leg(g, ROOT, args)["ms_per_step"])
        print(f"round {rnd}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in res.items()), flush=True)
    p = res["parent_full"]
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    summary = {"workload": "Trainer.train_step, bench.py C3 (RESISC45 dims, 16 agents, 16 steps), full(16) / ring(16)",
               "batch": args.batch, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
               "ms_per_step": res, "parent_spread_ms": max(p) - min(p), "parent_median_ms": med["parent_full"],
               "median_ms": med,
               "excess_over_parent_median_ms": {k: med[k] - med["parent_full"] for k in GRAD_LEGS}}
    summary["const_inside_parent_spread"] = min(p) <= med["full"] <= max(p)
    if args.trace:
        t = added_launches(args)
        summary["trace"] = t
        allowed = t["added_us_per_step"] / 1e3 + summary["parent_spread_ms"]
        summary["excess_vs_added_launches"] = {
            k: {"excess_ms": summary["excess_over_parent_median_ms"][k], "added_launches_plus_spread_ms": allowed,
                "explained": summary["excess_over_parent_median_ms"][k] <= allowed}
            for k in ("learn_full", "learn_ring")}
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


def range_rounds(args) -> None:
    res = {"parent_full": []}
    res.update({g: [] for g in RANGE_LEGS})
    for rnd in range(args.rounds):
        res["parent_full"].append(leg("full", os.path.abspath(args.parent), args)["ms_per_step"])
        for g in RANGE_LEGS:
            res[g].append(leg(g, ROOT, args)["ms_per_step"])
        print(f"round {rnd}: " + ", ".join(f"{k} {v[-1]:.3f} ms" for k, v in res.items()), flush=True)
    p = res["parent_full"]
    med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
    summary = {"workload": "Trainer.train_step, bench.py C3 (RESISC45 dims, 16 agents, 16 steps), full(16) / ring(16) "
                           f"under set_comm_range({args.range})",
               "radius": args.range, "batch": args.batch, "steps": args.steps, "warmup": args.warmup,
               "rounds": args.rounds, "ms_per_step": res, "parent_spread_ms": max(p) - min(p),
               "parent_median_ms": med["parent_full"], "median_ms": med,
               "excess_over_parent_median_ms": {k: med[k] - med["parent_full"] for k in RANGE_LEGS}}
    summary["const_inside_parent_spread"] = min(p) <= med["full"] <= max(p)
    summary["gated_inside_parent_spread"] = {
        k: summary["excess_over_parent_median_ms"][k] <= summary["parent_spread_ms"] for k in RANGE_LEGS[1:]}
    print(json.dumps(summary))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
