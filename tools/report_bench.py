#!/usr/bin/env python
"""Times the episode report at C3 (Ns = 16, Na = 16, Nb = 256, nC = 45) and writes profiles/report_c3.json.

    python tools/report_bench.py [--parent TREE] [--out FILE] [--rounds N] [--skip-iterations] [--skip-dump]
    python tools/report_bench.py --probe        (50 calls of either per-call arm: the workload of a kernel trace)

Per call: one ``EpisodeReport.add`` (windowed, accumulate = 0: what the trainer's meter does) against the five-launch
``ConfusionMeter.add`` sequence it replaces there, both in one process, alternating round by round.  A figure is the
wall-clock time of a window of CALLS eager calls with one synchronise behind it, divided by CALLS - what a training
loop pays per iteration, the larger of the host's enqueue time and the device's run time - and, for the report alone,
the device time between two events around the same window.  The traffic bound is Ns * Na * Nb * nC * 4 bytes over the
8.0 TB/s HBM peak.

Per iteration: ``Trainer.train_step`` without and with ``report``, and - ``--parent TREE``, a built checkout of the
parent commit - the parent's ``train_step`` in a worker process of its own, taking turns.  With ``--parent`` also
``bench.py --dump-outputs`` of both trees, whose arrays must be identical.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3 = dict(ft_extr="resisc45", window=12, n_b=256, n_a=256, n_m=64, n_m_o=96, n_d=16, nb_class=45, nlb=384, nla=384)
NA, NS, NB, IMG, GAMMA, LR = 16, 16, 256, (3, 256, 256), 0.99, 1e-4
ACTIONS = [[1, 0], [-1, 0], [0, 1], [0, -1]]
CALLS = 200     # calls per timed window of the per-call arms
ITERS = 10      # iterations per timed window of the train_step arms
HBM_PEAK = 8.0e12


class Worker:
    def __init__(self, tree: str) -> None:
        sys.path.insert(0, tree)
        import torch as th

        self.th = th
        self.dev = th.device("cuda:0")
        self.arms = {}

    def arm(self, name: str):
        if name in self.arms:
            return self.arms[name]
        th = self.th
        gen = th.Generator(device=self.dev).manual_seed(0)
        if name in ("add", "meter"):
            preds = th.randn(NS, NA, NB, C3["nb_class"], device=self.dev, generator=gen)
            y = th.randint(0, C3["nb_class"], (NB,), device=self.dev, generator=gen)
            if name == "add":
                from marlclassification_amd.report import EpisodeReport, ReportOptions

                rep = EpisodeReport(NS, NA, C3["nb_class"], ReportOptions(exit_thresholds=(0.5, 0.9)), self.dev,
                                    window_size=64)
                fn = lambda: rep.add(preds, y)  # noqa: E731
            else:
                from marlclassification_amd.metrics import ConfusionMeter

                meter = ConfusionMeter(C3["nb_class"], window_size=64)
                fn = lambda: meter.add(preds[-1].mean(dim=0), y)  # noqa: E731
        else:
            from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
            from marlclassification_amd.networks import ModelsWrapper
            from marlclassification_amd.networks.vision import CNN_BY_NAME
            from marlclassification_amd.training import Trainer

            th.manual_seed(0)
            model = ModelsWrapper(CNN_BY_NAME[C3["ft_extr"]](C3["window"]), C3["n_b"], C3["n_a"], C3["n_m"],
                                  C3["n_m_o"], C3["n_d"], 2, len(ACTIONS), C3["nb_class"], C3["nlb"],
                                  C3["nla"]).to(self.dev)
            img = th.rand(NB, *IMG, device=self.dev, generator=gen)
            y = th.randint(0, C3["nb_class"], (NB,), device=self.dev, generator=gen)
            sampler = EpisodeSampler(MultiAgent(NA, model), Environment(ACTIONS, C3["window"]), NS)
            kw = {}
            if name == "step_report":
                from marlclassification_amd.report import ReportOptions

                kw["report"] = ReportOptions(exit_thresholds=(0.5, 0.9))
            trainer = Trainer(model, C3["nb_class"], LR, GAMMA, **kw)
            if name == "step_report":
                fn = lambda: trainer.train_step(img, y, sampler)  # noqa: E731
            else:  # (the parent's iteration: the step and the confusion meter train_epoch feeds behind it)
                from marlclassification_amd.metrics import ConfusionMeter

                meter = ConfusionMeter(C3["nb_class"], window_size=64)

                def fn():
                    out, _ = trainer.train_step(img, y, sampler)
                    meter.add(out.step_preds[-1].mean(dim=0), y)
        for _ in range(3):
            fn()
        th.cuda.synchronize()
        self.arms[name] = fn
        return fn

    def time_arm(self, name: str, n: int) -> dict:
        th = self.th
        fn = self.arm(name)
        a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        th.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        th.cuda.synchronize()
        wall = (time.perf_counter() - t0) / n
        return {"wall_us": wall * 1e6, "device_us": a.elapsed_time(b) * 1e3 / n}


def worker_main(tree: str) -> None:
    w = Worker(tree)
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        print(json.dumps(w.time_arm(cmd[1], int(cmd[2]))), flush=True)


class Child:
    """The orchestrator never opens the GPU itself: every tree runs in a worker process of its own."""

    def __init__(self, tree: str) -> None:
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MARL_LIB_PATH"):
            env.pop(k, None)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, env=env, cwd=tree)
        self.ask(None)

    def ask(self, line):
        if line is not None:
            self.p.stdin.write(line + "\n")
            self.p.stdin.flush()
        while True:
            out = self.p.stdout.readline()
            if not out:
                raise SystemExit(f"worker died (exit {self.p.poll()})")
            if out.startswith("{"):
                return json.loads(out)

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=60)


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "spread": max(xs) - min(xs),
            "rounds": len(xs)}


def dump_identical(parent: str, steps: int = 2) -> dict:
    """bench.py --dump-outputs of both trees: every array must be identical."""
    import numpy as np

    dirs = {}
    for tag, tree in (("this", ROOT), ("parent", parent)):
        d = tempfile.mkdtemp(prefix=f"report_bench_{tag}_")
        subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--no-cpu-baseline", "--dump-outputs", d], cwd=tree, check=True, stdout=subprocess.DEVNULL)
        dirs[tag] = d
    names = sorted(f for f in os.listdir(dirs["this"]) if f.endswith(".npy"))
    assert names and names == sorted(f for f in os.listdir(dirs["parent"]) if f.endswith(".npy")), names
    differing = [n for n in names if not np.array_equal(np.load(os.path.join(dirs["this"], n)),
                                                        np.load(os.path.join(dirs["parent"], n)), equal_nan=True)]
    return {"arrays": len(names), "differing": differing, "identical": not differing}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_c3.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--skip-iterations", action="store_true")
    ap.add_argument("--skip-dump", action="store_true")
    ap.add_argument("--probe", action="store_true",
                    help="50 calls of either per-call arm in this process and nothing else: the workload of a kernel trace")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker_main(args.worker)
        return
    if args.probe:  # (for a kernel trace: rocprofv3 --kernel-trace -- python tools/report_bench.py --probe)
        w = Worker(ROOT)
        for name in ("add", "meter"):
            print(name, w.time_arm(name, 50))
        return
    parent = os.path.abspath(args.parent) if args.parent else None
    nbytes = NS * NA * NB * C3["nb_class"] * 4
    result = {"shape": {"Ns": NS, "Na": NA, "Nb": NB, "nC": C3["nb_class"]}, "calls_per_window": CALLS,
              "step_preds_bytes": nbytes, "traffic_bound_us": nbytes / HBM_PEAK * 1e6,
              "traffic_bound_is": "Ns * Na * Nb * nC * 4 bytes over the 8.0 TB/s HBM peak"}
    new = Child(ROOT)
    old = Child(parent) if parent and not args.skip_iterations else None
    try:
        times = {"add": [], "meter": []}
        device = {"add": [], "meter": []}
        for r in range(args.rounds):
            for k in (("add", "meter") if r % 2 == 0 else ("meter", "add")):
                t = new.ask(f"time {k} {CALLS}")
                times[k].append(t["wall_us"])
                device[k].append(t["device_us"])
        result["per_call_wall_us"] = {"EpisodeReport.add (2 launches)": stats(times["add"]),
                                      "ConfusionMeter.add (5 launches)": stats(times["meter"])}
        result["per_call_event_us"] = {"EpisodeReport.add (2 launches)": stats(device["add"]),
                                       "ConfusionMeter.add (5 launches)": stats(device["meter"])}
        result["per_call_is"] = (f"a window of {CALLS} eager calls, one synchronise behind it, / {CALLS}: wall = host "
                                 "clock, event = device events around the window; both include the enqueue rate")
        result["add_over_traffic_bound"] = statistics.median(device["add"]) / result["traffic_bound_us"]
        result["add_slower_than_the_meter"] = statistics.median(times["add"]) > statistics.median(times["meter"])
        if not args.skip_iterations:
            arms = [(new, "step_plain", "train_step + ConfusionMeter.add"), (new, "step_report", "train_step(report)")]
            if old is not None:
                arms.insert(0, (old, "step_plain", "parent: train_step + ConfusionMeter.add"))
            it = {label: [] for _, _, label in arms}
            for r in range(args.rounds):
                for c, a, label in (arms if r % 2 == 0 else arms[::-1]):
                    it[label].append(c.ask(f"time {a} {ITERS}")["wall_us"] / 1e3)
            result["per_iteration_ms"] = {k: stats(v) for k, v in it.items()}
            result["iterations_per_window"] = ITERS
    finally:
        new.close()
        if old is not None:
            old.close()
    if parent and not args.skip_dump:
        result["bench_dump_outputs"] = dump_identical(parent)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
