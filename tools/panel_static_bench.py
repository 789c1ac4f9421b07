"""bench.py with this tree's library against bench.py with the PARENT commit's library for the static-shape panel kernels
(``marl_plan_query`` key ``panel_static``): timing, outputs, kernel traces, phase timestamps.

    python tools/panel_static_bench.py (--parent DIR | --parent-lib PATH) [--rounds 3] [--steps 100] [--warmup 10]
                                       [--ts-lib PATH] [--no-trace] [--out profiles/panel_static_c3.json]

``--parent DIR`` is a built checkout of the parent commit; ``--parent-lib PATH`` its libmarl_hip.so alone, loaded into
this tree's Python through MARL_LIB_PATH (this change touches no Python on the benchmark's path).  Every leg is a fresh
child process running ``bench.py --gpus 1`` (the legs, the child runner and the trace reader are
tools/panel_sample_bench.py's):
  * ``rounds`` x (parent, this tree) at C3, alternating on one box; this tree once more under MARL_PANEL_STATIC=0;
  * --rollout-only, --graph, --config c4, --config c5 once each; --config c2 (run-time-shape panels) ``rounds`` times;
  * ``--dump-outputs`` of both, compared array by array (np.array_equal);
  * one ``rocprofv3 --kernel-trace --stats`` run of each: the panel_fwd / panel_bwd lines;
  * ``--ts-lib PATH`` (this tree's library built with EXTRA=-DMARL_KERNEL_TS): phase timestamps of the panel launches,
    static and under MARL_PANEL_STATIC=0.
Accepted when every C3 run of this tree is faster than every parent run, the difference of medians is at least three
times the spread of the parent's own runs and at least half of what the trace says the panel launches saved per
iteration, all dumped arrays are equal, and both flagship launches are faster per launch than the parent's."""
import argparse
import glob
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from panel_sample_bench import ROOT, bench, med, trace  # noqa: E402


LIMIT = ["timeout", "-k", "10", "300"]  # every GPU leg under its own time limit; a failed leg ends the run


def main():
    ap = argparse.ArgumentParser()
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--parent", help="checkout of the parent commit (built)")
    g.add_argument("--parent-lib", help="libmarl_hip.so of the parent commit (run from this tree's Python)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ts-lib", default=None, help="libmarl_hip.so of this tree built with EXTRA=-DMARL_KERNEL_TS")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ptree = os.path.abspath(args.parent) if args.parent else ROOT
    penv = {} if args.parent else {"MARL_LIB_PATH": os.path.abspath(args.parent_lib)}
    legs = (("parent", ptree, penv), ("this", ROOT, {}))
    res = {"workload": "bench.py --gpus 1 (C3: RESISC45 dims, 16 agents, 16 steps, 256 images)", "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds,
           "parent": "checkout" if args.parent else "library through MARL_LIB_PATH"}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    def run(leg, extra=(), env=None):
        return bench(leg[1], args, extra, env=dict(leg[2], **(env or {})), prefix=LIMIT)[0]

    ms = {"parent": [], "this": []}
    for rnd in range(args.rounds):
        for leg in legs:
            ms[leg[0]].append(run(leg)["ms_per_step"])
        print(f"round {rnd}: parent {ms['parent'][-1]:.3f} ms, this tree {ms['this'][-1]:.3f} ms", flush=True)
    spread = max(ms["parent"]) - min(ms["parent"])
    gain = med(ms["parent"]) - med(ms["this"])
    res["c3_ms_per_step"] = ms
    res["c3"] = {"parent_median_ms": med(ms["parent"]), "median_ms": med(ms["this"]), "parent_spread_ms": spread,
                 "spread_ms": max(ms["this"]) - min(ms["this"]), "gain_ms": gain,
                 "every_run_faster_than_every_parent_run": max(ms["this"]) < min(ms["parent"]),
                 "gain_at_least_3x_parent_spread": gain >= 3 * spread,
                 "runtime_form_ms": run(legs[1], env={"MARL_PANEL_STATIC": "0"})["ms_per_step"]}
    save()

    other = {}
    for tag, extra in (("rollout_only", ["--rollout-only"]), ("graph", ["--graph"]), ("c4", ["--config", "c4"]),
                       ("c5", ["--config", "c5"])):
        other[tag] = {leg[0]: run(leg, extra)["ms_per_step"] for leg in legs}
        print(f"{tag}: {other[tag]}", flush=True)
    c2 = {"parent": [], "this": []}
    for rnd in range(args.rounds):
        for leg in legs:
            c2[leg[0]].append(run(leg, ["--config", "c2"])["ms_per_step"])
    other["c2"] = dict(c2, parent_spread_ms=max(c2["parent"]) - min(c2["parent"]),
                       median_difference_ms=med(c2["this"]) - med(c2["parent"]))
    print(f"c2: {other['c2']}", flush=True)
    res["other_ms_per_step"] = other
    save()

    dumps = {}
    with tempfile.TemporaryDirectory() as dp, tempfile.TemporaryDirectory() as dt:
        run(legs[0], ["--dump-outputs", dp])
        run(legs[1], ["--dump-outputs", dt])
        names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(dp, "*.npy")))
        assert names == sorted(os.path.basename(f) for f in glob.glob(os.path.join(dt, "*.npy"))), names
        for n in names:
            a, b = np.load(os.path.join(dp, n)), np.load(os.path.join(dt, n))
            dumps[n] = bool(a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b))
    res["dump_outputs_equal"] = dumps
    res["dump_outputs_all_equal"] = bool(dumps) and all(dumps.values())
    print(f"dump-outputs: {dumps}", flush=True)
    save()

    if not args.no_trace:
        kt = {leg[0]: trace(leg[1], args, match=("panel_fwd", "panel_bwd"), env=leg[2]) for leg in legs}
        res["kernel_trace"] = kt
        iters = 25  # (trace(): 20 steps + 5 warm-up iterations)

        def per_iter(t):
            return sum(v["total_ms"] for k, v in t.items() if isinstance(v, dict)) / iters

        def flagship(t, what):  # the launch with the most calls of that direction
            c = [v for k, v in t.items() if isinstance(v, dict) and what in k]
            return max(c, key=lambda v: v["calls"])["avg_us"] if c else None

        saved = per_iter(kt["parent"]) - per_iter(kt["this"])
        res["c3"].update(panel_ms_per_iteration={"parent": per_iter(kt["parent"]), "this": per_iter(kt["this"])},
                         trace_saved_ms_per_iteration=saved, gain_at_least_half_of_trace_saving=gain >= 0.5 * saved,
                         flagship_fwd_us={k: flagship(kt[k], "panel_fwd") for k in kt},
                         flagship_bwd_us={k: flagship(kt[k], "panel_bwd") for k in kt})
        res["c3"]["both_flagship_launches_faster"] = bool(
            res["c3"]["flagship_fwd_us"]["this"] < res["c3"]["flagship_fwd_us"]["parent"] and
            res["c3"]["flagship_bwd_us"]["this"] < res["c3"]["flagship_bwd_us"]["parent"])
        print(json.dumps(kt), flush=True)
        save()

    if args.ts_lib:
        targs = argparse.Namespace(steps=5, warmup=3)
        ts = {}
        for tag, env in (("static", {}), ("runtime_form", {"MARL_PANEL_STATIC": "0"})):
            _, err = bench(ROOT, targs, [], env=dict(env, MARL_LIB_PATH=os.path.abspath(args.ts_lib)), prefix=LIMIT)
            ts[tag] = [ln for ln in err.splitlines() if ln.startswith("[ts] panel_")]
        res["phase_timestamps"] = {"unit": "10 ns ticks between consecutive stamps; start / end in us on the clock of role 0, wave 0",
                                   **ts}
        save()
    c = res["c3"]
    c["accepted"] = bool(c["every_run_faster_than_every_parent_run"] and c["gain_at_least_3x_parent_spread"] and
                         res["dump_outputs_all_equal"] and c.get("gain_at_least_half_of_trace_saving", False) and
                         c.get("both_flagship_launches_faster", False))
    save()
    print(json.dumps(c))


if __name__ == "__main__":
    main()
