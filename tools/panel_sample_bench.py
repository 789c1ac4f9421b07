"""bench.py of this tree against bench.py of ANOTHER checkout (the parent commit, built) for the sampling epilogue of the
chained panel launch (``marl_plan_query`` key ``panel_sample``): timing, outputs, kernel traces, role timestamps.

    python tools/panel_sample_bench.py --parent DIR [--rounds 3] [--steps 100] [--warmup 10]
                                       [--ts-lib PATH] [--out profiles/panel_sample_c3.json]

Every leg is a fresh child process running ``bench.py --gpus 1`` with its tree as working directory:
  * ``rounds`` x (parent, this tree) at C3, alternating on one box; then --rollout-only, --graph and --config c2 / c4 / c5 once each;
  * ``--dump-outputs`` of both trees, compared array by array (np.array_equal);
  * one ``rocprofv3 --kernel-trace --stats`` run of each tree: the sample_kernel / panel_fwd_kernel lines;
  * ``--ts-lib PATH`` (a libmarl_hip.so built with EXTRA=-DMARL_KERNEL_TS): phase timestamps of both roles of one chain
    launch, with the epilogue and with MARL_PANEL_SAMPLE=0.
Accepted when every C3 run of this tree is faster than every parent run and the difference of medians is at least three
times the spread of the parent's own runs."""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(tree, args, extra=(), env=None, prefix=()):
    cmd = list(prefix) + [sys.executable, "bench.py", "--gpus", "1", "--steps", str(args.steps), "--warmup",
                          str(args.warmup)] + list(extra)
    r = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=900, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        raise SystemExit(f"bench.py {' '.join(extra)} in {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-3000:]}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return (json.loads(lines[-1]) if lines else {}), r.stderr


def med(v):
    return sorted(v)[len(v) // 2]


def trace(tree, args, match=("sample_kernel", "panel_fwd_kernel"), env=None):
    """Kernel trace of one bench.py run (a run of its own): {short kernel name: {calls, avg_us, total_ms}} of the
    kernels this change touches (names containing one of `match`), and the kernel time of everything."""
    import sqlite3

    from rocpd_stats import short

    d = tempfile.mkdtemp(prefix="panel_sample_trace_")
    targs = argparse.Namespace(steps=20, warmup=5)
    bench(tree, targs, env=dict(env or {}, TMPDIR="/tmp"), prefix=["timeout", "-k", "10", "600", "rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "r", "--"])
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    if not dbs:
        raise SystemExit(f"no trace database under {d}")
    db = sqlite3.connect(dbs[0])
    cols = [row[1] for row in db.execute("pragma table_info(kernels)")]
    namecol = "name" if "name" in cols else "kernel_name"
    agg, total = {}, 0
    for n, dur in db.execute(f"select {namecol}, (end - start) from kernels"):
        total += dur
        n = short(n)
        if any(m in n for m in match):
            a = agg.setdefault(n, [0, 0])
            a[0] += 1
            a[1] += dur
    out = {k: {"calls": c, "avg_us": ns / c / 1e3, "total_ms": ns / 1e6} for k, (c, ns) in agg.items()}
    out["all_kernels_ms_per_iteration"] = total / 1e6 / (targs.steps + targs.warmup)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="checkout of the parent commit (built)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ts-lib", default=None, help="libmarl_hip.so of this tree built with EXTRA=-DMARL_KERNEL_TS")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parent = os.path.abspath(args.parent)
    res = {"workload": "bench.py --gpus 1 (C3: RESISC45 dims, 16 agents, 16 steps, 256 images)", "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    ms = {"parent": [], "this": []}
    for rnd in range(args.rounds):
        for who, tree in (("parent", parent), ("this", ROOT)):
            ms[who].append(bench(tree, args)[0]["ms_per_step"])
        print(f"round {rnd}: parent {ms['parent'][-1]:.3f} ms, this tree {ms['this'][-1]:.3f} ms", flush=True)
    spread = max(ms["parent"]) - min(ms["parent"])
    gain = med(ms["parent"]) - med(ms["this"])
    res["c3_ms_per_step"] = ms
    res["c3"] = {"parent_median_ms": med(ms["parent"]), "median_ms": med(ms["this"]), "parent_spread_ms": spread,
                 "spread_ms": max(ms["this"]) - min(ms["this"]), "gain_ms": gain,
                 "every_run_faster_than_every_parent_run": max(ms["this"]) < min(ms["parent"]),
                 "gain_at_least_3x_parent_spread": gain >= 3 * spread}
    res["c3"]["accepted"] = bool(res["c3"]["every_run_faster_than_every_parent_run"] and
                                 res["c3"]["gain_at_least_3x_parent_spread"])
    save()

    other = {}
    for tag, extra in (("rollout_only", ["--rollout-only"]), ("graph", ["--graph"]), ("c2", ["--config", "c2"]),
                       ("c4", ["--config", "c4"]), ("c5", ["--config", "c5"])):
        other[tag] = {who: bench(tree, args, extra)[0]["ms_per_step"] for who, tree in (("parent", parent), ("this", ROOT))}
        print(f"{tag}: {other[tag]}", flush=True)
    res["other_ms_per_step"] = other
    save()

    dumps = {}
    with tempfile.TemporaryDirectory() as dp, tempfile.TemporaryDirectory() as dt:
        bench(parent, args, ["--dump-outputs", dp])
        bench(ROOT, args, ["--dump-outputs", dt])
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
        res["kernel_trace"] = {"parent": trace(parent, args), "this": trace(ROOT, args)}
        sk = [v for k, v in res["kernel_trace"]["parent"].items() if "sample_kernel" in k]
        if sk:
            per_iter = 16 * sum(v["total_ms"] for v in sk) / sum(v["calls"] for v in sk)
            res["c3"]["parent_sample_kernel_ms_per_iteration"] = per_iter
            res["c3"]["gain_at_least_half_of_removed_launches"] = gain >= 0.5 * per_iter
        print(json.dumps(res["kernel_trace"]), flush=True)
        save()

    if args.ts_lib:
        targs = argparse.Namespace(steps=5, warmup=3)
        ts = {}
        for tag, env in (("epilogue", {}), ("separate_launch", {"MARL_PANEL_SAMPLE": "0"})):
            _, err = bench(ROOT, targs, ["--rollout-only"], env=dict(env, MARL_LIB_PATH=os.path.abspath(args.ts_lib)))
            ts[tag] = [ln for ln in err.splitlines() if ln.startswith("[ts] panel_fwd")]
        res["role_timestamps"] = {"unit": "10 ns ticks between consecutive stamps; start / end in us on the clock of role 0, wave 0",
                                  **ts}
        print(json.dumps(ts, indent=1), flush=True)
        save()
    print(json.dumps(res["c3"]))


if __name__ == "__main__":
    main()
