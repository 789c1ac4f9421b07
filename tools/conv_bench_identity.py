#!/usr/bin/env python3
"""The GPU half of the identity evidence of DESIGN.md 8.22: another build of the library (the parent commit's) against the
tree's on one GPU, at bench.py's c3 and c4 (AidCnn) configurations.

    python tools/conv_bench_identity.py outputs|launches|timing [ROUNDS] --parent-lib PATH --out DIR

outputs: sha-256 of every array of `bench.py --dump-outputs`; launches: the ordered (kernel, grid, workgroup, LDS) list of
one `rocprofv3 --kernel-trace` run each (no counters), cnn_dgrad_kernel under one name; timing: bench.py alternating
between the two libraries.  One child process at a time, each under its own time limit; the first failure ends the job.
Results: DIR/bench_identity_<mode>.json (tools/conv_plan_identity.py holds the host half)."""
import argparse
import csv
import glob
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("mode", choices=["outputs", "launches", "timing"])
ap.add_argument("rounds", nargs="?", type=int, default=3)
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--out", required=True, help="directory for the result and the logs of every child process")
args = ap.parse_args()
OUT = os.path.abspath(args.out)
LIBS = {"parent": os.path.abspath(args.parent_lib),
        "tree": os.path.join(ROOT, "marlclassification_amd", "csrc", "libmarl_hip.so")}
CONFIGS = ("c3", "c4")
res = {"outputs": {}, "launches": {}, "timing": {}}


def save():
    with open(os.path.join(OUT, f"bench_identity_{mode}.json"), "w") as fh:
        json.dump(res, fh, indent=1)


def run(tag, cmd, lib, limit):
    log = os.path.join(OUT, f"bi_{tag}.log")
    with open(log, "w") as fh:
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, stdout=fh, stderr=subprocess.STDOUT,
                            env=dict(os.environ, MARL_LIB_PATH=LIBS[lib])).returncode
    print(tag, "rc", rc, flush=True)
    if rc != 0:
        res["failed"] = {"tag": tag, "rc": rc}
        save()
        sys.exit(1)
    return open(log).read()


def bench_line(text):
    for ln in reversed(text.splitlines()):
        if ln.startswith("{") and '"metric"' in ln:
            return json.loads(ln)
    raise SystemExit("no result line")


os.makedirs(OUT, exist_ok=True)
mode = args.mode
if mode == "outputs":
    for cfg in CONFIGS:
        for lib in LIBS:
            d = os.path.join("/tmp", f"bi_dump_{lib}_{cfg}")
            shutil.rmtree(d, ignore_errors=True)
            run(f"dump_{lib}_{cfg}", [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2",
                                      "--config", cfg, "--dump-outputs", d], lib, 240)
            res["outputs"].setdefault(cfg, {})[lib] = {
                os.path.basename(f): hashlib.sha256(open(f, "rb").read()).hexdigest() for f in sorted(glob.glob(d + "/*.npy"))}
            shutil.rmtree(d, ignore_errors=True)
        o = res["outputs"][cfg]
        o["arrays"] = len(o["parent"])
        o["identical"] = o["parent"] == o["tree"] and o["arrays"] > 0
        save()
elif mode == "launches":
    for cfg in CONFIGS:
        lists = {}
        for lib in LIBS:
            d = os.path.join("/tmp", f"bi_trace_{lib}_{cfg}")
            shutil.rmtree(d, ignore_errors=True)
            run(f"trace_{lib}_{cfg}", ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
                                       sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                                       "--config", cfg], lib, 300)
            files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
            rows = list(csv.DictReader(open(files[0])))
            rows.sort(key=lambda r: int(r["Dispatch_Id"]))
            res["launches"]["csv_columns"] = list(rows[0].keys())
            lds_cols = [k for k in rows[0] if "LDS" in k.upper() or "SHARED" in k.upper() or "GROUP_SEG" in k.upper()]
            lists[lib] = [[re.sub(r"(void )?marl::cnn_dgrad_kernel(<false>)?", "marl::cnn_dgrad_kernel", r["Kernel_Name"]),
                           [int(r[f"Grid_Size_{a}"]) for a in "XYZ"], [int(r[f"Workgroup_Size_{a}"]) for a in "XYZ"],
                           [int(r[k]) for k in lds_cols]] for r in rows]
            shutil.rmtree(d, ignore_errors=True)
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(lists["parent"], lists["tree"])) if a != b]
        conv = [x for x in lists["tree"] if "cnn_" in x[0]]
        res["launches"][cfg] = {
            "lds_columns": lds_cols,
            "dispatches_parent": len(lists["parent"]), "dispatches_tree": len(lists["tree"]),
            "identical": not diff and len(lists["parent"]) == len(lists["tree"]), "first_differences": diff[:10],
            "sha256_tree": hashlib.sha256(json.dumps(lists["tree"]).encode()).hexdigest(),
            "conv_launches_of_the_tree": [list(x) for x in {json.dumps(c): c for c in conv}.values()]}
        save()
elif mode == "timing":
    rounds = args.rounds
    for cfg in CONFIGS:
        t = {"parent": [], "tree": []}
        for r in range(rounds):
            for lib in LIBS:
                line = bench_line(run(f"time_{lib}_{cfg}_{r}", [sys.executable, "bench.py", "--gpus", "1", "--steps", "200",
                                                                 "--warmup", "20", "--config", cfg], lib, 240))
                t[lib].append(line["ms_per_step"])
        med = {k: sorted(v)[len(v) // 2] for k, v in t.items()}
        spread = round(max(abs(a - b) for a, b in zip(t["parent"], t["parent"][1:])), 6)
        res["timing"][cfg] = {"ms_per_step_runs_in_order": t, "median_parent": med["parent"], "median_tree": med["tree"],
                              "parent_largest_round_to_round_difference": spread,
                              # (bench.py prints three decimals: compare at that precision, not in binary fractions)
                              "tree_within_parent_spread": round(med["tree"] - med["parent"], 6) <= round(spread, 6)}
        save()
print(json.dumps(res)[:3000])
