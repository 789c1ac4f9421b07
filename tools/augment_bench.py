"""Cost of the augmenting batch gather (``marl_batch_augment``, ``augment.apply``) against the ``index_select`` it
replaces, and the unchanged path against ANOTHER checkout (the parent commit, built), on one box:

    python tools/augment_bench.py [--parent DIR] [--rounds 3] [--launches 50] [--trace] [--out profiles/augment_c3.json]

  * the kernel: per case (C3 uint8 B = 256, C3 fp32 B = 256, AID uint8 B = 32) HIP events around ``launches`` launches,
    ``rounds`` alternating rounds of: ``x.index_select(0, rows)``, the kernel with ``ops = NULL``, under hflip only,
    under a quarter turn (a transposing code), and under a full random ``d4,shift:8,erase:32`` draw.  The resident set
    is larger than the 256 MB Infinity Cache, rows are random over it, and rows / ops / destinations rotate over
    ``ROTATE`` buffers, so the figures are HBM figures.  Per class: every time, the median, its fraction of the 6.29 TB/s
    a float4 copy reaches, and the spread of the ``index_select`` rounds;
  * ``--parent DIR``: ``rounds`` x (parent, this tree) ``bench.py --gpus 1``, every leg a fresh child process, and
    ``--dump-outputs`` of both trees compared array by array;
  * ``--trace``: one ``rocprofv3 --kernel-trace --stats`` run of its own over the kernel legs (``--leg`` is the child's
    entry): the durations of the ``batch_augment_kernel`` instantiations and of torch's gather kernel."""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_TBS = 6.29  # what a float4 copy reaches on this part
ROTATE = 6
# name -> (dtype, images in the resident set, batch, [C, H, W])
CASES = {
    "c3_u8_b256": ("uint8", 4096, 256, (3, 256, 256)),
    "c3_f32_b256": ("float32", 1024, 256, (3, 256, 256)),
    "aid_u8_b32": ("uint8", 800, 32, (3, 600, 600)),
}
CLASSES = ("index_select", "ops_null", "hflip", "quarter_turn", "d4_shift8_erase32")


def med(v):
    return sorted(v)[len(v) // 2]


# ---- the child: the kernel legs -------------------------------------------------------------------------------------
def leg(rounds, launches, cases):
    sys.path.insert(0, ROOT)
    import torch as th

    from marlclassification_amd import augment

    dev = th.device("cuda", 0)
    out = {}
    for name in cases:
        dtype_name, n_set, batch, shape = CASES[name]
        dtype = getattr(th, dtype_name)
        if dtype == th.uint8:
            x = th.randint(0, 256, (n_set,) + shape, dtype=th.uint8, device=dev)
        else:
            x = th.rand((n_set,) + shape, device=dev)
        g = th.Generator(device=dev).manual_seed(1)
        rows = [th.randint(0, n_set, (batch,), generator=g, device=dev) for _ in range(ROTATE)]
        dst = [th.empty((batch,) + shape, dtype=dtype, device=dev) for _ in range(ROTATE)]
        full = augment.parse("d4,shift:8,erase:32")

        def const(code):
            ops = th.zeros(batch, 8, dtype=th.int32, device=dev)
            ops[:, 0] = code
            return [ops] * ROTATE

        ops = {"ops_null": [None] * ROTATE, "hflip": const(2), "quarter_turn": const(3),
               "d4_shift8_erase32": [full.draw(batch, g, size=shape[1:]) for _ in range(ROTATE)]}
        nbytes = 2 * batch * x[0].numel() * x.element_size()

        def run(cls, k):
            if cls == "index_select":
                th.index_select(x, 0, rows[k], out=dst[k])
            else:
                augment.apply(x, rows[k], ops[cls][k], out=dst[k])

        times = {cls: [] for cls in CLASSES}
        for cls in CLASSES:  # warm-up, and one equality check of the plain gather
            for k in range(ROTATE):
                run(cls, k)
        assert th.equal(augment.apply(x, rows[0]), x.index_select(0, rows[0]))
        for _ in range(rounds):
            for cls in CLASSES:
                start, end = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                th.cuda.synchronize(dev)
                start.record()
                for i in range(launches):
                    run(cls, i % ROTATE)
                end.record()
                end.synchronize()
                times[cls].append(round(1e3 * start.elapsed_time(end) / launches, 3))
        res = {"bytes_per_launch": nbytes, "estimate_us_at_6.29_TBs": round(nbytes / COPY_TBS / 1e6, 2),
               "resident_set_mb": round(x.numel() * x.element_size() / 1e6, 1), "us_per_launch": times,
               "plan": augment.plan(x, dst[0])}
        res["median_us"] = {cls: med(v) for cls, v in times.items()}
        res["fraction_of_6.29_TBs"] = {cls: round(nbytes / (med(v) * 1e-6) / (COPY_TBS * 1e12), 3)
                                        for cls, v in times.items()}
        sel = times["index_select"]
        res["index_select_spread_us"] = round(max(sel) - min(sel), 3)
        res["ops_null_inside_index_select_spread"] = min(sel) <= med(times["ops_null"]) <= max(sel)
        res["ops_null_not_slower_than_index_select_max"] = med(times["ops_null"]) <= max(sel)
        res["quarter_turn_over_ops_null"] = round(med(times["quarter_turn"]) / med(times["ops_null"]), 3)
        out[name] = res
        del x, dst
        th.cuda.empty_cache()
    print(json.dumps(out))


# ---- the parent process ---------------------------------------------------------------------------------------------
def run(cmd, tree, prefix=(), timeout=900):
    r = subprocess.run(list(prefix) + [sys.executable] + cmd, cwd=tree, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} in {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-3000:]}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]) if lines else {}


def trace(args):
    import sqlite3

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from rocpd_stats import short

    d = tempfile.mkdtemp(prefix="augment_trace_")
    run([os.path.abspath(__file__), "--leg", args.cases, "--rounds", "1", "--launches", "20"], ROOT,
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
        if "batch_augment" in n or "index" in n.lower() or "gather" in n.lower():
            a = agg.setdefault(n, [0, 0, None, 0])
            a[0] += 1
            a[1] += dur
            a[2] = dur if a[2] is None else min(a[2], dur)
            a[3] = max(a[3], dur)
    return {k: {"calls": c, "avg_us": round(ns / c / 1e3, 3), "min_us": round(lo / 1e3, 3), "max_us": round(hi / 1e3, 3)}
            for k, (c, ns, lo, hi) in sorted(agg.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit (built): bench.py alternation")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) comma-separated cases")
    args = ap.parse_args()
    if args.leg:
        leg(args.rounds, args.launches, args.leg.split(","))
        return
    res = {"rounds": args.rounds, "launches_per_timing": args.launches, "rotate": ROTATE}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    me = os.path.abspath(__file__)
    res["kernel"] = run([me, "--leg", args.cases, "--rounds", str(args.rounds), "--launches", str(args.launches)], ROOT)
    for name, r in res["kernel"].items():
        print(f"{name}: " + ", ".join(f"{k} {v} us" for k, v in r["median_us"].items()), flush=True)
    save()
    if args.parent:
        import numpy as np

        parent = os.path.abspath(args.parent)
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
    if args.trace:
        res["kernel_trace"] = trace(args)
        print(json.dumps(res["kernel_trace"]), flush=True)
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
