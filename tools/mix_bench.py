"""Cost of the mixing batch gather (``marl_batch_mix``, ``mix.apply``) against this tree's unchanged
``marl_batch_augment`` on the same rows and ops, of a train step under soft targets, and the unchanged path against
ANOTHER checkout (the parent commit, built), on one box:

    python tools/mix_bench.py [--parent DIR] [--rounds 3] [--launches 50] [--trace] [--iteration]
                              [--out profiles/mix_c3.json]

  * the kernel: per case (C3 uint8 B = 256, C3 fp32 B = 256, AID uint8 B = 32) HIP events around ``launches`` launches,
    ``rounds`` alternating rounds of: ``augment.apply`` (the yardstick), ``mix.apply`` with ``mix = NULL``, under a
    CutMix draw for every image, under a Mixup draw for every image, both under the same ``hflip,shift:8`` ops; and a
    quarter turn (a transposing code, resolved per pixel under a mix) under ``augment.apply`` and under CutMix.  The
    resident set is larger than the 256 MB Infinity Cache, rows are random over it, and rows / ops / mix / destinations
    rotate over ``ROTATE`` buffers, so the figures are HBM figures.  Bars: CutMix 1.0 x, Mixup 1.5 x the yardstick's
    median, with the yardstick's own max - min over the rounds as the margin;
  * ``--iteration``: ``rounds`` x (parent plain, this tree plain, this tree under ``targets=Q`` of a CutMix draw)
    ``Trainer.train_step`` at C3, B = 256, every leg a fresh child process;
  * ``--parent DIR``: ``rounds`` x (parent, this tree) ``bench.py --gpus 1``, every leg a fresh child process, and
    ``--dump-outputs`` of both trees compared array by array;
  * ``--trace``: one ``rocprofv3 --kernel-trace --stats`` run of its own over the kernel legs: the durations of the
    ``batch_mix_kernel`` and ``batch_augment_kernel`` instantiations."""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COPY_TBS = 6.29  # what a float4 copy reaches on this part
ROTATE = 6
# name -> (dtype, images in the resident set, batch, [C, H, W])
CASES = {
    "c3_u8_b256": ("uint8", 4096, 256, (3, 256, 256)),
    "c3_f32_b256": ("float32", 1024, 256, (3, 256, 256)),
    "aid_u8_b32": ("uint8", 800, 32, (3, 600, 600)),
}
CLASSES = ("augment", "mix_null", "cutmix", "mixup", "augment_quarter_turn", "cutmix_quarter_turn")
BARS = {"cutmix": 1.0, "mixup": 1.5}


def med(v):
    return sorted(v)[len(v) // 2]


# ---- the child: the kernel legs -------------------------------------------------------------------------------------
def leg(rounds, launches, cases):
    sys.path.insert(0, ROOT)
    import torch as th

    from marlclassification_amd import augment, mix

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
        aug = augment.parse("hflip,shift:8")
        ops = [aug.draw(batch, g, size=shape[1:]) for _ in range(ROTATE)]
        turn = th.zeros(batch, 8, dtype=th.int32, device=dev)
        turn[:, 0] = 3
        draws = {"cutmix": [mix.parse("cutmix:1:1").draw(batch, g, shape[1:]) for _ in range(ROTATE)],
                 "mixup": [mix.parse("mixup:1:1").draw(batch, g, shape[1:]) for _ in range(ROTATE)]}
        nbytes = 2 * batch * x[0].numel() * x.element_size()

        def run(cls, k):
            if cls == "augment":
                augment.apply(x, rows[k], ops[k], out=dst[k])
            elif cls == "augment_quarter_turn":
                augment.apply(x, rows[k], turn, out=dst[k])
            elif cls == "mix_null":
                mix.apply(x, rows[k], ops[k], None, out=dst[k])
            elif cls == "cutmix_quarter_turn":
                mix.apply(x, rows[k], turn, draws["cutmix"][k], out=dst[k])
            else:
                mix.apply(x, rows[k], ops[k], draws[cls][k], out=dst[k])

        times = {cls: [] for cls in CLASSES}
        for cls in CLASSES:  # warm-up, and one equality check of the unmixed launch
            for k in range(ROTATE):
                run(cls, k)
        assert th.equal(mix.apply(x, rows[0], ops[0]), augment.apply(x, rows[0], ops[0]))
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
        res = {"bytes_per_launch_plain_gather": nbytes, "estimate_us_at_6.29_TBs": round(nbytes / COPY_TBS / 1e6, 2),
               "resident_set_mb": round(x.numel() * x.element_size() / 1e6, 1), "us_per_launch": times,
               "plan": mix.plan(x, dst[0])}
        res["median_us"] = {cls: med(v) for cls, v in times.items()}
        yard = times["augment"]
        margin = max(yard) - min(yard)
        res["yardstick_spread_us"] = round(margin, 3)
        res["over_yardstick"] = {cls: round(med(times[cls]) / med(yard), 3) for cls in ("mix_null", "cutmix", "mixup")}
        res["inside_bar"] = {cls: med(times[cls]) <= bar * med(yard) + margin for cls, bar in BARS.items()}
        res["excess_over_bar_us"] = {cls: round(max(0.0, med(times[cls]) - (bar * med(yard) + margin)), 3)
                                     for cls, bar in BARS.items()}
        res["cutmix_quarter_turn_over_augment_quarter_turn"] = round(
            med(times["cutmix_quarter_turn"]) / med(times["augment_quarter_turn"]), 3)
        lam = mix.label_weights(draws["cutmix"][0], *shape[1:])
        res["cutmix_mean_own_share"] = round(float(lam.mean()), 3)
        out[name] = res
        del x, dst
        th.cuda.empty_cache()
    print(json.dumps(out))


# ---- the child: one train-step leg ----------------------------------------------------------------------------------
def step_leg(tree, soft, steps, warmup):
    """``Trainer.train_step`` on bench.py's C3 workload (its model, sizes and seeds) of ``tree``; ``soft``: under the
    target distributions of a CutMix draw (this tree only)"""
    sys.path.insert(0, tree)
    os.chdir(tree)
    import bench
    import torch as th

    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import CNN_BY_NAME
    from marlclassification_amd.training import Trainer

    dev = th.device("cuda", 0)
    c, nb = bench.C3, 256
    actions = [[1, 0], [-1, 0], [0, 1], [0, -1]]
    th.manual_seed(0)
    model = ModelsWrapper(CNN_BY_NAME[c["ft_extr"]](c["window"]), c["n_b"], c["n_a"], c["n_m"], c["n_m_o"], c["n_d"], 2,
                          len(actions), c["nb_class"], c["nlb"], c["nla"]).to(dev)
    sampler = EpisodeSampler(MultiAgent(bench.NA, model), Environment(actions, c["window"]), bench.NS)
    trainer = Trainer(model, c["nb_class"], bench.LR, bench.GAMMA)
    gen = th.Generator(device=dev).manual_seed(0)
    img = th.rand(nb, *bench.IMG, device=dev, generator=gen)
    y = th.randint(0, c["nb_class"], (nb,), device=dev, generator=gen)
    kw = {}
    if soft:
        from marlclassification_amd import mix

        m = mix.parse("cutmix:1:1").draw(nb, gen, bench.IMG[1:])
        kw["targets"] = mix.soft_targets(y, m, *bench.IMG[1:], c["nb_class"])
    for _ in range(warmup):
        trainer.train_step(img, y, sampler, **kw)
    th.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        out, scalars = trainer.train_step(img, y, sampler, **kw)
    th.cuda.synchronize(dev)
    ms = 1e3 * (time.perf_counter() - t0) / steps
    assert bool(th.isfinite(scalars).all())
    print(json.dumps({"ms_per_step": round(ms, 4), "loss": float(scalars[0])}))


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

    d = tempfile.mkdtemp(prefix="mix_trace_")
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
        if "batch_mix" in n or "batch_augment" in n:
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
    ap.add_argument("--iteration", action="store_true", help="Trainer.train_step legs (with --parent: its plain leg too)")
    ap.add_argument("--iteration-steps", type=int, default=30)
    ap.add_argument("--no-bench", action="store_true", help="with --parent: skip the bench.py alternation")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) comma-separated cases")
    ap.add_argument("--step-leg", default=None, metavar="TREE", help="(child) one train-step leg of the tree")
    ap.add_argument("--soft", action="store_true", help="(child) the train-step leg runs under targets=Q")
    args = ap.parse_args()
    if args.leg:
        leg(args.rounds, args.launches, args.leg.split(","))
        return
    if args.step_leg:
        step_leg(args.step_leg, args.soft, args.iteration_steps, 5)
        return
    res = {"rounds": args.rounds, "launches_per_timing": args.launches, "rotate": ROTATE}
    if args.out and os.path.exists(args.out):  # (sections measured by an earlier call are kept)
        with open(args.out) as f:
            res = {**json.load(f), **res}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)

    me = os.path.abspath(__file__)
    parent = os.path.abspath(args.parent) if args.parent else None
    if args.cases:
        res["kernel"] = run([me, "--leg", args.cases, "--rounds", str(args.rounds), "--launches", str(args.launches)],
                            ROOT)
        for name, r in res["kernel"].items():
            print(f"{name}: " + ", ".join(f"{k} {v} us" for k, v in r["median_us"].items()), flush=True)
        save()
    if args.iteration:
        legs = ([("parent_plain", parent, False)] if parent else []) + [("plain", ROOT, False), ("soft", ROOT, True)]
        ms = {who: [] for who, _, _ in legs}
        for rnd in range(args.rounds):
            for who, tree, soft in legs:
                cmd = [me, "--step-leg", tree, "--iteration-steps", str(args.iteration_steps)] + (["--soft"] if soft else [])
                ms[who].append(run(cmd, tree)["ms_per_step"])
            print(f"train_step round {rnd}: " + ", ".join(f"{who} {v[-1]:.3f} ms" for who, v in ms.items()), flush=True)
        it = {"ms_per_step": ms, "median_ms": {who: med(v) for who, v in ms.items()}}
        it["soft_minus_plain_ms"] = round(med(ms["soft"]) - med(ms["plain"]), 4)
        if parent:
            pp = ms["parent_plain"]
            it["plain_inside_parent_spread"] = min(pp) <= med(ms["plain"]) <= max(pp)
            it["plain_not_slower_than_parent_max"] = med(ms["plain"]) <= max(pp)
        res["train_step_c3_b256"] = it
        save()
    if parent and not args.no_bench:
        import numpy as np

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
