"""Cost of the per-image input normalisation (``marl_batch_stats`` + ``marl_batch_normalize``, ``transforms.apply``)
against what a user writes without it and against the traffic bound; of a training step fed by it; and of the unchanged
path against ANOTHER checkout (the parent commit, built), on one box:

    python tools/normalize_bench.py [--parent DIR] [--rounds 5] [--launches 50] [--iteration] [--out profiles/normalize_c3.json]

  * the kernels: per case (C3 uint8 B = 256, C3 fp32 B = 256) HIP events around ``launches`` repetitions, ``rounds``
    alternating rounds of the legs: the two statistics launches alone; the apply launch alone under ``channel-normal``
    (records kept from a statistics call) and under ``user-normal``; all three together (``transforms.apply`` of
    ``channel-normal``); and the torch expression ``index_select -> .float().div(255) -> mean / std over (H, W) -> sub
    -> div`` (fp32 sources: without the div(255)) on the same rows.  The resident set is larger than the 256 MB Infinity
    Cache, rows are random over it, and rows / destinations rotate over ``ROTATE`` buffers.  Bounds: the statistics
    read the selected images once; the apply reads them once and writes the fp32 batch once; at the rate a float4 copy
    reaches.  Requirement: the three launches together are not slower than the torch expression (medians; no margin).
    The ratios to the bound are findings;
  * ``--iteration``: ``rounds`` x (parent plain uint8 step, this tree's plain uint8 step, this tree's step on a batch
    normalised by ``channel-normal`` with the three launches inside the timed loop) ``Trainer.train_step`` at C3,
    B = 256, every leg a fresh child process;
  * ``--parent DIR``: ``rounds`` x (parent, this tree) ``bench.py --gpus 1``, every leg a fresh child process, and
    ``--dump-outputs`` of both trees compared array by array."""
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
}
LEGS = ("stats_two_launches", "apply_channel_normal", "apply_user_normal", "all_three_channel_normal",
        "torch_expression")
USER = "user-normal:0.485,0.456,0.406:0.229,0.224,0.225"


def med(v):
    return sorted(v)[len(v) // 2]


# ---- the child: the kernel legs -------------------------------------------------------------------------------------
def leg(rounds, launches, cases):
    sys.path.insert(0, ROOT)
    import torch as th

    from marlclassification_amd import transforms

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
        dst = [th.empty((batch,) + shape, dtype=th.float32, device=dev) for _ in range(ROTATE)]
        recs = [transforms.stats(x, r) for r in rows]
        src_bytes = batch * x[0].numel() * x.element_size()
        dst_bytes = batch * x[0].numel() * 4

        def torch_expression(k):
            xb = x.index_select(0, rows[k]).float()
            if dtype == th.uint8:
                xb = xb.div(255)
            mean, std = xb.mean(dim=(2, 3), keepdim=True), xb.std(dim=(2, 3), keepdim=True)
            return xb.sub(mean).div(std)

        def run(cls, k):
            if cls == "stats_two_launches":
                transforms.stats(x, rows[k])
            elif cls == "apply_channel_normal":
                transforms.apply(x, rows[k], "channel-normal", out=dst[k], records=recs[k])
            elif cls == "apply_user_normal":
                transforms.apply(x, rows[k], USER, out=dst[k])
            elif cls == "all_three_channel_normal":
                transforms.apply(x, rows[k], "channel-normal", out=dst[k])
            else:
                torch_expression(k)

        times = {cls: [] for cls in LEGS}
        for cls in LEGS:  # warm-up
            for k in range(ROTATE):
                run(cls, k)
        # the launches compute what they should at the size that is timed
        got = transforms.apply(x, rows[1], "channel-normal")
        err = float((got - torch_expression(1)).abs().max())
        assert err <= 1e-4, err
        sub = rows[1][:4]
        if dtype == th.uint8:
            assert th.equal(transforms.stats(x, sub).cpu(), transforms.reference_stats(x.index_select(0, sub).cpu()))
        del got
        for _ in range(rounds):
            for cls in LEGS:
                n = launches if cls != "torch_expression" else max(5, launches // 5)
                start, end = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                th.cuda.synchronize(dev)
                start.record()
                for i in range(n):
                    run(cls, i % ROTATE)
                end.record()
                end.synchronize()
                times[cls].append(round(1e3 * start.elapsed_time(end) / n, 3))
        bound = {"stats_two_launches": src_bytes, "apply_channel_normal": src_bytes + dst_bytes,
                 "apply_user_normal": src_bytes + dst_bytes, "all_three_channel_normal": 2 * src_bytes + dst_bytes}
        res = {"bytes_bound": bound, "bound_us_at_6.29_TBs": {k: round(v / COPY_TBS / 1e6, 2) for k, v in bound.items()},
               "resident_set_mb": round(x.numel() * x.element_size() / 1e6, 1), "us": times,
               "plan": transforms.plan(x, dst[0]), "max_abs_diff_to_torch_expression": err}
        res["median_us"] = {cls: med(v) for cls, v in times.items()}
        res["range_us"] = {cls: [min(v), max(v)] for cls, v in times.items()}
        m = res["median_us"]
        res["over_bound"] = {cls: round(m[cls] / res["bound_us_at_6.29_TBs"][cls], 3) for cls in LEGS[:4]}
        res["torch_over_all_three"] = round(m["torch_expression"] / m["all_three_channel_normal"], 3)
        res["not_slower_than_torch"] = m["all_three_channel_normal"] <= m["torch_expression"]
        out[name] = res
        del x, dst, recs
        th.cuda.empty_cache()
    print(json.dumps(out))


# ---- the child: one train-step leg ----------------------------------------------------------------------------------
def step_leg(tree, steps, warmup, normalize):
    """``Trainer.train_step`` on bench.py's C3 workload (its model, sizes and seeds) of ``tree``, B = 256, fed from a
    resident uint8 set: the plain ``index_select`` batch, or (``normalize``) ``transforms.apply`` of the same rows"""
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
    resident = th.randint(0, 256, (2048,) + tuple(bench.IMG), dtype=th.uint8, device=dev, generator=gen)
    rows = [th.randint(0, 2048, (nb,), device=dev, generator=gen) for _ in range(ROTATE)]
    y = th.randint(0, c["nb_class"], (nb,), device=dev, generator=gen)
    if normalize:
        from marlclassification_amd import transforms

        def batch(k):
            return transforms.apply(resident, rows[k % ROTATE], normalize)
    else:
        def batch(k):
            return resident.index_select(0, rows[k % ROTATE])
    for k in range(warmup):
        trainer.train_step(batch(k), y, sampler)
    th.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for k in range(steps):
        out, scalars = trainer.train_step(batch(k), y, sampler)
    th.cuda.synchronize(dev)
    ms = 1e3 * (time.perf_counter() - t0) / steps
    assert bool(th.isfinite(scalars).all())
    print(json.dumps({"ms_per_step": round(ms, 4), "loss": float(scalars[0])}))


# ---- the parent process ---------------------------------------------------------------------------------------------
def run(cmd, tree, timeout=900):
    r = subprocess.run([sys.executable] + cmd, cwd=tree, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} in {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-3000:]}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]) if lines else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="checkout of the parent commit (built): the unchanged path")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iteration", action="store_true", help="Trainer.train_step legs (with --parent: its leg too)")
    ap.add_argument("--iteration-steps", type=int, default=30)
    ap.add_argument("--no-bench", action="store_true", help="with --parent: skip the bench.py alternation")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, help="(child) comma-separated cases")
    ap.add_argument("--step-leg", default=None, metavar="TREE", help="(child) one train-step leg of the tree")
    ap.add_argument("--step-normalize", default=None, metavar="SPEC", help="(child) the step's batches are normalised")
    args = ap.parse_args()
    if args.leg:
        leg(args.rounds, args.launches, args.leg.split(","))
        return
    if args.step_leg:
        step_leg(args.step_leg, args.iteration_steps, 5, args.step_normalize)
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
            print(f"{name}: " + ", ".join(f"{k} {v} us" for k, v in r["median_us"].items()) +
                  f"; bounds {r['bound_us_at_6.29_TBs']}", flush=True)
        res["three_launches_not_slower_than_torch"] = all(r["not_slower_than_torch"] for r in res["kernel"].values())
        save()
    if args.iteration:
        legs = ([("parent_plain_u8", parent, None)] if parent else []) + [("this_plain_u8", ROOT, None),
                                                                          ("this_channel_normal", ROOT, "channel-normal")]
        ms = {who: [] for who, _, _ in legs}
        for rnd in range(args.rounds):
            for who, tree, spec in legs:
                cmd = [me, "--step-leg", tree, "--iteration-steps", str(args.iteration_steps)]
                ms[who].append(run(cmd + (["--step-normalize", spec] if spec else []), ROOT)["ms_per_step"])
            print(f"train_step round {rnd}: " + ", ".join(f"{who} {v[-1]:.3f} ms" for who, v in ms.items()), flush=True)
        it = {"ms_per_step": ms, "median_ms": {who: med(v) for who, v in ms.items()},
              "range_ms": {who: [min(v), max(v)] for who, v in ms.items()}}
        it["normalised_minus_plain_ms"] = round(med(ms["this_channel_normal"]) - med(ms["this_plain_u8"]), 4)
        if parent:
            it["plain_not_slower_than_parent_max"] = med(ms["this_plain_u8"]) <= max(ms["parent_plain_u8"])
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
    print(json.dumps(res))


if __name__ == "__main__":
    main()
