"""Cost of the resampling batch gather (``marl_batch_warp``, ``warp.apply``) against this tree's plain
``marl_batch_augment`` gather, against what a user writes without it (``index_select`` -> ``.float()`` ->
``affine_grid`` + ``grid_sample``) and against the traffic bound; and the unchanged path against ANOTHER checkout (the
parent commit, built), on one box:

    python tools/warp_bench.py [--parent DIR] [--rounds 5] [--launches 50] [--iteration] [--out profiles/warp_c3.json]

  * the kernel: per case (C3 uint8 B = 256, C3 fp32 B = 256, AID uint8 B = 32, AID fp32 B = 32) HIP events around
    ``launches`` launches, ``rounds`` alternating rounds of the legs: ``warp.apply`` under identity matrices, under a
    15 degree rotation, under the full ``d4,rotate:15,scale:0.8:1.25,shift:8,erase:32`` draw; ``augment.apply`` (the
    plain gather of the same rows); and the torch path on the same rows and the 15 degree matrices (zero padding,
    bilinear, ``align_corners=False``; for uint8 the fp32 batch it yields is what a user trains on).  The resident set
    is larger than the 256 MB Infinity Cache, rows are random over it, and rows / matrices / destinations rotate over
    ``ROTATE`` buffers, so the figures are HBM figures.  The bound is the selected images read once plus the batch
    written once, at the rate a float4 copy reaches.  Requirement: the warp launch is not slower than the torch leg
    (medians; no margin).  The ratios to the plain gather and to the bound are findings;
  * ``--iteration``: ``rounds`` x (parent, this tree) ``Trainer.train_step`` at C3, B = 256, no augmentation, every
    leg a fresh child process;
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
SPEC = "d4,rotate:15,scale:0.8:1.25,shift:8,erase:32"
# name -> (dtype, images in the resident set, batch, [C, H, W])
CASES = {
    "c3_u8_b256": ("uint8", 4096, 256, (3, 256, 256)),
    "c3_f32_b256": ("float32", 1024, 256, (3, 256, 256)),
    "aid_u8_b32": ("uint8", 800, 32, (3, 600, 600)),
    "aid_f32_b32": ("float32", 400, 32, (3, 600, 600)),
}
LEGS = ("warp_identity", "warp_rotate15", "warp_full_draw", "augment_plain_gather", "torch_grid_sample")


def med(v):
    return sorted(v)[len(v) // 2]


# ---- the child: the kernel legs -------------------------------------------------------------------------------------
def leg(rounds, launches, cases):
    sys.path.insert(0, ROOT)
    import torch as th
    import torch.nn.functional as F

    from marlclassification_amd import augment, warp

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
        ident = warp.identity(batch, dev)
        rot = warp.matrices(th.full((batch,), 15.0, device=dev), th.ones(batch, device=dev), th.ones(batch, device=dev))
        policy = augment.parse(SPEC)
        full = [policy.draw_warp(batch, g, size=shape[1:]) for _ in range(ROTATE)]
        # the torch path's theta of the same 15 degree map: affine_grid works in (x, y), normalised by (W, H)
        a = rot[:, :4].float() / warp.ONE
        theta = th.zeros(batch, 2, 3, device=dev)
        theta[:, 0, 0], theta[:, 0, 1] = a[:, 3], a[:, 2] * shape[1] / shape[2]
        theta[:, 1, 0], theta[:, 1, 1] = a[:, 1] * shape[2] / shape[1], a[:, 0]
        nbytes = 2 * batch * x[0].numel() * x.element_size()

        def run(cls, k):
            if cls == "warp_identity":
                warp.apply(x, rows[k], ident, out=dst[k])
            elif cls == "warp_rotate15":
                warp.apply(x, rows[k], rot, pad_mode="zero", out=dst[k])
            elif cls == "warp_full_draw":
                warp.apply(x, rows[k], full[k][1], full[k][0], out=dst[k])
            elif cls == "augment_plain_gather":
                augment.apply(x, rows[k], None, out=dst[k])
            else:
                xb = x.index_select(0, rows[k]).float()
                grid = F.affine_grid(theta, list(xb.shape), align_corners=False)
                F.grid_sample(xb, grid, mode="bilinear", padding_mode="zeros", align_corners=False)

        times = {cls: [] for cls in LEGS}
        for cls in LEGS:  # warm-up
            for k in range(ROTATE):
                run(cls, k)
        # the launches compute what they should at the size that is timed
        assert th.equal(dst[0].copy_(warp.apply(x, rows[0], ident)), x.index_select(0, rows[0]))
        xb = x.index_select(0, rows[1]).float()
        ref = F.grid_sample(xb, F.affine_grid(theta, list(xb.shape), align_corners=False), mode="bilinear",
                            padding_mode="zeros", align_corners=False)
        got = warp.apply(x, rows[1], rot, pad_mode="zero").float()
        span = 255.0 if dtype == th.uint8 else 1.0
        err = float((got - ref).abs().max()) / span
        assert err <= 4.5e-3 + (0.5 / 255 if dtype == th.uint8 else 0.0), err  # (uint8: plus its own rounding)
        del xb, ref, got
        for _ in range(rounds):
            for cls in LEGS:
                n = launches if cls != "torch_grid_sample" else max(5, launches // 5)
                start, end = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
                th.cuda.synchronize(dev)
                start.record()
                for i in range(n):
                    run(cls, i % ROTATE)
                end.record()
                end.synchronize()
                times[cls].append(round(1e3 * start.elapsed_time(end) / n, 3))
        res = {"bytes_per_launch_bound": nbytes, "bound_us_at_6.29_TBs": round(nbytes / COPY_TBS / 1e6, 2),
               "resident_set_mb": round(x.numel() * x.element_size() / 1e6, 1), "us_per_launch": times,
               "plan": warp.plan(x, dst[0]), "max_err_vs_grid_sample_over_span": round(err, 6)}
        res["median_us"] = {cls: med(v) for cls, v in times.items()}
        res["range_us"] = {cls: [min(v), max(v)] for cls, v in times.items()}
        m = res["median_us"]
        res["over_plain_gather"] = {cls: round(m[cls] / m["augment_plain_gather"], 3) for cls in LEGS[:3]}
        res["over_bound"] = {cls: round(m[cls] / res["bound_us_at_6.29_TBs"], 3) for cls in LEGS[:4]}
        res["torch_over_warp_rotate15"] = round(m["torch_grid_sample"] / m["warp_rotate15"], 3)
        res["not_slower_than_torch"] = {cls: m[cls] <= m["torch_grid_sample"] for cls in LEGS[:3]}
        out[name] = res
        del x, dst
        th.cuda.empty_cache()
    print(json.dumps(out))


# ---- the child: one train-step leg ----------------------------------------------------------------------------------
def step_leg(tree, steps, warmup):
    """``Trainer.train_step`` on bench.py's C3 workload (its model, sizes and seeds) of ``tree``, B = 256"""
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
    for _ in range(warmup):
        trainer.train_step(img, y, sampler)
    th.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        out, scalars = trainer.train_step(img, y, sampler)
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
    args = ap.parse_args()
    if args.leg:
        leg(args.rounds, args.launches, args.leg.split(","))
        return
    if args.step_leg:
        step_leg(args.step_leg, args.iteration_steps, 5)
        return
    res = {"rounds": args.rounds, "launches_per_timing": args.launches, "rotate": ROTATE, "full_draw_spec": SPEC}
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
                  f"; bound {r['bound_us_at_6.29_TBs']} us", flush=True)
        res["warp_not_slower_than_torch"] = all(all(r["not_slower_than_torch"].values())
                                                for r in res["kernel"].values())
        save()
    if args.iteration:
        legs = ([("parent", parent)] if parent else []) + [("this", ROOT)]
        ms = {who: [] for who, _ in legs}
        for rnd in range(args.rounds):
            for who, tree in legs:
                ms[who].append(run([me, "--step-leg", tree, "--iteration-steps", str(args.iteration_steps)],
                                   tree)["ms_per_step"])
            print(f"train_step round {rnd}: " + ", ".join(f"{who} {v[-1]:.3f} ms" for who, v in ms.items()), flush=True)
        it = {"ms_per_step": ms, "median_ms": {who: med(v) for who, v in ms.items()},
              "range_ms": {who: [min(v), max(v)] for who, v in ms.items()}}
        if parent:
            it["this_not_slower_than_parent_max"] = med(ms["this"]) <= max(ms["parent"])
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
