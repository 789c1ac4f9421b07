"""Cost of the colour jitter (``marl_batch_color``, ``color.apply``) against the same definition written in torch and
against the traffic bound; of a training step fed by it; and of the unchanged path against ANOTHER checkout (the parent
commit, built), on one box:

    python tools/color_bench.py [--parent DIR] [--rounds 3] [--launches 50] [--iteration] [--out profiles/color_c3.json]

  * the kernel: C3 (3 x 256 x 256 uint8, B = 256, rows random over a resident set larger than the 256 MB Infinity
    Cache; rows and destinations rotate over ``ROTATE`` buffers), HIP events around ``launches`` repetitions,
    ``rounds`` alternating rounds of the legs: the colour launch without records; with records kept from a statistics
    call; the two statistics launches and the colour launch together; the ``out_form="norm"`` launch; colour to uint8
    followed by ``transforms.apply`` of the same user transform (two launches); and the torch expression
    ``index_select -> .float() -> four stages -> round -> clamp -> .to(uint8)`` on the same rows.  Bounds: a launch
    reads the selected images once and writes the batch once (uint8, or fp32 for the fused form); the statistics read
    them once more; at the rate a float4 copy reaches.  Recorded, not gated;
  * ``--iteration``: ``rounds`` x (parent plain uint8 step, this tree's plain uint8 step, this tree's step on a batch
    jittered inside the timed loop - statistics and the colour launch) ``Trainer.train_step`` at C3, B = 256, every
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
N_SET, BATCH, SHAPE = 4096, 256, (3, 256, 256)
LEGS = ("color_no_records", "color_with_records", "stats_and_color", "color_out_norm", "color_then_normalize",
        "torch_expression")
USER = "user-normal:0.485,0.456,0.406:0.229,0.224,0.225"
JITTER = "brightness:0.4,contrast:0.4,saturation:0.4,hue:0.1,gray:0.1"


def med(v):
    return sorted(v)[len(v) // 2]


# ---- the child: the kernel legs -------------------------------------------------------------------------------------
def leg(rounds, launches):
    sys.path.insert(0, ROOT)
    import torch as th

    from marlclassification_amd import color, transforms

    dev = th.device("cuda", 0)
    x = th.randint(0, 256, (N_SET,) + SHAPE, dtype=th.uint8, device=dev)
    g = th.Generator(device=dev).manual_seed(1)
    policy = color.parse(JITTER)
    rows = [th.randint(0, N_SET, (BATCH,), generator=g, device=dev) for _ in range(ROTATE)]
    params = [policy.draw(BATCH, g) for _ in range(ROTATE)]
    dst8 = [th.empty((BATCH,) + SHAPE, dtype=th.uint8, device=dev) for _ in range(ROTATE)]
    dst32 = [th.empty((BATCH,) + SHAPE, dtype=th.float32, device=dev) for _ in range(ROTATE)]
    recs = [transforms.stats(x, r) for r in rows]
    grey = th.tensor(color.GREY, dtype=th.float32, device=dev).view(1, 3, 1, 1) / 256
    kmat = th.tensor(color.K, dtype=th.float32, device=dev)
    eye = th.eye(3, device=dev)

    def torch_expression(k):
        p = params[k].float()
        beta, kappa, sigma = (p[:, j].view(-1, 1, 1, 1) / color.Q12 for j in range(3))
        hc, hs = (p[:, j].view(-1, 1, 1) / color.Q14 for j in (3, 4))
        xb = x.index_select(0, rows[k]).float() * beta
        mu = (xb * grey).sum(1, keepdim=True).mean(dim=(2, 3), keepdim=True)
        xb = kappa * xb + (1 - kappa) * mu
        xb = sigma * xb + (1 - sigma) * (xb * grey).sum(1, keepdim=True)
        big_g = grey.view(1, 1, 3).expand(1, 3, 3)
        hue = big_g + hc * (eye - big_g) + hs * kmat
        return th.einsum("bij,bjhw->bihw", hue, xb).round().clamp(0, 255).to(th.uint8)

    def run(cls, k):
        if cls == "color_no_records":
            color.apply(x, rows[k], params[k], None, out=dst8[k])
        elif cls == "color_with_records":
            color.apply(x, rows[k], params[k], recs[k], out=dst8[k])
        elif cls == "stats_and_color":
            color.apply(x, rows[k], params[k], transforms.stats(x, rows[k]), out=dst8[k])
        elif cls == "color_out_norm":
            color.apply(x, rows[k], params[k], recs[k], out_form="norm", normalize=USER, out=dst32[k])
        elif cls == "color_then_normalize":
            transforms.apply(color.apply(x, rows[k], params[k], recs[k], out=dst8[k]), None, USER, out=dst32[k])
        else:
            torch_expression(k)

    times = {cls: [] for cls in LEGS}
    for cls in LEGS:  # warm-up
        for k in range(ROTATE):
            run(cls, k)
    # the launch computes what it should at the size that is timed
    got = color.apply(x, rows[1], params[1], recs[1])
    diff = int((got.int() - torch_expression(1).int()).abs().max())
    assert diff <= 2, diff  # (1 grey level of the definition, 1 of the fp32 expression)
    sub = rows[1][:4].cpu()
    assert th.equal(got[:4].cpu(), color.reference_apply(x.index_select(0, rows[1][:4]).cpu(), None, params[1][:4].cpu(),
                                                         recs[1][:4].cpu())), sub
    fused = color.apply(x, rows[1], params[1], recs[1], out_form="norm", normalize=USER)
    assert th.equal(fused.view(th.int32), transforms.apply(got, None, USER).view(th.int32))
    del got, fused
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
    src_bytes = BATCH * x[0].numel()
    bound = {"color_no_records": 2 * src_bytes, "color_with_records": 2 * src_bytes, "stats_and_color": 3 * src_bytes,
             "color_out_norm": 5 * src_bytes, "color_then_normalize": 7 * src_bytes}
    res = {"bytes_bound": bound, "bound_us_at_6.29_TBs": {k: round(v / COPY_TBS / 1e6, 2) for k, v in bound.items()},
           "resident_set_mb": round(x.numel() / 1e6, 1), "us": times, "jitter": JITTER, "normalize": USER,
           "plan": color.plan(x, dst8[0]), "plan_out_norm": color.plan(x, dst32[0], "norm"),
           "max_grey_levels_to_torch_expression": diff}
    res["median_us"] = {cls: med(v) for cls, v in times.items()}
    res["range_us"] = {cls: [min(v), max(v)] for cls, v in times.items()}
    m = res["median_us"]
    res["over_bound"] = {cls: round(m[cls] / res["bound_us_at_6.29_TBs"][cls], 3) for cls in LEGS[:5]}
    res["torch_over_stats_and_color"] = round(m["torch_expression"] / m["stats_and_color"], 3)
    res["two_steps_over_out_norm"] = round(m["color_then_normalize"] / m["color_out_norm"], 3)
    print(json.dumps(res))


# ---- the child: one train-step leg ----------------------------------------------------------------------------------
def step_leg(tree, steps, warmup, jitter):
    """``Trainer.train_step`` on bench.py's C3 workload (its model, sizes and seeds) of ``tree``, B = 256, fed from a
    resident uint8 set: the plain ``index_select`` batch, or (``jitter``) statistics + ``color.apply`` of the same rows
    under freshly drawn parameters"""
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
    if jitter:
        from marlclassification_amd import color, transforms

        policy = color.parse(jitter)

        def batch(k):
            r = rows[k % ROTATE]
            return color.apply(resident, r, policy.draw(nb, gen), transforms.stats(resident, r))
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-kernel", action="store_true", help="skip the kernel legs")
    ap.add_argument("--iteration", action="store_true", help="Trainer.train_step legs (with --parent: its leg too)")
    ap.add_argument("--iteration-steps", type=int, default=30)
    ap.add_argument("--no-bench", action="store_true", help="with --parent: skip the bench.py alternation")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", action="store_true", help="(child) the kernel legs")
    ap.add_argument("--step-leg", default=None, metavar="TREE", help="(child) one train-step leg of the tree")
    ap.add_argument("--step-jitter", default=None, metavar="SPEC", help="(child) the step's batches are jittered")
    args = ap.parse_args()
    if args.leg:
        leg(args.rounds, args.launches)
        return
    if args.step_leg:
        step_leg(args.step_leg, args.iteration_steps, 5, args.step_jitter)
        return
    res = {"rounds": args.rounds, "launches_per_timing": args.launches, "rotate": ROTATE}
    if args.out and os.path.exists(args.out):  # (sections measured by an earlier call are kept)
        with open(args.out) as f:
            res = {**json.load(f), **res}

    def save():
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")

    me = os.path.abspath(__file__)
    parent = os.path.abspath(args.parent) if args.parent else None
    if not args.no_kernel:
        res["kernel_c3_u8_b256"] = r = run([me, "--leg", "--rounds", str(args.rounds), "--launches", str(args.launches)],
                                           ROOT)
        print(", ".join(f"{k} {v} us" for k, v in r["median_us"].items()) + f"; bounds {r['bound_us_at_6.29_TBs']}",
              flush=True)
        save()
    if args.iteration:
        legs = ([("parent_plain_u8", parent, None)] if parent else []) + [("this_plain_u8", ROOT, None),
                                                                          ("this_jittered", ROOT, JITTER)]
        ms = {who: [] for who, _, _ in legs}
        for rnd in range(args.rounds):
            for who, tree, spec in legs:
                cmd = [me, "--step-leg", tree, "--iteration-steps", str(args.iteration_steps)]
                ms[who].append(run(cmd + (["--step-jitter", spec] if spec else []), ROOT)["ms_per_step"])
            print(f"train_step round {rnd}: " + ", ".join(f"{who} {v[-1]:.3f} ms" for who, v in ms.items()), flush=True)
        it = {"ms_per_step": ms, "median_ms": {who: med(v) for who, v in ms.items()},
              "range_ms": {who: [min(v), max(v)] for who, v in ms.items()}}
        it["jittered_minus_plain_ms"] = round(med(ms["this_jittered"]) - med(ms["this_plain_u8"]), 4)
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
