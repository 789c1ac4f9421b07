"""Trainer.train_step at the flagship shape (bench.py's C3: RESISC45 dims, 16 agents, 16 steps, B = 256) under
communication graphs, next to the plain step of ANOTHER checkout (the parent commit) as the yardstick.

    python tools/comm_bench.py --parent DIR [--rounds 3] [--steps 30] [--warmup 5] [--out profiles/comm_c3.json]
    python tools/comm_bench.py --one GRAPH [--tree DIR]       # one leg: plain | full | ring | none (a JSON line)

Every leg is a fresh child process; a round runs parent-plain, plain, full, ring, none in that order, so the legs
alternate with the yardstick on one box.  ``--tree DIR`` imports the package (and bench.py's constants) from DIR."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("plain", "full", "ring", "none")


def one(graph: str, tree: str, steps: int, warmup: int, batch: int) -> None:
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
    form = None
    if graph != "plain":
        from marlclassification_amd import comm

        model.set_comm(getattr(comm, graph)(bench.NA).to(dev))
    sampler = EpisodeSampler(MultiAgent(bench.NA, model), Environment(actions, c["window"]), bench.NS)
    trainer = Trainer(model, c["nb_class"], bench.LR, bench.GAMMA)
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
    print(json.dumps({"graph": graph, "ms_per_step": ms, "steps": steps, "batch": batch, "comm_form": form,
                      "loss": scalars[0].item()}))


def leg(graph: str, tree: str, args) -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--one", graph, "--tree", tree, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--batch", str(args.batch)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tree)
    if r.returncode != 0:
        raise SystemExit(f"leg {graph} in {tree} failed ({r.returncode}):\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=LEGS)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--parent", help="checkout of the parent commit (built): its plain step is the yardstick")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.one:
        one(args.one, os.path.abspath(args.tree), args.steps, args.warmup, args.batch)
        return
    if not args.parent:
        ap.error("--parent DIR (or --one GRAPH)")
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


if __name__ == "__main__":
    main()
