"""Cost of PPO's extra update epochs at C3 shapes: ms per Trainer.train_step at ppo_epochs = 1 (the plain A2C step),
2 and 4, in alternating rounds on one box, and ms per extra epoch.  The yardstick is the PARENT commit's plain
train_step, never this tree's own: ``--parent-tree DIR`` (a checkout of the parent with its library built) runs it in a
second process that stays resident and takes its turns in the same alternation.  An extra epoch launches one replay
forward, the PPO loss, one backward, Adam and a re-pack - one parent iteration less the draws and the image upload -
so it should cost one parent train_step within the parent's own round-to-round spread.  Also prints the traffic
estimates of the new launches (HBM-bound at COPY_GBS).  Their own durations and the launch counts come from a
rocprofv3 kernel trace of ``--trace-leg N`` (one process, ppo_epochs = N with max_grad_norm, no alternation;
tools/rocpd_stats.py; kernels loss_gae_kernel, loss_standardize_kernel, ppo_grads_kernel, ppo_final_kernel,
clip_partials_kernel, clip_scale_kernel).  Prints one JSON line.
usage: python tools/ppo_bench.py --parent-tree DIR [--batch 256] [--iters 10] [--rounds 3]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
COPY_GBS = 6290.0  # what a float4 copy reaches on this part
ACTIONS = [[1, 0], [-1, 0], [0, 1], [0, -1]]


def worker(tree: str, batch: int, iters: int) -> None:
    """Resident leg runner for the package under ``tree``: reads one leg per line ("1", "2", "4", "1c" = with
    max_grad_norm, ...; "q" quits), runs ``iters`` train_steps of it, answers with ms per step.  Leg "1" uses no
    keyword the parent commit lacks."""
    sys.path.insert(0, tree)
    import torch as th
    from bench import C3, IMG, NA, NS
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.networks import ModelsWrapper
    from marlclassification_amd.networks.vision import CNN_BY_NAME
    from marlclassification_amd.training import Trainer

    dev = th.device("cuda", 0)
    img = th.rand(batch, *IMG, device=dev)
    y = th.randint(C3["nb_class"], (batch,), device=dev)
    legs = {}

    def leg(name: str):
        if name not in legs:  # one model per leg (each has its own Adam state)
            th.manual_seed(0)
            model = ModelsWrapper(CNN_BY_NAME[C3["ft_extr"]](C3["window"]), C3["n_b"], C3["n_a"], C3["n_m"],
                                  C3["n_m_o"], C3["n_d"], 2, len(ACTIONS), C3["nb_class"], C3["nlb"], C3["nla"]).to(dev)
            sampler = EpisodeSampler(MultiAgent(NA, model), Environment(ACTIONS, C3["window"]), NS)
            kw = {}
            if name != "1":
                kw["ppo_epochs"] = int(name.rstrip("c"))
                if name.endswith("c"):
                    kw["max_grad_norm"] = 0.5
            trainer = Trainer(model, C3["nb_class"], 1e-4, 0.99, **kw)
            legs[name] = lambda t=trainer, s=sampler: t.train_step(img, y, s)
            for _ in range(3):
                legs[name]()
        return legs[name]

    print("ready", flush=True)
    for line in sys.stdin:
        name = line.strip()
        if name == "q":
            break
        f = leg(name)
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            f()
        th.cuda.synchronize()
        print(round(1e3 * (time.perf_counter() - t0) / iters, 3), flush=True)


class Proc:
    def __init__(self, tree: str, batch: int, iters: int) -> None:
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", tree, "--batch", str(batch),
                                   "--iters", str(iters)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        self._expect("ready")

    def _expect(self, what=None) -> str:
        line = self.p.stdout.readline().strip()
        if not line or (what is not None and line != what):
            raise RuntimeError(f"worker answered {line!r} (exit code {self.p.poll()})")
        return line

    def run(self, leg: str) -> float:
        self.p.stdin.write(leg + "\n")
        self.p.stdin.flush()
        return float(self._expect())

    def close(self) -> None:
        self.p.stdin.write("q\n")
        self.p.stdin.flush()
        self.p.wait(timeout=120)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit, library built: the yardstick")
    ap.add_argument("--worker", metavar="TREE", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--trace-leg", default=None, help="run only this leg (e.g. 2c) in this process, for a kernel trace")
    args = ap.parse_args()
    tree = os.path.dirname(HERE)
    if args.worker is not None:
        worker(args.worker, args.batch, args.iters)
        return
    if args.trace_leg is not None:
        import io

        sys.stdin = io.StringIO(f"{args.trace_leg}\nq\n")  # (in this process: the profiler sees the kernels)
        worker(tree, args.batch, args.iters)
        return

    if args.parent_tree is None:
        ap.error("--parent-tree is required: the yardstick is the parent commit's plain train_step, never this tree's")
    sys.path.insert(0, tree)
    import numpy as np
    from bench import C3, NA, NS
    from oracle import marl_oracle as mo

    here = Proc(tree, args.batch, args.iters)
    parent = Proc(os.path.abspath(args.parent_tree), args.batch, args.iters)
    legs = [
        ("parent_plain", parent, "1"), ("ppo_epochs_1", here, "1"), ("ppo_epochs_2", here, "2"), ("ppo_epochs_4", here, "4"),
        ("ppo_epochs_2_clip", here, "2c")]
    times = {k: [] for k, _, _ in legs}
    for k, p, leg in legs:  # builds the leg's trainer and warms it up
        p.run(leg)
    for _ in range(args.rounds):
        for k, p, leg in legs:
            times[k].append(p.run(leg))
    here.close()
    parent.close()

    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    base_key = "parent_plain"
    base = med[base_key]
    rows = NS * NA * args.batch
    us = lambda nbytes: round(nbytes / (COPY_GBS * 1e3), 2)  # noqa: E731
    out = {
        "shape": f"C3 Na={NA} Ns={NS} Nb={args.batch} nA={len(ACTIONS)} nC={C3['nb_class']}",
        "yardstick": base_key,
        "train_step_ms": times,
        "median_ms": med,
        "ms_per_extra_epoch": {"from_2": round(med["ppo_epochs_2"] - base, 3),
                               "from_4": round((med["ppo_epochs_4"] - base) / 3.0, 3)},
        "yardstick_round_to_round_spread_ms": round(max(times[base_key]) - min(times[base_key]), 3),
        "grad_clip_ms_per_epoch": round((med["ppo_epochs_2_clip"] - med["ppo_epochs_2"]) / 2.0, 3),
        "rows_Ns_R": rows,
        "traffic_bytes": {
            # reads logp, old_logp, values, ret, advn; writes g_logp, g_values
            "ppo_grads_kernel": 7 * rows * 4,
            # reads rewards and values, writes ret and the raw advantage
            "loss_gae_kernel": 4 * rows * 4,
            "loss_standardize_kernel": 2 * rows * 4,
        },
        "traffic_hbm_bound_us": {"ppo_grads_kernel": us(7 * rows * 4), "loss_gae_kernel": us(4 * rows * 4),
                                 "loss_standardize_kernel": us(2 * rows * 4)},
        "copy_gbs": COPY_GBS,
    }
    cfg = mo.OracleConfig(C3["ft_extr"], C3["window"], C3["n_b"], C3["n_a"], C3["n_m"], C3["n_m_o"], C3["n_d"],
                          C3["nb_class"], C3["nlb"], C3["nla"])
    n_params = sum((int(np.prod(shape)) + 3) & ~3 for shape in mo.param_shapes(cfg).values())  # FlatParams' layout
    out["flat_gradient_floats"] = n_params
    out["traffic_bytes"].update(clip_partials_kernel=4 * n_params, clip_scale_kernel=8 * n_params)
    out["traffic_hbm_bound_us"].update(clip_partials_kernel=us(4 * n_params), clip_scale_kernel=us(8 * n_params))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
