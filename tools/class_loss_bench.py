"""Cost of the loss options (class weights, label smoothing, step weights, weighted rewards) at C3 shapes: ms per
Trainer.train_step with all four on, with none, and of the PARENT commit's plain train_step - the yardstick, never this
tree's own: ``--parent-tree DIR`` (a checkout of the parent with its library built) runs it in a second process that
stays resident and takes its turns in the same alternation (tools/ppo_bench.py is the model).  The options add no
launch: loss_error_kernel / loss_rewards_kernel run their option instances, which read nC + Ns more floats per wave, so
the step should cost the parent's within the parent's own round-to-round spread.  ``--trace-leg all`` runs one leg in
this process with no alternation, for whoever wants the two kernels' own durations from a rocprofv3 kernel trace
(tools/rocpd_stats.py); the numbers this tool prints need none.  Prints one JSON line.
usage: python tools/class_loss_bench.py --parent-tree DIR [--batch 256] [--iters 10] [--rounds 3]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ACTIONS = [[1, 0], [-1, 0], [0, 1], [0, -1]]


def worker(tree: str, batch: int, iters: int) -> None:
    """Resident leg runner for the package under ``tree``: reads one leg per line ("plain", "all"; "q" quits), runs
    ``iters`` train_steps of it, answers with ms per step.  Leg "plain" uses no keyword the parent commit lacks."""
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
            if name == "all":
                from marlclassification_amd.class_loss import balanced_weights

                kw = dict(class_weights=balanced_weights(y.cpu(), C3["nb_class"]).tolist(), label_smoothing=0.1,
                          error_step_weights="linear", weight_rewards=True)
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
    ap.add_argument("--trace-leg", default=None,
                    help="run only this leg (plain, all) in this process, for a kernel trace")
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
    from bench import C3, NA, NS

    here = Proc(tree, args.batch, args.iters)
    parent = Proc(os.path.abspath(args.parent_tree), args.batch, args.iters)
    legs = [("parent_plain", parent, "plain"), ("plain", here, "plain"), ("all_options", here, "all")]
    times = {k: [] for k, _, _ in legs}
    for k, p, leg in legs:  # builds the leg's trainer and warms it up
        p.run(leg)
    for _ in range(args.rounds):
        for k, p, leg in legs:
            times[k].append(p.run(leg))
    here.close()
    parent.close()

    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    base = med["parent_plain"]
    nc = C3["nb_class"]
    out = {
        "shape": f"C3 Na={NA} Ns={NS} Nb={args.batch} nA={len(ACTIONS)} nC={nc}",
        "yardstick": "parent_plain",
        "options": "class_weights=balanced, label_smoothing=0.1, error_step_weights=linear, weight_rewards",
        "iters_per_round": args.iters,
        "train_step_ms": times,
        "median_ms": med,
        "yardstick_round_to_round_spread_ms": round(max(times["parent_plain"]) - min(times["parent_plain"]), 3),
        "all_options_minus_yardstick_ms": round(med["all_options"] - base, 3),
        "plain_minus_yardstick_ms": round(med["plain"] - base, 3),
        # what the option instances read beyond the plain ones, per wave: the class weights and one step weight
        # (loss_error_kernel, Ns * Nb waves), one class weight (loss_rewards_kernel, Ns * Na * Nb waves)
        "extra_bytes_read": {"loss_error_kernel": NS * args.batch * (nc + 1) * 4,
                             "loss_rewards_kernel": NS * NA * args.batch * 4},
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
