#!/usr/bin/env python
"""Times the flat optimiser step at the C3 parameter count and writes profiles/optim_c3.json.

    python tools/optim_bench.py [--parent TREE] [--out FILE] [--rounds N] [--skip-iterations] [--lib FILE]

Per launch (1.69 M parameters): ``adam_kernel`` against ``optim_kernel`` in three forms - neutral options, decay plus
groups, and with the averaged weights.  Every form is captured as a hipGraph of LAUNCHES kernel nodes (a 10 us kernel
launched from Python measures the enqueue, not the kernel) and the replays are timed with device events, the forms
alternating round by round.  The bar of a form is the median of adam_kernel in that same run times the byte ratio of
the form (7 streams of 4n bytes, 9 with the averaged weights) plus the spread (max - min) of adam_kernel's own rounds.

Per iteration (C3, batch 256): ``Trainer.train_step`` with optim=None and with full options, and ``iteration_graph``
under a cosine schedule against the constant-rate Adam graph, alternating.  ``--parent TREE`` (a built checkout of the
parent commit): its adam_kernel is the per-launch baseline and its Trainer / FusedA2C run as further arms, in a worker
process of their own that takes turns with this tree's worker; without it the baseline is this library's adam_kernel
(the same source) and this tree's optim=None path (the parent's sequence of calls).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3 = dict(ft_extr="resisc45", window=12, n_b=256, n_a=256, n_m=64, n_m_o=96, n_d=16, nb_class=45, nlb=384, nla=384)
NA, NS, IMG, GAMMA, LR = 16, 16, (3, 256, 256), 0.99, 1e-4
ACTIONS = [[1, 0], [-1, 0], [0, 1], [0, -1]]
LAUNCHES = 100  # kernel nodes per captured graph
ITERS = 10      # iterations per timed window


# ---- worker: one tree, one process, arms built on first use ---------------------------------------------------------
class Worker:
    def __init__(self, tree: str, batch: int, parent_lib: str) -> None:
        sys.path.insert(0, tree)
        import torch as th

        self.th, self.batch, self.parent_lib = th, batch, parent_lib
        self.dev = th.device("cuda:0")
        self.arms = {}
        self.launch = None

    def model(self):
        from marlclassification_amd.networks import ModelsWrapper
        from marlclassification_amd.networks.vision import CNN_BY_NAME

        self.th.manual_seed(0)
        return ModelsWrapper(CNN_BY_NAME[C3["ft_extr"]](C3["window"]), C3["n_b"], C3["n_a"], C3["n_m"], C3["n_m_o"],
                             C3["n_d"], 2, len(ACTIONS), C3["nb_class"], C3["nlb"], C3["nla"]).to(self.dev)

    def options(self, total: int):
        from marlclassification_amd import optim as O

        return O.OptimOptions(weight_decay=0.01, groups={"cnn": 0.1, "critic": (1.0, 0.02)},
                              schedule=O.Schedule("cosine", None, 10, total, 0.1), ema_decay=0.999)

    def data(self):
        th = self.th
        gen = th.Generator(device=self.dev).manual_seed(0)
        img = th.rand(self.batch, *IMG, device=self.dev, generator=gen)
        y = th.randint(0, C3["nb_class"], (self.batch,), device=self.dev, generator=gen)
        return img, y

    def arm(self, name: str):
        """A callable that runs ONE iteration of the arm."""
        if name in self.arms:
            return self.arms[name]
        th = self.th
        img, y = self.data()
        model = self.model()
        if name.startswith("step_"):
            from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
            from marlclassification_amd.training import Trainer

            sampler = EpisodeSampler(MultiAgent(NA, model), Environment(ACTIONS, C3["window"]), NS)
            kw = {"optim": self.options(100000)} if name == "step_optim" else {}
            trainer = Trainer(model, C3["nb_class"], LR, GAMMA, **kw)
            fn = lambda: trainer.train_step(img, y, sampler)  # noqa: E731
        else:
            from marlclassification_amd.fused import FusedA2C

            eng = model.hip_engine(ACTIONS)
            eng.configure(NA, self.batch, NS, IMG)
            kw = {"optim": self.options(100000)} if name == "graph_cosine" else {}
            fa = FusedA2C(eng, model.flat_state(), LR, GAMMA, use_graph=True, **kw)
            it = [0]

            def fn():
                fa.iteration_graph(img, y, 42, it[0])
                it[0] += 1
        for _ in range(3):
            fn()
        th.cuda.synchronize()
        self.arms[name] = fn
        return fn

    def time_arm(self, name: str, iters: int) -> float:
        fn = self.arm(name)
        self.th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        self.th.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3  # ms per iteration

    # -- per launch ---------------------------------------------------------------------------------------------------
    def launch_setup(self):
        import ctypes as C

        from marlclassification_amd import _lib
        from marlclassification_amd import optim as O
        from marlclassification_amd.engine import _stream

        th = self.th
        model = self.model()
        flat = model.flat_state()
        eng = model.hip_engine(ACTIONS)
        n = flat.numel
        gen = th.Generator(device=self.dev).manual_seed(1)
        flat.grads.copy_(th.randn(n, device=self.dev, generator=gen) * 1e-2)
        flat.ema_buffer()
        adam_lib = _lib.load()
        if self.parent_lib:
            adam_lib = C.CDLL(self.parent_lib)
            vp, i64, f = C.c_void_p, C.c_int64, C.c_float
            adam_lib.marl_adam_step.argtypes = [vp, vp, vp, vp, i64, i64, f, f, f, f, f, vp, vp]
            adam_lib.marl_adam_step.restype = C.c_int
        base = O.Schedule("cosine", LR, 10, 100000, 0.1)
        forms = {
            "optim_neutral": O.OptimOptions(schedule=O.Schedule("constant", LR)),
            "optim_groups": O.OptimOptions(weight_decay=0.01, groups={"cnn": 0.1, "critic": (1.0, 0.02)}, schedule=base),
            "optim_ema": O.OptimOptions(weight_decay=0.01, groups={"cnn": 0.1, "critic": (1.0, 0.02)}, schedule=base,
                                        ema_decay=0.999),
        }
        tables = {k: O.segments(flat, o) for k, o in forms.items()}

        def one(name):
            if name == "adam":
                rc = adam_lib.marl_adam_step(flat.params.data_ptr(), flat.grads.data_ptr(), flat.exp_avg.data_ptr(),
                                             flat.exp_avg_sq.data_ptr(), n, 100, LR, 0.9, 0.999, 1e-8, 1.0, None,
                                             _stream(self.dev))
                assert rc == 0
            else:
                eng.optim_step(flat.params, flat.grads, flat.exp_avg, flat.exp_avg_sq, tables[name], forms[name],
                               step=100, ema=flat.ema if name == "optim_ema" else None)

        stream = th.cuda.Stream(device=self.dev)
        graphs = {}
        for name in ["adam"] + list(forms):
            one(name)  # (eager once: code objects load outside the capture)
            th.cuda.synchronize()
            with th.cuda.stream(stream):
                eng.graph_begin()
                for _ in range(LAUNCHES):
                    one(name)
                graphs[name] = eng.graph_end()
                for _ in range(3):
                    eng.graph_launch(graphs[name])
            th.cuda.synchronize()
        self.launch = (eng, stream, graphs)
        return {"n": n, "segments": {k: len(t) for k, t in tables.items()}}

    def time_launch(self, name: str, replays: int) -> float:
        th = self.th
        eng, stream, graphs = self.launch
        a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
        with th.cuda.stream(stream):
            a.record(stream)
            for _ in range(replays):
                eng.graph_launch(graphs[name])
            b.record(stream)
        th.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / (replays * LAUNCHES)  # us per launch


def worker_main(args) -> None:
    w = Worker(args.worker, args.batch, args.parent_lib)
    print(json.dumps({"ready": True}), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        if cmd[0] == "launch_setup":
            res = w.launch_setup()
        elif cmd[0] == "launch":
            res = {"us": w.time_launch(cmd[1], int(cmd[2]))}
        else:
            res = {"ms": w.time_arm(cmd[1], int(cmd[2]))}
        print(json.dumps(res), flush=True)


# ---- orchestrator (never opens the GPU itself) ----------------------------------------------------------------------
class Child:
    def __init__(self, tree: str, batch: int, parent_lib: str, lib: str = "") -> None:
        env = dict(os.environ)
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MARL_LIB_PATH"):
            env.pop(k, None)
        if lib:  # (another build of this tree's library: an ablation)
            env["MARL_LIB_PATH"] = os.path.abspath(lib)
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", tree, "--batch", str(batch)]
        if parent_lib:
            cmd += ["--parent-lib", parent_lib]
        self.p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=tree)
        self.ask(None)

    def ask(self, line):
        if line is not None:
            self.p.stdin.write(line + "\n")
            self.p.stdin.flush()
        while True:
            out = self.p.stdout.readline()
            if not out:
                raise SystemExit(f"worker died (exit {self.p.poll()})")
            if out.startswith("{"):
                return json.loads(out)

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=60)


def stats(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_c3.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--skip-iterations", action="store_true")
    ap.add_argument("--lib", default="", help="another build of this tree's library (an ablation build)")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        worker_main(args)
        return
    parent_lib = ""
    if args.parent:
        parent_lib = os.path.join(os.path.abspath(args.parent), "marlclassification_amd", "csrc", "libmarl_hip.so")
        if not os.path.exists(parent_lib):
            raise SystemExit(f"{parent_lib} is missing: build the parent tree first")
    new = Child(ROOT, args.batch, parent_lib, args.lib)
    old = Child(os.path.abspath(args.parent), args.batch, "") if args.parent and not args.skip_iterations else None
    result = {"parameters": None, "batch": args.batch, "launches_per_graph": LAUNCHES,
              "adam_kernel_from": "the parent commit's library" if parent_lib else "this library (same source)"}
    try:
        info = new.ask("launch_setup")
        n = info["n"]
        result["parameters"], result["segments"] = n, info["segments"]
        forms = ["adam", "optim_neutral", "optim_groups", "optim_ema"]
        times = {f: [] for f in forms}
        for r in range(args.rounds):
            for f in (forms if r % 2 == 0 else forms[::-1]):
                times[f].append(new.ask(f"launch {f} 20")["us"])
        per = {f: stats(t) for f, t in times.items()}
        adam = per["adam"]
        spread = adam["max"] - adam["min"]
        for f in forms:
            streams = 9 if f == "optim_ema" else 7
            per[f]["bytes"] = streams * 4 * n
            per[f]["GB_per_s"] = per[f]["bytes"] / (per[f]["median"] * 1e-6) / 1e9
            if f != "adam":
                per[f]["bar_us"] = adam["median"] * streams / 7.0 + spread
                per[f]["within_bar"] = per[f]["median"] <= per[f]["bar_us"]
        result["per_launch_us"] = per
        result["per_launch_bar"] = "median(adam_kernel) * bytes ratio (1, or 9/7 with ema) + (max - min) of adam_kernel"
        if not args.skip_iterations:
            arms = [(new, "step_adam"), (new, "step_optim"), (new, "graph_adam"), (new, "graph_cosine")]
            if old is not None:
                arms = [(old, "step_adam"), (old, "graph_adam")] + arms
            names = [("parent:" if c is old else "") + a for c, a in arms]
            it = {k: [] for k in names}
            for r in range(args.rounds):
                order = list(zip(names, arms))
                for k, (c, a) in (order if r % 2 == 0 else order[::-1]):
                    it[k].append(c.ask(f"time {a} {ITERS}")["ms"])
            result["per_iteration_ms"] = {k: stats(v) for k, v in it.items()}
            result["iterations_per_window"] = ITERS
    finally:
        new.close()
        if old is not None:
            old.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
