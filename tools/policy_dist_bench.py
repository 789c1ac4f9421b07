"""Cost of the action distributions at C3 shapes, alternating rounds on one box:
  (a) Trainer.train_step with entropy_coef = 0.01 against entropy_coef = 0 (the plain entries),
  (b) one autograd iteration (EpisodeSampler.run_episode + loss.backward()) with return_probs on against off,
plus the HBM-bound estimate of the added work: three passes over Ns * R * nA floats (the loss reads the
probabilities and writes g_probs, the backward's logit kernel reads both) and the copy into step_probs.  Prints one
JSON line.  The added launches' own durations come from a rocprofv3 kernel trace of this script
(tools/rocpd_stats.py; kernels copy2d_kernel, loss_grads_kernel<true, ...>, policy_dlogits_probs_v4_kernel).
usage: python tools/policy_dist_bench.py [--batch 256] [--iters 10] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

import torch as th

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench import C3, IMG, NA, NS  # noqa: E402
from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent  # noqa: E402
from marlclassification_amd.networks import ModelsWrapper  # noqa: E402
from marlclassification_amd.networks.vision import CNN_BY_NAME  # noqa: E402
from marlclassification_amd.training import Trainer  # noqa: E402

COPY_GBS = 6290.0  # what a float4 copy reaches on this part
ACTIONS = [[1, 0], [-1, 0], [0, 1], [0, -1]]


def _model(dev):
    th.manual_seed(0)
    return ModelsWrapper(CNN_BY_NAME[C3["ft_extr"]](C3["window"]), C3["n_b"], C3["n_a"], C3["n_m"], C3["n_m_o"],
                         C3["n_d"], 2, len(ACTIONS), C3["nb_class"], C3["nlb"], C3["nla"]).to(dev)


def _alternate(fns, iters, rounds):
    times = {k: [] for k in fns}
    for f in fns.values():
        f()
    for _ in range(rounds):
        for k, f in fns.items():
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                f()
            th.cuda.synchronize()
            times[k].append(round(1e3 * (time.perf_counter() - t0) / iters, 3))
    return times


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = th.device("cuda", 0)
    nb = args.batch
    img = th.rand(nb, *IMG, device=dev)
    y = th.randint(C3["nb_class"], (nb,), device=dev)

    # (a) the fused trainer, one model per coefficient (each has its own Adam state)
    steps = {}
    for beta in (0.0, 0.01):
        model = _model(dev)
        sampler = EpisodeSampler(MultiAgent(NA, model), Environment(ACTIONS, C3["window"]), NS)
        trainer = Trainer(model, C3["nb_class"], 1e-4, 0.99, entropy_coef=beta)
        steps[f"entropy_coef_{beta:g}"] = (lambda t=trainer, s=sampler: t.train_step(img, y, s))
    trainer_ms = _alternate(steps, args.iters, args.rounds)

    # (b) the autograd node
    model = _model(dev)
    sampler = EpisodeSampler(MultiAgent(NA, model), Environment(ACTIONS, C3["window"]), NS)

    def iteration(probs: bool) -> None:
        sampler.return_probs = probs
        out = sampler.run_episode(img)
        loss = out.step_preds.square().mean() - out.step_log_probas.mean() + out.step_values.square().mean()
        if probs:
            loss = loss + out.step_probs.square().mean()
        loss.backward()

    autograd_ms = _alternate({"return_probs_off": lambda: iteration(False), "return_probs_on": lambda: iteration(True)},
                             args.iters, args.rounds)

    pass_bytes = NS * NA * nb * len(ACTIONS) * 4
    us = lambda nbytes: round(nbytes / (COPY_GBS * 1e3), 2)  # noqa: E731
    print(json.dumps({
        "shape": f"C3 Na={NA} Ns={NS} Nb={nb} img={list(IMG)} nA={len(ACTIONS)}",
        "trainer_train_step_ms": trainer_ms,
        "autograd_iteration_ms": autograd_ms,
        "bytes_per_pass_over_the_distributions": pass_bytes,
        "added_traffic": {
            "forward_copy_read_write": 2 * pass_bytes,
            "loss_read_probs_write_g_probs": 2 * pass_bytes,
            "backward_logit_kernel_read_g_probs": pass_bytes,
        },
        "added_traffic_hbm_bound_us": {"forward": us(2 * pass_bytes), "loss": us(2 * pass_bytes),
                                       "backward": us(pass_bytes)},
        "added_launches": {"forward": 1, "loss": 0, "backward": 0},
        "copy_gbs": COPY_GBS,
    }))


if __name__ == "__main__":
    main()
