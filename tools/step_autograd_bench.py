"""Per-step autograd (MultiAgent.act in a Python loop, one marl_step_forward_train / marl_step_backward node per
step) next to the fused episode node (EpisodeSampler, one marl_episode_forward / marl_episode_backward) at C3
shapes: forward + loss.backward() of one 16-step episode, same loss on (preds, logp, values).  Also prints the
bytes of saved state per live step (the one-step training workspace).
usage: python tools/step_autograd_bench.py [--batch 256] [--iters 10]"""
import argparse
import os
import sys
import time

import torch as th

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bench import C3, IMG, NA, NS  # noqa: E402
from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent  # noqa: E402
from marlclassification_amd.networks import ModelsWrapper  # noqa: E402
from marlclassification_amd.networks.vision import CNN_BY_NAME  # noqa: E402


def loss_of(preds, logp, values):
    return preds.square().mean() - logp.mean() + values.square().mean()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    dev = th.device("cuda", 0)
    actions = [[1, 0], [-1, 0], [0, 1], [0, -1]]
    th.manual_seed(0)
    model = ModelsWrapper(CNN_BY_NAME[C3["ft_extr"]](C3["window"]), C3["n_b"], C3["n_a"], C3["n_m"], C3["n_m_o"],
                          C3["n_d"], 2, len(actions), C3["nb_class"], C3["nlb"], C3["nla"]).to(dev)
    nb = args.batch
    img = th.rand(nb, *IMG, device=dev)
    sampler = EpisodeSampler(MultiAgent(NA, model), Environment(actions, C3["window"]), NS)
    agents, env = MultiAgent(NA, model, stream_id=2), Environment(actions, C3["window"])

    def fused():
        out = sampler.run_episode(img)
        loss_of(out.step_preds, out.step_log_probas, out.step_values).backward()

    def per_step():
        obs = env.reset(img, NA)
        agents.reset(nb)
        preds, logp, values = [], [], []
        for _ in range(NS):
            o = agents.act(obs, env.normalized_positions)
            obs = env.step(o.actions)
            preds.append(o.predictions)
            logp.append(o.actions_log_probs)
            values.append(o.values)
        loss_of(th.stack(preds), th.stack(logp), th.stack(values)).backward()

    res = {}
    for name, fn in (("fused episode", fused), ("per-step act loop", per_step)):
        for _ in range(2):
            fn()
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        th.cuda.synchronize()
        res[name] = 1e3 * (time.perf_counter() - t0) / args.iters
        model.zero_grad(set_to_none=True)
    eng = model.hip_engine(None)
    eng.configure(NA, nb, 1, (IMG[0], C3["window"] + 1, C3["window"] + 1))
    ws_bytes = eng._sizes(True)[1]
    print(f"C3 shapes, Na={NA} Nb={nb} Ns={NS}: forward + backward of one episode")
    for name, ms in res.items():
        print(f"  {name:18s} {ms:8.3f} ms  ({ms / NS:.3f} ms per step)")
    print(f"  saved state per live step (one-step training workspace): {ws_bytes / 2**20:.1f} MiB")


if __name__ == "__main__":
    main()
