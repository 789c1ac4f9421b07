"""Cost of the image gradient at C3 shapes: one autograd iteration (EpisodeSampler.run_episode + loss.backward())
with and without the image requiring grad, alternating, plus the HBM-bound estimate of the image-gradient launch
(dZ_0 read once, d_img written once).  Prints one JSON line.  The kernel's own time comes from a rocprofv3
kernel trace of this script (tools/rocpd_stats.py; kernel name cnn_dimg_kernel).
usage: python tools/pixel_grad_bench.py [--batch 256] [--iters 10] [--rounds 3]"""
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

HBM_PEAK_GBS = 8000.0  # spec; a float4 copy measures 6290 GB/s on this part


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = th.device("cuda", 0)
    actions = [[1, 0], [-1, 0], [0, 1], [0, -1]]
    th.manual_seed(0)
    model = ModelsWrapper(CNN_BY_NAME[C3["ft_extr"]](C3["window"]), C3["n_b"], C3["n_a"], C3["n_m"], C3["n_m_o"],
                          C3["n_d"], 2, len(actions), C3["nb_class"], C3["nlb"], C3["nla"]).to(dev)
    nb = args.batch
    img = th.rand(nb, *IMG, device=dev)
    sampler = EpisodeSampler(MultiAgent(NA, model), Environment(actions, C3["window"]), NS)

    def iteration(with_img: bool) -> None:
        x = img.detach().requires_grad_(with_img)
        out = sampler.run_episode(x)
        (out.step_preds.square().mean() - out.step_log_probas.mean() + out.step_values.square().mean()).backward()

    times = {False: [], True: []}
    for flag in (False, True):
        iteration(flag)
    for _ in range(args.rounds):
        for flag in (False, True):
            th.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                iteration(flag)
            th.cuda.synchronize()
            times[flag].append(1e3 * (time.perf_counter() - t0) / args.iters)
    f = C3["window"]
    hout = (f - 1) // 2 + 1
    cout = 16  # layer 0 of the RESISC45 extractor
    dz0 = NS * NA * nb * hout * hout * cout * 4
    dimg = nb * IMG[0] * IMG[1] * IMG[2] * 4
    print(json.dumps({
        "shape": f"C3 Na={NA} Ns={NS} Nb={nb} img={list(IMG)} f={f}",
        "ms_per_iteration_params_only": [round(t, 3) for t in times[False]],
        "ms_per_iteration_with_image_grad": [round(t, 3) for t in times[True]],
        "dimg_kernel_bytes": {"dz0_read": dz0, "d_img_write": dimg, "total": dz0 + dimg},
        "dimg_kernel_hbm_bound_us": round((dz0 + dimg) / (HBM_PEAK_GBS * 1e3), 1),
        "hbm_peak_gbs": HBM_PEAK_GBS,
    }))


if __name__ == "__main__":
    main()
