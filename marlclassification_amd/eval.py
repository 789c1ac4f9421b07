"""``eval_main``: the reference's ``test`` mode (eval.py:15-87) on the HIP path - load ``marl.json``
and a state dict (reference checkpoints load as they are), run every image of an image-folder
dataset through ``run_episode_get_last_step`` and report the confusion matrix, per-class
precision and recall.  Images go up as uint8 (ToTensor inside the gather kernel)."""

import os
from os.path import exists, isdir, isfile

import torch as th
from torch.utils.data import DataLoader

from .config import EvalConfig, MainConfig, ModelConfig
from .core import EpisodeSampler
from .data import DevicePrefetcher, ImageFolderU8
from .metrics import ConfusionMeter, format_metric


def eval_main(main_config: MainConfig, eval_config: EvalConfig) -> ConfusionMeter:
    for what, path in (("JSON path", eval_config.json_path), ("State dict path", eval_config.state_dict_path)):
        assert exists(path), f'{what} "{path}" does not exist'
        assert isfile(path), f'"{path}" is not a file'
    if exists(eval_config.output_dir) and not isdir(eval_config.output_dir):
        raise NotADirectoryError(f'"{eval_config.output_dir}" is not a directory')
    os.makedirs(eval_config.output_dir, exist_ok=True)
    if not main_config.cuda:
        raise RuntimeError("this implementation only runs on the GPU: pass --cuda")
    device = th.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))

    dataset = ImageFolderU8(eval_config.dataset_path, img_size=eval_config.img_size)
    marl_config = ModelConfig.load_marl_config(eval_config.json_path)
    if eval_config.comm is not None:
        marl_config.comm = eval_config.comm
    if eval_config.comm_range is not None:
        marl_config.comm_range = eval_config.comm_range
    if eval_config.normalize is not None:  # (--normalize SPEC|none: replaces what marl.json names)
        marl_config.normalize = None if eval_config.normalize == "none" else eval_config.normalize
    nn_models, marl_m, env = marl_config.build_marl(main_config.nb_agent)
    nn_models.load_state_dict(th.load(eval_config.state_dict_path, map_location="cpu"))
    nn_models.eval()
    nn_models.to(device)
    if eval_config.greedy or eval_config.temperature != 1.0:  # (--greedy: two runs of one checkpoint report the same)
        nn_models.set_exploration(temperature=eval_config.temperature, greedy=eval_config.greedy)
    loader = DevicePrefetcher(DataLoader(dataset, batch_size=eval_config.batch_size, shuffle=True,
                                         num_workers=0, drop_last=False, pin_memory=True), device)
    normalize = None
    if marl_config.normalize is not None:
        from . import transforms as _transforms

        normalize = _transforms.resolve(marl_config.normalize)
    sampler = EpisodeSampler(marl_m, env, main_config.step)
    meter = ConfusionMeter(nn_models.nb_class)
    views = view_mats = None
    if eval_config.tta is not None:  # (--tta: one episode per flip / rotation of the spec, predictions averaged)
        from . import augment as _augment

        policy = _augment.parse_tta(eval_config.tta)
        policy.check_size(eval_config.img_size, eval_config.img_size)
        views = policy.views().to(device)
        if policy.has_warp:  # (zoom:Z1/Z2/...: every code under every zoom, through the resampling gather)
            views, view_mats = (t.to(device) for t in policy.warp_views())

    def normalized(x):
        """the batch as the episode takes it: under marl.json's transform, each view with its own statistics"""
        return x if normalize is None else _transforms.apply(x, None, normalize)

    def view_of(x, v):
        ops = views[v: v + 1].expand(x.shape[0], -1).contiguous()
        if view_mats is None:
            return normalized(_augment.apply(x, None, ops))
        from . import warp as _warp

        return normalized(_warp.apply(x, None, view_mats[v: v + 1].expand(x.shape[0], -1).contiguous(), ops))

    rep = None
    if eval_config.report:  # (--report: every step of every episode into an episode report, report.py)
        from .report import EpisodeReport, ReportOptions, parse_exit_at, step_table

        opts = ReportOptions(eval_config.report_topk, eval_config.report_bins, parse_exit_at(eval_config.exit_at))
        n_views = 1 if views is None else views.shape[0]
        # (under --tta the views are stacked along the agent axis: the vote is the mean over views x agents)
        rep = EpisodeReport(main_config.step, main_config.nb_agent * n_views, nn_models.nb_class, opts, device)
        with th.no_grad():
            for x, y in loader:
                if n_views == 1 and view_mats is None:
                    preds = sampler.run_episode(normalized(x)).step_preds
                else:
                    preds = th.cat([sampler.run_episode(view_of(x, v)).step_preds for v in range(n_views)], dim=1)
                rep.add(preds, y.to(device))
        meter = rep  # (it has the meter's reading methods)
    with th.no_grad():
        for x, y in (() if rep is not None else loader):
            if views is None or (views.shape[0] == 1 and view_mats is None):
                out = sampler.run_episode_get_last_step(normalized(x))
                meter.add(out.prediction.mean(dim=0), y)  # mean over agents; stays on the device
                continue
            pred = None
            for v in range(views.shape[0]):
                p = sampler.run_episode_get_last_step(view_of(x, v)).prediction.mean(dim=0)
                pred = p if pred is None else pred + p
            meter.add(pred / views.shape[0], y)

    print(meter.conf_mat().cpu())
    precs, recs = meter.precision(), meter.recall()
    print(f"Precision : {format_metric(precs, dataset.class_to_idx)}")
    print(f"Precision mean = {precs.mean().item()}")
    print(f"Recall : {format_metric(recs, dataset.class_to_idx)}")
    print(f"Recall mean : {recs.mean().item()}")
    meter.save_conf_matrix(0, eval_config.output_dir, "test")
    if rep is not None:
        for line in step_table(rep.result(), opts):
            print(line)
        rep.to_json(os.path.join(eval_config.output_dir, "report.json"))
        rep.save_step_curve(os.path.join(eval_config.output_dir, "accuracy_per_step.png"))
    return meter
