"""``train_main``: the reference's training driver (train.py:18-168) on the HIP path -
same configs, same output tree (``marl.json``, ``class_to_idx.json``,
``models/nn_models_epoch_{e}.pt`` with reference state-dict keys).  MLflow is optional (not
installed here); images are uploaded as uint8 (data.py).  Multi-GPU: launch with
``torchrun --nproc-per-node N -m marlclassification_amd ...``; every rank trains on its
shard of each batch and gradients are all-reduced over RCCL."""

import json
import os
from os.path import exists, isdir, join
from typing import Dict, Optional

import torch as th
from torch.utils.data import DataLoader, Sampler

from .config import MainConfig, ModelConfig, TrainConfig
from .core import EpisodeSampler
from .data import DevicePrefetcher, ImageFolderU8, ResidentLoader, StripedLoader, SyntheticImages
from .parallel import BucketedGradAllReduce
from .training import Trainer


# where each image-folder dataset lives under the resources directory (reference
# data/datasets.py:25-79,217-235: MnistDataset / Resisc45Dataset / AidDataset / SkinCancerDataset)
_DATASET_SUBDIR = {
    "mnist": ("downloaded", "mnist_png", "all_png"),
    "resisc45": ("downloaded", "NWPU-RESISC45"),
    "aid": ("downloaded", "AID"),
    "skin_cancer": ("downloaded", "skin_cancer"),
}


def _dataset(model_config: ModelConfig, train_config: TrainConfig):
    """``--res-folder synthetic`` (explicit) = random images of the configured shape; anything else
    must be the reference's resources directory: the dataset is read from the same sub-folder
    the reference's dataset class uses, and a missing folder is an error (never silent noise)."""
    root = train_config.resources_dir
    if root == "synthetic":
        channels = 1 if model_config.ft_extr_str == "mnist" else 3
        return SyntheticImages(max(4 * train_config.batch_size, 64), channels, train_config.img_size,
                               model_config.nb_class)
    sub = _DATASET_SUBDIR.get(model_config.ft_extr_str)
    if sub is None:
        raise ValueError(f'no image-folder dataset is known for "{model_config.ft_extr_str}" '
                         f"(supported: {sorted(_DATASET_SUBDIR)}, or --res-folder synthetic)")
    path = join(root, *sub)
    if not (exists(path) and isdir(path)):
        raise NotADirectoryError(f'"{path}" does not exist or is not a directory '
                                 "(pass the reference's resources folder, or --res-folder synthetic)")
    dataset = ImageFolderU8(path, img_size=train_config.img_size)
    if len(dataset) == 0 or len(dataset.class_to_idx) != model_config.nb_class:
        raise ValueError(f'"{path}": {len(dataset)} images in {len(dataset.class_to_idx)} classes, '
                         f"--nb-class is {model_config.nb_class}")
    return dataset


def _split_spec(dataset, indices, device, chunk: int = 256):
    """``--normalize dataset``: the mean / std of the images ``indices`` of ``dataset`` as a ``user-normal`` Spec
    (``transforms.dataset_spec`` over uploaded chunks: the statistics are taken on the device, summed in integers)"""
    from . import transforms as _transforms

    def chunks():
        for at in range(0, len(indices), chunk):
            yield th.stack([dataset[i][0] for i in indices[at: at + chunk]]).to(device)

    return _transforms.dataset_spec_of(chunks())


def _split_labels(dataset, indices) -> th.Tensor:
    """The labels of ``indices`` without decoding an image (both dataset classes keep them in memory)."""
    if isinstance(dataset, SyntheticImages):
        return dataset.y[th.as_tensor(indices, dtype=th.int64)]
    if isinstance(dataset, ImageFolderU8):
        return th.tensor([dataset.items[i][1] for i in indices], dtype=th.int64)
    return th.tensor([int(dataset[i][1]) for i in indices], dtype=th.int64)


class ShardedBatchSampler(Sampler):
    """Batches of dataset INDICES for one rank.  Every rank derives the same shuffled order of
    the same index list from (seed, epoch) and takes its contiguous slice of every global batch,
    so a rank only decodes the images it trains on (the reference has one process and 6 loader
    workers, train.py:91-107; slicing after the decode would repeat the host work on every
    rank).  The last, smaller global batch is trimmed to a multiple of the world size."""

    def __init__(self, indices, global_batch: int, rank: int, world: int, shuffle: bool, seed: int) -> None:
        if global_batch % world != 0:
            raise ValueError(f"batch size {global_batch} is not divisible by the world size {world}")
        self.indices = list(indices)
        self.global_batch, self.rank, self.world = global_batch, rank, world
        self.shuffle, self.seed, self.epoch = shuffle, seed, 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def _batches(self):
        order = self.indices
        if self.shuffle:
            g = th.Generator().manual_seed(self.seed * 1_000_003 + self.epoch)
            order = [self.indices[i] for i in th.randperm(len(order), generator=g).tolist()]
        for lo in range(0, len(order), self.global_batch):
            chunk = order[lo: lo + self.global_batch]
            n = (len(chunk) // self.world) * self.world
            if n == 0:
                continue
            per = n // self.world
            yield chunk[self.rank * per: (self.rank + 1) * per]

    def __iter__(self):
        return self._batches()

    def __len__(self) -> int:
        full, rest = divmod(len(self.indices), self.global_batch)
        return full + (1 if rest >= self.world else 0)


def loader_workers(dataset) -> int:
    """Decode processes per rank: the reference uses 6 (train.py:95); MARL_LOADER_WORKERS
    overrides; in-memory synthetic data needs none."""
    if isinstance(dataset, SyntheticImages):
        return 0
    env = os.environ.get("MARL_LOADER_WORKERS")
    if env is not None:
        return max(0, int(env))
    return max(0, min(6, (os.cpu_count() or 1) - 1))


def resident_fits(dataset) -> bool:
    """Keep the decoded uint8 image set in HBM (data.ResidentLoader) when it is an image
    folder no larger than MARL_RESIDENT_GB (default 64; 0 = always stream from the loader)."""
    if not isinstance(dataset, ImageFolderU8) or len(dataset) == 0:
        return False
    budget = float(os.environ.get("MARL_RESIDENT_GB", "64")) * 1e9
    # peak while the shards are exchanged: this rank's 1/world + the gathered whole (data.ResidentLoader._fill)
    import torch.distributed as dist

    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    return ResidentLoader.nbytes(dataset, len(dataset)) * (1.0 + (1.0 / world if world > 1 else 0.0)) <= budget


def train_main(main_config: MainConfig, model_config: ModelConfig, train_config: TrainConfig,
               metric_logger=None, exact_standardize: bool = False) -> Trainer:
    """``exact_standardize`` (multi-GPU): one extra 3-double all-reduce per iteration makes the
    advantage standardisation global, so the update equals the single-GPU big-batch update."""
    assert model_config.state_dim == 2, "the HIP path implements 2-D images (state_dim == 2)"
    output_dir = train_config.output_dir
    model_dir = join(output_dir, "models")
    os.makedirs(model_dir, exist_ok=True)
    if not isdir(model_dir):
        raise NotADirectoryError(f'"{model_dir}" is not a directory.')
    if not main_config.cuda:
        raise RuntimeError("this implementation only runs on the GPU: pass --cuda")

    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # launched by torch.distributed.run (any world size: one rank still goes through RCCL, so
    # the exact command line of a multi-GPU run is what a 1-GPU box tests)
    distributed = "RANK" in os.environ
    device = th.device("cuda", local_rank)
    th.cuda.set_device(device)
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        dist.init_process_group("nccl", device_id=device)
    # one base seed for the run: identical initial weights and data order on every rank; the episode draws
    # mix the rank in (core/episode.py), so shards draw differently.  MARL_SEED unset: a fresh seed per run
    # like the reference (train.py never seeds), agreed on by all ranks; it is printed, so a run can be
    # repeated with MARL_SEED=<that value>.
    # --resume: the trainer state of a checkpoint epoch; it names the run's seed (data order, generator streams)
    resumed = None
    if train_config.resume is not None:
        resumed = th.load(train_config.resume, map_location="cpu", weights_only=True)
        for k in ("epoch", "base_seed"):
            if k not in resumed:
                raise ValueError(f'"{train_config.resume}" is no trainer checkpoint of this program (no {k})')
    if resumed is not None:
        base_seed = int(resumed["base_seed"])
    elif "MARL_SEED" in os.environ:
        base_seed = int(os.environ["MARL_SEED"])
    else:
        t = th.tensor([int.from_bytes(os.urandom(4), "little")], dtype=th.int64, device=device)
        if distributed:
            dist.broadcast(t, 0)
        base_seed = int(t.item())
    th.manual_seed(base_seed)
    if rank == 0:
        print(f"seed {base_seed}, world size {world}", flush=True)

    nn_models, marl_m, env = model_config.build_marl(main_config.nb_agent)
    dataset = _dataset(model_config, train_config)
    g = th.Generator().manual_seed(base_seed)  # same split on every rank
    idx = th.randperm(len(dataset), generator=g)
    cut = int(0.85 * idx.shape[0])
    # --normalize: part of the model (marl.json).  `dataset` is resolved here, on the whole training split before the
    # per-rank sharding - every rank computes the same integers - and stored as the user-normal:... it stands for
    normalize = None
    if model_config.normalize is not None:
        from . import transforms as _transforms

        if model_config.normalize == "dataset":
            model_config.normalize = _split_spec(dataset, idx[:cut].tolist(), device).spelling
        normalize = _transforms.resolve(model_config.normalize)
    if rank == 0:
        model_config.save_marl_config(join(output_dir, "marl.json"))
        with open(join(output_dir, "class_to_idx.json"), "w", encoding="utf-8") as f:
            json.dump(dataset.class_to_idx, f)
    nn_models.to(device)
    learned = None
    if train_config.learn_comm:
        # the graph is learned: row-softmax weights over the support of --comm (deterministic initial logits:
        # identical on every rank, and d_comm is averaged over the ranks, so they stay identical)
        from . import comm as _comm

        init = _comm.parse(model_config.comm or "full", main_config.nb_agent)
        if not bool((init != 0).any()):
            raise ValueError(f'--learn-comm: the graph "{model_config.comm}" has no link to learn on')
        learned = _comm.LearnableComm(init).to(device)
        nn_models.set_comm(learned)
    if distributed:  # identical initial weights on every rank
        for p in nn_models.parameters():
            dist.broadcast(p.data, src=0)

    # --class-weights: `balanced` counts the labels of the WHOLE training split (before the per-rank sharding: every
    # rank gets the same weights); a file or a list is checked against the class count
    from . import class_loss as _class_loss

    class_weights = _class_loss.resolve_class_weights(
        train_config.class_weights, model_config.nb_class,
        _split_labels(dataset, idx[:cut].tolist()) if train_config.class_weights == "balanced" else None)
    if train_config.error_steps is not None:
        _class_loss.step_schedule(train_config.error_steps, main_config.step)  # (last:K against --step)
    loaders, samplers = [], []
    workers = loader_workers(dataset)
    resident = resident_fits(dataset)
    if rank == 0:
        print(f"input pipeline: {'HBM-resident uint8 image set' if resident else 'streamed'}, "
              f"{workers} decode processes per rank", flush=True)
    # --augment: the training split only (loaders[1] stays plain); ops are drawn on the device from a generator of
    # its own, seeded per rank, so ranks draw differently and MARL_SEED repeats a run
    policy = aug_gen = None
    if train_config.augment is not None:
        from . import augment as _augment

        policy = _augment.parse(train_config.augment)
        policy.check_size(train_config.img_size, train_config.img_size)
        aug_gen = th.Generator(device=device).manual_seed(base_seed + 104729 * (rank + 1))
    # --mix: likewise the training split only, drawn from the same per-rank device generator (behind the ops)
    mix_policy = None
    if train_config.mix is not None:
        from . import mix as _mix

        mix_policy = _mix.parse(train_config.mix)
        if aug_gen is None:
            aug_gen = th.Generator(device=device).manual_seed(base_seed + 104729 * (rank + 1))
    # --color: likewise the training split only, drawn last from the same per-rank device generator
    color_policy = None
    if train_config.color is not None:
        from . import color as _color

        color_policy = _color.parse(train_config.color)
        if aug_gen is None:
            aug_gen = th.Generator(device=device).manual_seed(base_seed + 104729 * (rank + 1))
    for k, part in enumerate((idx[:cut].tolist(), idx[cut:].tolist())):
        aug = {"augment": policy, "generator": aug_gen} if policy is not None and k == 0 else {}
        if color_policy is not None and k == 0:
            aug.update(color=color_policy, generator=aug_gen)
        if mix_policy is not None and k == 0:
            aug.update(mix=mix_policy, nb_class=model_config.nb_class, generator=aug_gen)
        if normalize is not None:  # (both splits: the evaluation sees what the model was trained on)
            aug["normalize"] = normalize
        bs = ShardedBatchSampler(part, train_config.batch_size, rank, world, shuffle=True,
                                 seed=base_seed + 1 + k)
        samplers.append(bs)
        if resident:  # decoded once (1/world per rank), then batches are row gathers in HBM
            loaders.append(ResidentLoader(dataset, part, bs, device, workers=workers, rank=rank, world=world, **aug))
            continue
        # (MARL_LOADER_STRIPES DataLoaders share the workers: one collate / pin thread each, data.StripedLoader)
        dl = StripedLoader(dataset, bs, workers, int(os.environ.get("MARL_LOADER_STRIPES", max(1, workers // 8))))
        loaders.append(DevicePrefetcher(dl, device, **aug))  # upload of batch i+1 overlaps step i

    sampler = EpisodeSampler(marl_m, env, main_config.step)
    # the flat optimiser step (optim.py): any of its flags makes every update a marl_optim_step; none: plain Adam
    optim_opts = None
    if train_config.optim_on():
        from . import optim as _optim

        total_steps = train_config.nb_epoch * len(samplers[0]) * train_config.ppo_epochs
        optim_opts = _optim.OptimOptions(
            weight_decay=train_config.weight_decay, decay="all" if train_config.decay_all else "matrices",
            groups=_optim.parse_groups(train_config.lr_groups or ""),
            betas=train_config.adam_betas or (0.9, 0.999),
            schedule=_optim.parse_schedule(train_config.lr_schedule or "constant", train_config.warmup_steps,
                                           max(total_steps, train_config.warmup_steps),
                                           train_config.learning_rate),
            ema_decay=train_config.ema)
    if train_config.eval_ema and train_config.ema is None:
        raise ValueError("--eval-ema needs --ema")
    report_opts = None
    if train_config.report:  # (--report: the training meter and the evaluation are episode reports, report.py)
        from .report import EpisodeReport, ReportOptions, parse_exit_at, summary_metrics

        report_opts = ReportOptions(train_config.report_topk, train_config.report_bins,
                                    parse_exit_at(train_config.exit_at))
    trainer = Trainer(nn_models, marl_m.nb_class, train_config.learning_rate, train_config.gamma,
                      report=report_opts,
                      metric_logger=metric_logger if rank == 0 else None,
                      allreduce=(BucketedGradAllReduce(world, None, nn_models.flat_state().offsets, nn_models.flat_state().numel,
                                                      device) if distributed else None),
                      exact_standardize_group=(dist.group.WORLD if distributed and world > 1 and
                                               exact_standardize else None),
                      entropy_coef=train_config.entropy_coef, ppo_epochs=train_config.ppo_epochs,
                      ppo_clip=train_config.ppo_clip, gae_lambda=train_config.gae_lambda,
                      max_grad_norm=train_config.max_grad_norm,
                      comm_lr=((train_config.comm_lr if train_config.comm_lr is not None else
                                train_config.learning_rate) if learned is not None else None),
                      class_weights=class_weights, label_smoothing=train_config.label_smoothing,
                      error_step_weights=train_config.error_steps, weight_rewards=train_config.weight_rewards,
                      optim=optim_opts)
    first_epoch = 0
    if resumed is not None:
        first_epoch = int(resumed["epoch"]) + 1
        weights = join(os.path.dirname(os.path.abspath(train_config.resume)),
                       f"nn_models_epoch_{first_epoch - 1}.pt")
        nn_models.load_state_dict(th.load(weights, map_location=device, weights_only=True))
        trainer.load_state_dict(resumed, sampler)
        if rank == 0:
            print(f"resumed from epoch {first_epoch - 1}: optimiser step {nn_models.flat_state().step}", flush=True)
    from . import explore as _explore

    t_ends, e_ends, cw_spec = train_config.temperature, train_config.explore_eps, train_config.class_weights
    if rank == 0:
        print("update: " + ", ".join(f"{k}={getattr(train_config, k)}" for k in (
            "entropy_coef", "ppo_epochs", "ppo_clip", "gae_lambda", "max_grad_norm")) +
              (f", learn_comm on {model_config.comm or 'full'}" if learned is not None else "") +
              (f", temperature {t_ends}, explore_eps {e_ends}" if t_ends or e_ends else "") +
              (f", normalize {model_config.normalize}" if normalize is not None else "") +
              (f", augment {policy.spec}" if policy is not None else "") +
              (f", mix {mix_policy.spec}" if mix_policy is not None else "") +
              (f", color {color_policy.spec}" if color_policy is not None else "") +
              (f", class weights {cw_spec if isinstance(cw_spec, str) else 'given'}" if cw_spec is not None else "") +
              (f", label_smoothing {train_config.label_smoothing}" if train_config.label_smoothing else "") +
              (f", error steps {train_config.error_steps}" if train_config.error_steps else "") +
              (", weighted rewards" if train_config.weight_rewards else "") +
              (f", optim {trainer.optim_options.fingerprint()}" if optim_opts is not None else ""), flush=True)
    for e in range(first_epoch, train_config.nb_epoch):
        for bs in samplers:
            bs.set_epoch(e)
        if t_ends is not None:  # (the exploration schedules: linear over the epochs, applied at each epoch's start)
            trainer.temperature = _explore.schedule_value(t_ends, e, train_config.nb_epoch)
        if e_ends is not None:
            trainer.explore_eps = _explore.schedule_value(e_ends, e, train_config.nb_epoch)
        trainer.train_epoch(loaders[0], e, sampler)
        eval_kw = {}
        if report_opts is not None:
            eval_kw["report"] = EpisodeReport(main_config.step, main_config.nb_agent, marl_m.nb_class, report_opts,
                                              device)
        if train_config.eval_ema:
            with trainer.ema_weights():
                conf = trainer.eval_epoch(loaders[1], e, sampler, **eval_kw)
        else:
            conf = trainer.eval_epoch(loaders[1], e, sampler, **eval_kw)
        if distributed:
            conf.all_reduce()  # every rank evaluated its shard only
        if rank == 0:
            m: Dict[str, float] = trainer.metrics()
            m["eval_prec"] = conf.precision().mean().item()
            m["eval_recs"] = conf.recall().mean().item()
            if report_opts is not None:
                m.update(summary_metrics(conf.result(), report_opts, "eval"))
                conf.to_json(join(output_dir, f"report_epoch_{e}.json"))
                conf.save_step_curve(join(output_dir, f"accuracy_per_step_epoch_{e}.png"))
            print(f"epoch {e}: " + ", ".join(f"{k}={v:.8e}" if k == "lr" else f"{k}={v:.4f}" for k, v in m.items()),
                  flush=True)
            conf.save_conf_matrix(e, output_dir, "eval")  # reference train.py:134
            th.save(nn_models.state_dict(), join(model_dir, f"nn_models_epoch_{e}.pt"))
            # what --resume continues from (rank 0's generator position: a multi-GPU run resumes its ranks from it)
            state = trainer.state_dict(sampler)
            state["epoch"], state["base_seed"] = e, base_seed
            th.save(state, join(model_dir, f"trainer_epoch_{e}.pt"))
            if train_config.ema is not None:  # (reference state-dict keys: test / infer load it as it is)
                with trainer.ema_weights():
                    th.save(nn_models.state_dict(), join(model_dir, f"nn_models_ema_epoch_{e}.pt"))
            if learned is not None:  # the learned matrix: `test` / `infer` load it with --comm FILE.npy
                import numpy as np

                np.save(join(model_dir, f"comm_epoch_{e}.npy"), learned.to_matrix().numpy())
    if rank == 0 and len(idx) > cut:
        # one evaluation image, step by step (reference train.py:149-166): frames + GIF in output_dir
        from .visualization import visualize_steps

        pick = int(idx[cut + int(th.randint(0, len(idx) - cut, (1,)).item())])
        x_u8 = dataset[pick][0]
        x_in = x_u8.to(device)
        if normalize is not None:  # (the episode sees the normalised image; the frames paint the original)
            x_in = _transforms.apply(x_in.unsqueeze(0).contiguous(), None, normalize)[0]
        visualize_steps(sampler, x_in, x_u8, model_config.window_size, output_dir, dataset.class_to_idx)
    if distributed:
        dist.destroy_process_group()
    return trainer
