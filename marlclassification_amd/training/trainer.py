"""Trainer: the A2C loop of the reference (training/trainer.py) on the HIP path.

One training iteration is: ``marl_episode_forward`` (all steps) -> ``marl_a2c_loss_fwd_bwd``
(loss + dL/d outputs) -> ``marl_episode_backward`` (BPTT, every parameter gradient) ->
[one RCCL all-reduce of the flat gradient buffer] -> ``marl_adam_step`` -> re-pack.  No host
synchronisation happens inside an iteration; meters are read every ``log_interval`` steps.
With a PPO option off its default (``ppo_epochs``, ``ppo_clip``, ``gae_lambda``, ``max_grad_norm``) one rollout
feeds K updates: ``marl_advantages`` once, then per epoch [replay forward] -> ``marl_ppo_loss_fwd_bwd`` -> backward
-> [all-reduce] -> [``marl_grad_clip``] -> Adam -> re-pack.
Same constructor and ``train_epoch`` / ``eval_epoch`` signatures as the reference.
"""

from contextlib import contextmanager
from typing import Callable, Dict, Iterable, Optional, Tuple

import torch as th

from ..core import EpisodeSampler
from ..engine import EpisodeTensors
from ..fused import (ClassLossOptions, CommUpdate, OptimRun, apply_update, check_ppo_options, comm_update_for, ppo_bufs_fit,
                     ppo_epochs_loop, ppo_options_on, soft_targets_installed)
from ..metrics import ConfusionMeter, LossMeter
from ..networks import ModelsWrapper

MetricLogger = Callable[[int, Dict[str, float]], None]


class Trainer:
    def __init__(
        self,
        model: ModelsWrapper,
        nb_class: int,
        learning_rate: float,
        gamma: float,
        metric_logger: Optional[MetricLogger] = None,
        log_interval: int = 100,
        meter_window_size: int = 64,
        allreduce: Optional[Callable[[th.Tensor], float]] = None,
        exact_standardize_group=None,
        entropy_coef: float = 0.0,
        ppo_epochs: int = 1,
        ppo_clip: float = 0.2,
        gae_lambda: float = 1.0,
        max_grad_norm: Optional[float] = None,
        comm_lr: Optional[float] = None,
        temperature: Optional[float] = None,
        explore_eps: Optional[float] = None,
        class_weights=None,
        label_smoothing: float = 0.0,
        error_step_weights=None,
        weight_rewards: bool = False,
        optim=None,
        report=None,
    ) -> None:
        """``report`` (a ``report.ReportOptions``): the per-iteration training meter is a windowed
        ``report.EpisodeReport`` (``meter_window_size`` batches) that every ``train_step`` feeds from ALL of the
        rollout's ``step_preds`` with one ``marl_episode_report`` call, in place of ``ConfusionMeter.add`` on the last
        step's vote; ``metrics()`` gains ``train_acc``, ``train_top{k}``, ``train_nll`` and ``train_ece``, and
        ``train_prec`` / ``train_rec`` come from the report's confusion matrix.  None: the confusion meter, as before.

        ``optim`` (an ``optim.OptimOptions``): every update - ``train_step`` with or without the entropy bonus, every
        PPO epoch, on every rank - is one ``marl_optim_step`` under these options: AdamW with decoupled weight decay,
        per-module learning-rate multipliers (0 freezes a module; with ``max_grad_norm`` its gradient leaves the
        clipped norm), a schedule whose base rate is ``learning_rate`` (unless it names its own) and, with
        ``ema_decay``, an averaged copy of the weights (``ema_weights()``).  ``metrics()["lr"]`` is the rate the last
        step applied, as the kernel wrote it.  None: ``marl_adam_step`` exactly as before.

        ``class_weights`` ([nb_class], >= 0) / ``label_smoothing`` (in [0, 1)) / ``error_step_weights`` (``all``,
        ``last``, ``last:K``, ``linear`` or one weight per step) / ``weight_rewards``: the options of the vote error and
        the rewards (``class_loss.py``: err[t,b] = s_t * weighted, smoothed cross-entropy of the vote; rewards times
        w_y) in ``train_step`` and in every PPO epoch: each step installs them on the model's engine
        (``HipEngine.set_class_loss``) around its loss calls and puts the engine's own setting back behind them, so a
        second trainer on the same model never inherits them.  All four at their defaults: the engine's own setting
        applies - without one the reference's loss, through today's sequence of calls.

        ``temperature`` / ``explore_eps``: the behaviour policy of the rollouts, (1 - eps) softmax(z / T) + eps / nA
        (``ModelsWrapper.set_exploration``; replays and PPO epochs run under the rollout's setting).  Plain
        attributes that may be changed between ``train_step``s; each ``train_step`` hands the values that are not
        None to the model (its ``greedy`` flag stays); None: the model's own setting is left alone.

        ``comm_lr``: learning rate of the model's LIVE communication source (``model.set_comm`` with a tensor that
        requires grad, a module such as ``comm.LearnableComm`` or a callable with ``parameters()``).  Each update then
        evaluates the source, rolls out, takes the loss, runs the backward WITH d_comm (marl_comm_grad), sums d_comm
        over the ranks with the scale the flat gradient gets, calls ``matrix.backward(d_comm)`` and steps a
        ``torch.optim.Adam(model.comm_parameters(), lr=comm_lr)`` - in ``train_step`` with or without the entropy bonus
        and in every PPO epoch (the source is evaluated again before every replay): ``fused.apply_update``.  None, or a
        constant matrix: ``episode_backward`` is called without ``d_comm`` and nothing more is launched.
        ``max_grad_norm`` keeps covering the flat parameter buffer only: the graph's leaves are not part of the
        clipped norm."""
        if not entropy_coef >= 0.0:
            raise ValueError(f"entropy_coef must be >= 0, got {entropy_coef}")
        check_ppo_options(ppo_epochs, ppo_clip, gae_lambda, max_grad_norm)
        if comm_lr is not None and not comm_lr > 0.0:
            raise ValueError(f"comm_lr must be > 0 or None, got {comm_lr}")
        from .. import explore as _explore

        _explore.check(1.0 if temperature is None else temperature, 0.0 if explore_eps is None else explore_eps)
        self.temperature, self.explore_eps = temperature, explore_eps
        if class_weights is not None and len(class_weights) != nb_class:
            raise ValueError(f"class_weights must have nb_class = {nb_class} entries, got {len(class_weights)}")
        self.__class_loss = ClassLossOptions(class_weights, label_smoothing, error_step_weights, weight_rewards)
        self.__optim: Optional[OptimRun] = None if optim is None else OptimRun(optim, learning_rate)
        self.__comm_pending: Optional[dict] = None  # (a loaded state of the communication source's Adam)
        self.__comm_lr = None if comm_lr is None else float(comm_lr)
        self.__comm_update: Optional[CommUpdate] = None
        self.__model = model
        self.__nb_class = nb_class
        self.__lr = learning_rate
        self.__gamma = gamma
        self.__metric_logger = metric_logger
        self.__log_interval = log_interval
        self.__allreduce = allreduce
        self.__exact_group = exact_standardize_group
        # beta of the entropy bonus (loss - beta * mean_{a,b} sum_t H): 0 = the reference's loss through the plain
        # entries; > 0 = marl_episode_forward_probs / marl_a2c_loss_entropy_fwd_bwd / marl_episode_backward_probs
        self.__entropy_coef = float(entropy_coef)
        # PPO (marl_advantages / marl_ppo_loss_fwd_bwd / marl_grad_clip): K update epochs per rollout on the clipped
        # surrogate with GAE(lambda) advantages, epochs 1 .. K-1 replaying the stored trajectory under the new
        # weights.  All four at their defaults: the A2C step below, verbatim - nothing new is launched
        self.__ppo_epochs, self.__ppo_clip, self.__gae_lambda = int(ppo_epochs), float(ppo_clip), float(gae_lambda)
        self.__max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.__ppo = ppo_options_on(ppo_epochs, ppo_clip, gae_lambda, max_grad_norm)
        self.__ppo_bufs: Optional[Tuple[th.Tensor, ...]] = None
        self.__grad_norm: Optional[th.Tensor] = None
        self.__curr_step = 0
        self.__loss_bufs: Optional[Tuple[th.Tensor, ...]] = None
        self.__conf_meter = ConfusionMeter(nb_class, window_size=meter_window_size)
        if report is not None:
            from ..report import ReportOptions

            if not isinstance(report, ReportOptions):
                raise ValueError(f"report must be a report.ReportOptions or None, got {type(report).__name__}")
        self.__report_opts = report
        self.__report = None  # (the EpisodeReport: made at the first step, which knows the steps and the agents)
        self.__meter_window_size = meter_window_size
        self.__meter_keys = ("loss", "path", "error", "critic") + (("entropy",) if entropy_coef > 0 else ())
        # (scalars index of every meter: the PPO scalars keep the entropy slot, zero without a bonus)
        self.__meter_idx = {k: i for i, k in enumerate(self.__meter_keys)}
        if self.__ppo:
            self.__meter_idx.update(approx_kl=5, clip_frac=6)
            self.__meter_keys += ("approx_kl", "clip_frac")
        self.__meters = {k: LossMeter(window_size=meter_window_size) for k in self.__meter_keys}
        if self.__max_grad_norm is not None:
            self.__meters["grad_norm"] = LossMeter(window_size=meter_window_size)

    @property
    def curr_step(self) -> int:
        return self.__curr_step

    def __comm(self) -> Optional[CommUpdate]:
        """The update of the model's live communication source for this step (None: no ``comm_lr`` or no live source)."""
        model = self.__model
        self.__comm_update = comm_update_for(self.__comm_update, model.comm_source, model.comm_parameters,
                                             self.__comm_lr)
        if self.__comm_update is not None and self.__comm_pending is not None:
            self.__comm_update.opt.load_state_dict(self.__comm_pending)
            self.__comm_pending = None
        return self.__comm_update

    def __exact_phases(self, call: Callable[[int], Tuple[th.Tensor, ...]]) -> None:
        """``call(phase)`` (``a2c_loss`` / ``advantages``; adv_stats = result[4]) in one piece, or - with an
        ``exact_standardize_group`` - around one 3-double all-reduce: global mean / std of the advantages (the only
        batch-wide statistic: phase 1 leaves the entropy alone)."""
        if self.__exact_group is None:
            call(0)
            return
        from ..parallel import allreduce_adv_stats

        allreduce_adv_stats(call(1)[4], self.__exact_group)
        call(2)

    # one optimisation step on a batch (reference trainer.py:67-116)
    def train_step(self, x: th.Tensor, y: th.Tensor, sampler: EpisodeSampler,
                   targets: Optional[th.Tensor] = None) -> Tuple[EpisodeTensors, th.Tensor]:
        """``targets``: fp32 [Nb, nC] target distributions on the device (``mix.soft_targets`` of a CutMix / Mixup
        batch, a teacher's distribution) that the vote error and the rewards take in place of ``y``
        (``HipEngine.set_soft_targets``), installed around this step's loss calls - every PPO epoch among them - and
        cleared behind them; ``y`` stays the hard label for the meters."""
        model = self.__model
        y = y.to(model.device)
        if self.temperature is not None or self.explore_eps is not None:  # (checked here: ValueError before any call)
            x0 = model.exploration
            model.set_exploration(x0.temperature if self.temperature is None else self.temperature,
                                  x0.eps if self.explore_eps is None else self.explore_eps, x0.greedy)
        step = self.__train_step_ppo if self.__ppo else self.__train_step_a2c
        out, scalars = step(x, y, sampler, targets)
        if self.__report_opts is not None:  # (here, not in train_epoch: all steps and the labels are at hand)
            self.__report_add(out.step_preds, y)
        return out, scalars

    def __report_add(self, step_preds: th.Tensor, y: th.Tensor) -> None:
        if self.__report is None:
            from ..report import EpisodeReport

            ns, na = step_preds.shape[0], step_preds.shape[1]
            self.__report = EpisodeReport(ns, na, self.__nb_class, self.__report_opts, step_preds.device,
                                          window_size=self.__meter_window_size)
        self.__report.add(step_preds, y)

    @property
    def report(self):
        """The training meter's ``EpisodeReport`` (None without ``report`` or before the first step)."""
        return self.__report

    def __train_step_a2c(self, x: th.Tensor, y: th.Tensor, sampler: EpisodeSampler,
                         targets: Optional[th.Tensor] = None) -> Tuple[EpisodeTensors, th.Tensor]:
        model = self.__model
        # with the entropy bonus: the same sequence through the three entries that carry the step distributions
        # (scalars[4] = the mean entropy)
        beta = self.__entropy_coef
        ent = beta > 0
        eng, out = sampler.run_episode_raw(x, train=True, probs=ent)
        bufs = self.__loss_bufs
        if (bufs is None or len(bufs) != (6 if ent else 5) or bufs[0].shape != out.step_preds.shape or
                (ent and bufs[5].shape != out.step_probs.shape)):
            bufs = self.__loss_bufs = eng.new_loss_bufs(out, ent)
        with self.__class_loss.installed(eng), soft_targets_installed(eng, targets):
            self.__exact_phases(lambda phase: eng.a2c_loss(out, y, self.__gamma, phase, bufs, entropy_coef=beta))
        flat = model.flat_state()
        apply_update(eng, flat, bufs[0], bufs[1], bufs[2], bufs[5] if ent else None, flat.grad_views(), self.__lr,
                     self.__allreduce, None, lambda: model.mark_updated(eng), self.__comm(), self.__optim)
        return out, bufs[3]

    def __train_step_ppo(self, x: th.Tensor, y: th.Tensor, sampler: EpisodeSampler,
                         targets: Optional[th.Tensor] = None) -> Tuple[EpisodeTensors, th.Tensor]:
        """One rollout, K updates.  Returns the ROLLOUT's outputs (meters and confusion matrix stay on-policy) and
        the last epoch's scalars {loss, surrogate, error, critic, entropy, approx_kl, clip_frac}."""
        model, beta = self.__model, self.__entropy_coef
        ent = beta > 0
        # the draws of this rollout and the batch on the device: epochs 1 .. K-1 replay with them (nothing is drawn or
        # uploaded again); run_episode_raw(draws=...) takes given draws as they are
        _, img, draws = sampler.prepare(x)
        eng, out = sampler.run_episode_raw(img, train=True, draws=draws, probs=ent)
        if not ppo_bufs_fit(self.__ppo_bufs, out, ent):
            self.__ppo_bufs = eng.new_ppo_bufs(out, ent)
        bufs = self.__ppo_bufs
        flat = model.flat_state()
        with self.__class_loss.installed(eng), soft_targets_installed(eng, targets):
            self.__exact_phases(lambda phase: eng.advantages(out, y, self.__gamma, self.__gae_lambda, phase, bufs))
            norm = ppo_epochs_loop(
                eng, flat, out, y, bufs, self.__ppo_epochs, self.__ppo_clip, beta, self.__lr, self.__allreduce,
                self.__max_grad_norm, flat.grad_views(),
                replay=lambda: sampler.run_episode_raw(img, train=True, draws=draws, probs=ent,
                                                       forced=out.step_actions)[1],
                repack=lambda: model.mark_updated(eng), comm=self.__comm(), optim=self.__optim)
        if norm is not None:
            self.__grad_norm = norm
        return out, bufs[3]

    def train_epoch(self, dataloader: Iterable, epoch_index: int, episode_sampler: EpisodeSampler) -> None:
        self.__model.train()
        for x_train, y_train, *rest in dataloader:  # (a mixing loader yields (x, y_primary, Q): data.py)
            out, scalars = self.train_step(x_train, y_train, episode_sampler, targets=rest[0] if rest else None)
            # device-side meters, no sync (select last step, mean over agents: trainer.py:124-128)
            if self.__report_opts is None:  # (else train_step fed the report)
                self.__conf_meter.add(out.step_preds[-1].mean(dim=0), y_train)
            for k in self.__meter_keys:
                self.__meters[k].add(scalars[self.__meter_idx[k]].clone())
            if self.__max_grad_norm is not None:  # (the norm before clipping, of the last epoch's gradient)
                self.__meters["grad_norm"].add(self.__grad_norm.clone())
            if self.__metric_logger is not None and self.__curr_step % self.__log_interval == 0:
                self.__metric_logger(self.__curr_step, self.metrics())
            self.__curr_step += 1

    def metrics(self) -> Dict[str, float]:
        """Synchronises: windowed means of the loss terms + train precision / recall."""
        meter = self.__conf_meter if self.__report is None else self.__report
        m = {
            "error": self.__meters["error"].loss(),
            "path_loss": self.__meters["path"].loss(),
            "loss": self.__meters["loss"].loss(),
            "critic_loss": self.__meters["critic"].loss(),
            "train_prec": meter.precision().mean().item(),
            "train_rec": meter.recall().mean().item(),
        }
        if self.__report is not None:
            from ..report import summary_metrics

            m.update(summary_metrics(self.__report.result(), self.__report_opts, "train"))
        if "entropy" in self.__meters:  # (only with an entropy bonus: the plain trainer never sees the distributions)
            m["entropy"] = self.__meters["entropy"].loss()
        for k in ("approx_kl", "clip_frac", "grad_norm"):  # (only with the matching PPO option on)
            if k in self.__meters:
                m[k] = self.__meters[k].loss()
        if self.__optim is not None and self.__optim.scalars is not None:  # (the rate of the last step, from the kernel)
            m["lr"] = self.__optim.scalars[0].item()
        return m

    @property
    def optim_options(self):
        """The ``optim.OptimOptions`` in force (the schedule's base rate filled in), or None."""
        return None if self.__optim is None else self.__optim.opts

    @contextmanager
    def ema_weights(self):
        """Inside the context the model holds the AVERAGED weights (``optim.OptimOptions.ema_decay``): episodes,
        ``eval_epoch`` and ``model.state_dict()`` see them; on exit the trained weights are back, bit for bit.  No
        ``train_step`` may run inside."""
        if self.__optim is None or self.__optim.opts.ema_decay is None:
            raise ValueError("ema_weights(): the trainer keeps no averaged weights (OptimOptions.ema_decay)")
        model = self.__model
        flat = model.flat_state()
        ema = flat.ema_views()
        named = list(model.named_parameters())
        saved = {k: p.detach().clone() for k, p in named}
        with th.no_grad():
            for k, p in named:  # (through the parameters: their version counters tell ensure_packed to re-pack)
                p.copy_(ema[k])
        try:
            yield model
        finally:
            with th.no_grad():
                for k, p in named:
                    p.copy_(saved[k])

    # ---- resume ---------------------------------------------------------------------------------------------------
    def __fingerprint(self) -> str:
        return f"adam;lr={self.__lr!r}" if self.__optim is None else self.__optim.opts.fingerprint()

    def state_dict(self, sampler: Optional[EpisodeSampler] = None) -> Dict[str, object]:
        """Everything beside the model's weights that an interrupted run needs to continue bit for bit: the Adam
        moments per parameter (``exp_avg.<key>``, ``exp_avg_sq.<key>``), the averaged weights when there are any
        (``ema.<key>``), the optimiser step, ``curr_step``, the fingerprint of the update rule, the state of the
        communication source's Adam, and ``sampler``'s generator position.  Tensors, numbers and strings only:
        ``th.load(weights_only=True)`` reads it."""
        flat = self.__model.flat_state()
        out: Dict[str, object] = {"format": 1, "optim_step": int(flat.step), "curr_step": int(self.__curr_step),
                                  "fingerprint": self.__fingerprint()}
        for tag, buf in (("exp_avg", flat.exp_avg), ("exp_avg_sq", flat.exp_avg_sq), ("ema", flat.ema)):
            if buf is None:
                continue
            for k, v in flat._views(buf).items():
                out[f"{tag}.{k}"] = v.detach().cpu().clone()
        if self.__comm_update is not None:
            out["comm_adam"] = self.__comm_update.opt.state_dict()
        if sampler is not None:
            rng = sampler.rng_state()
            out["rng_seed"], out["rng_episodes"] = rng["seed"], rng["episodes"]
        return out

    def load_state_dict(self, state: Dict[str, object], sampler: Optional[EpisodeSampler] = None) -> None:
        """Continue from ``state_dict()``'s dictionary (the model's weights are loaded separately, before this).
        ValueError: another update rule (fingerprint), a missing entry or another shape."""
        if state.get("format") != 1:
            raise ValueError(f"trainer state: unknown format {state.get('format')!r}")
        if state.get("fingerprint") != self.__fingerprint():
            raise ValueError("trainer state: it was written under another update rule\n"
                             f"  file:    {state.get('fingerprint')}\n  trainer: {self.__fingerprint()}")
        flat = self.__model.flat_state()
        want_ema = self.__optim is not None and self.__optim.opts.ema_decay is not None
        loads = []
        for tag in ("exp_avg", "exp_avg_sq") + (("ema",) if want_ema else ()):
            for k, shape in flat.shapes.items():
                t = state.get(f"{tag}.{k}")
                if not isinstance(t, th.Tensor) or tuple(t.shape) != tuple(shape):
                    raise ValueError(f"trainer state: {tag}.{k} is "
                                     f"{'missing' if t is None else tuple(getattr(t, 'shape', ()))}, "
                                     f"the model needs {tuple(shape)}")
                loads.append((tag, k, t))
        bufs = {"exp_avg": flat.exp_avg, "exp_avg_sq": flat.exp_avg_sq}
        if want_ema:
            bufs["ema"] = flat.ema_buffer()
        views = {tag: flat._views(b) for tag, b in bufs.items()}
        with th.no_grad():
            for tag, k, t in loads:  # (nothing is written before everything is checked)
                views[tag][k].copy_(t)
        flat.step = int(state["optim_step"])
        self.__curr_step = int(state["curr_step"])
        if "comm_adam" in state:
            self.__comm_pending, self.__comm_update = state["comm_adam"], None
        if sampler is not None and "rng_seed" in state:
            sampler.set_rng_state({"seed": state["rng_seed"], "episodes": state["rng_episodes"]})

    def eval_epoch(self, dataloader: Iterable, epoch_index: int, episode_sampler: EpisodeSampler,
                   report=None) -> ConfusionMeter:
        """``report`` (a ``report.EpisodeReport`` on the model's device): every batch runs ``run_episode``, which
        returns all steps, and fills the report, which is returned - it has ``ConfusionMeter``'s reading methods.
        None: the last step's vote into a ``ConfusionMeter``, as before."""
        self.__model.eval()
        if report is not None:
            with th.no_grad():
                for x_test, y_test in dataloader:
                    report.add(episode_sampler.run_episode(x_test).step_preds, y_test.to(self.__model.device))
            return report
        conf_meter = ConfusionMeter(self.__nb_class, None)
        with th.no_grad():
            for x_test, y_test in dataloader:
                out = episode_sampler.run_episode_get_last_step(x_test)
                conf_meter.add(out.prediction.mean(dim=0), y_test)
        return conf_meter
