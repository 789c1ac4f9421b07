"""One A2C training iteration entirely on the HIP path (the body of the reference's
``Trainer.train_epoch`` loop, training/trainer.py:66-116): rollout -> loss + output
gradients -> backward through the episode -> [gradient all-reduce] -> Adam -> re-pack.

Parameters live in ONE flat fp32 buffer (the model's ``nn.Parameter``s are views into it),
gradients in a second one, so that Adam is a single kernel and data parallelism is a single
all-reduce (parallel.py).  No host synchronisation happens inside ``iteration``.
"""

from __future__ import annotations

from contextlib import contextmanager
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch as th

from .engine import EpisodeTensors, HipEngine, ModelSpec


@dataclass
class EpisodeDraws:
    """The reference's random draws for one episode, in its draw order:
    positions (environment.py:33-43), h, c, h^, c^ (models.py:148-159), then one Exp(1)
    tensor per step (``th.multinomial`` == argmax(p / q), agent.py:53-55)."""

    pos0: th.Tensor
    h0: th.Tensor
    c0: th.Tensor
    hc0: th.Tensor
    cc0: th.Tensor
    noise: Optional[th.Tensor]  # None: the sampling kernel draws its own Exp(1) variates (`rng`)
    rng: Optional[Tuple[int, int]] = None  # (seed, offset) of the library's counter-based generator


def draw_episode(spec: ModelSpec, na: int, nb: int, ns: int, sizes, device,
                 generator: Optional[th.Generator] = None) -> EpisodeDraws:
    """Device-side draws (torch's Philox generator: RNG plumbing, not compute)."""
    f = spec.window
    pos0 = th.stack(
        [th.randint(int(s) - f, (na, nb), device=device, generator=generator) for s in sizes],
        dim=-1,
    )
    h0 = th.randn(na, nb, spec.n_b, device=device, generator=generator)
    c0 = th.randn(na, nb, spec.n_b, device=device, generator=generator)
    hc0 = th.randn(na, nb, spec.n_a, device=device, generator=generator)
    cc0 = th.randn(na, nb, spec.n_a, device=device, generator=generator)
    noise = th.empty(ns, na, nb, len(spec.actions), device=device).exponential_(
        1.0, generator=generator
    )
    return EpisodeDraws(pos0, h0, c0, hc0, cc0, noise)


def draw_episode_device(engine: HipEngine, seed: int, offset: int) -> EpisodeDraws:
    """Perf mode: every draw of the episode comes from the library (one launch for positions
    and initial states; the per-step Exp(1) noise is drawn inside the sampling kernel)."""
    pos0, h0, c0, hc0, cc0, _ = engine.draw_episode(seed, offset)
    return EpisodeDraws(pos0, h0, c0, hc0, cc0, None, (seed, offset))


class FlatParams:
    """Flat fp32 parameter / gradient / Adam-moment buffers with per-tensor views."""

    def __init__(self, shapes: Dict[str, Tuple[int, ...]], device: th.device) -> None:
        self.names: List[str] = list(shapes)
        self.shapes = dict(shapes)
        self.offsets: Dict[str, int] = {}
        off = 0
        for k, s in shapes.items():
            self.offsets[k] = off
            n = 1
            for d in s:
                n *= d
            # 16-byte aligned slices so every tensor can be read with 128-bit loads
            off += (n + 3) & ~3
        self.numel = off
        self.params = th.zeros(off, device=device)
        self.grads = th.zeros(off, device=device)
        self.exp_avg = th.zeros(off, device=device)
        self.exp_avg_sq = th.zeros(off, device=device)
        self.ema: Optional[th.Tensor] = None  # averaged weights (optim.OptimOptions.ema_decay): see ema_buffer()
        self.step = 0

    def ema_buffer(self) -> th.Tensor:
        """The averaged copy of the weights; allocated when first asked for, as a copy of ``params``."""
        if self.ema is None:
            self.ema = self.params.clone()
        return self.ema

    def ema_views(self) -> Dict[str, th.Tensor]:
        return self._views(self.ema_buffer())

    def _views(self, flat: th.Tensor) -> Dict[str, th.Tensor]:
        out = {}
        for k, s in self.shapes.items():
            n = 1
            for d in s:
                n *= d
            out[k] = flat[self.offsets[k]: self.offsets[k] + n].view(s)
        return out

    def param_views(self) -> Dict[str, th.Tensor]:
        return self._views(self.params)

    def grad_views(self) -> Dict[str, th.Tensor]:
        return self._views(self.grads)

    def load(self, tensors: Dict[str, th.Tensor]) -> None:
        views = self.param_views()
        with th.no_grad():
            for k in self.names:
                views[k].copy_(tensors[k])


def check_ppo_options(ppo_epochs: int, ppo_clip: float, gae_lambda: float, max_grad_norm: Optional[float]) -> None:
    """The constructor guards ``Trainer`` and ``FusedA2C`` share."""
    if isinstance(ppo_epochs, bool) or not isinstance(ppo_epochs, int) or ppo_epochs < 1:
        raise ValueError(f"ppo_epochs must be an integer >= 1, got {ppo_epochs!r}")
    if not ppo_clip > 0.0:
        raise ValueError(f"ppo_clip must be > 0, got {ppo_clip}")
    if not 0.0 <= gae_lambda <= 1.0:
        raise ValueError(f"gae_lambda must lie in [0, 1], got {gae_lambda}")
    if max_grad_norm is not None and not max_grad_norm > 0.0:
        raise ValueError(f"max_grad_norm must be > 0 or None, got {max_grad_norm}")


def ppo_options_on(ppo_epochs: int, ppo_clip: float, gae_lambda: float, max_grad_norm: Optional[float]) -> bool:
    """False = all four at their defaults: the A2C entries."""
    return ppo_epochs != 1 or ppo_clip != 0.2 or gae_lambda != 1.0 or max_grad_norm is not None


class CommUpdate:
    """The update of a LIVE communication source (``set_comm`` with a tensor that requires grad, a module or a
    callable) next to the flat Adam step; ``Trainer`` and ``FusedA2C`` both run this when they are given a
    ``comm_lr``.  Per update: the backward also writes ``d_comm`` (marl_comm_grad) into ``buffer()``; ``step``
    sums it over the ranks with the collective the flat gradient took and applies the same scale (1 / world),
    back-propagates it from the matrix the forward evaluated to the source's leaves (``matrix.backward(d_comm)``)
    and steps a ``torch.optim.Adam`` over those leaves - a dozen tiny torch launches on Na^2 values.
    ``max_grad_norm`` does not reach here: the global-norm clip covers the flat parameter buffer only."""

    def __init__(self, source, leaves: Sequence[th.Tensor], lr: float) -> None:
        if not lr > 0.0:
            raise ValueError(f"comm_lr must be > 0 or None, got {lr}")
        leaves = list(leaves)
        if not leaves:
            raise ValueError("comm_lr: the live communication source has no leaf that requires grad (a plain "
                             "callable offers no parameters(): pass a module or a tensor)")
        self.source = source
        self.opt = th.optim.Adam(leaves, lr=lr)
        self._d: Optional[th.Tensor] = None

    def buffer(self, eng: HipEngine) -> th.Tensor:
        na = eng.cfg.nb_agents
        if self._d is None or self._d.shape[0] != na or self._d.device != eng.device:
            self._d = th.empty(na, na, device=eng.device)
        return self._d

    def step(self, live: Optional[th.Tensor], allreduce, scale: float) -> None:
        if live is None or not live.requires_grad:
            raise RuntimeError("comm_lr: the communication source was evaluated without a graph (grad mode off, or a "
                               "source that does not depend on its leaves): nothing to update")
        d = self._d
        if allreduce is not None:
            allreduce(d)  # (sum over ranks; `scale` = what the flat gradient's collective returned)
        self.opt.zero_grad(set_to_none=True)
        live.backward((d if scale == 1.0 else d * scale).to(live.dtype))
        self.opt.step()


def comm_update_for(current: Optional[CommUpdate], source, leaves, comm_lr: Optional[float]) -> Optional[CommUpdate]:
    """The ``CommUpdate`` of this iteration: None without a ``comm_lr`` or a live source (the caller then runs
    today's sequence of calls, verbatim); the current one while the source is the same object; else a new one."""
    if comm_lr is None or source is None:
        return None
    if current is not None and current.source is source:
        return current
    return CommUpdate(source, leaves(), comm_lr)


class ClassLossOptions:
    """The four loss options as ``Trainer`` and ``FusedA2C`` take them (``class_weights``, ``label_smoothing``,
    ``error_step_weights``: a ``class_loss.step_schedule`` spec or a sequence, ``weight_rewards``), checked as far as
    they can be without the episode's sizes; ``resolve`` makes the ``class_loss.ClassLoss`` of a configured engine -
    once per (classes, steps) - or None with all four at their defaults; ``with installed(eng):`` runs loss calls
    under it (``HipEngine.set_class_loss``) and puts the engine's own setting back behind them, so another trainer on
    the same engine never inherits it - with all four at their defaults the engine's own setting is left alone."""

    def __init__(self, class_weights=None, label_smoothing: float = 0.0, error_step_weights=None,
                 weight_rewards: bool = False) -> None:
        from . import class_loss as _cl

        _cl.check_label_smoothing(label_smoothing)
        if isinstance(error_step_weights, str):
            _cl.parse_error_steps(error_step_weights)
        if class_weights is not None:  # (finite, >= 0, not all zero; the length waits for the class count)
            class_weights = _cl.check_vector(class_weights, "class weights", len(class_weights))
        self.options = (class_weights, label_smoothing, error_step_weights, weight_rewards)
        self._resolved: Dict[Tuple[int, int], object] = {}

    def resolve(self, eng: HipEngine):
        from . import class_loss as _cl

        key = (eng.cfg.nb_class, eng.cfg.nb_steps)
        if key not in self._resolved:
            self._resolved[key] = _cl.from_options(key[0], key[1], *self.options)
        return self._resolved[key]

    @contextmanager
    def installed(self, eng: HipEngine):
        c = self.resolve(eng)
        if c is None:
            yield
            return
        before = eng.class_loss
        eng.set_class_loss(c)
        try:
            yield
        finally:
            eng.class_loss = before


@contextmanager
def soft_targets_installed(eng: HipEngine, targets: Optional[th.Tensor], check_values: bool = True):
    """``with soft_targets_installed(eng, Q):`` runs loss calls under the target distributions ``Q`` (fp32 [Nb, nC],
    ``HipEngine.set_soft_targets``) and puts the engine's own setting back behind them; None: nothing is touched."""
    if targets is None:
        yield
        return
    before = eng.soft_targets
    eng.set_soft_targets(targets, check_values)
    try:
        yield
    finally:
        eng.soft_targets = before


class OptimRun:
    """The optimiser options (``optim.OptimOptions``) as ``Trainer`` and ``FusedA2C`` hold them: the schedule's base
    rate filled in from the learning rate, the merged segment table of each flat buffer it met (host arrays, built
    once), and the device block {lr_t, 1 - beta1^t, 1 - beta2^t, t} the kernel writes for the meters."""

    def __init__(self, opts, lr: float) -> None:
        from . import optim as _optim

        if not isinstance(opts, _optim.OptimOptions):
            raise ValueError(f"optim must be an optim.OptimOptions or None, got {opts!r}")
        self.opts = opts.with_lr(lr)
        self._tables: Dict[int, tuple] = {}
        self.scalars: Optional[th.Tensor] = None

    def table(self, flat: "FlatParams"):
        """(segment table, its ctypes array, the frozen element ranges) of ``flat``."""
        from . import optim as _optim

        hit = self._tables.get(id(flat))
        if hit is None or hit[0] is not flat:
            tab = _optim.segments(flat, self.opts)
            hit = self._tables[id(flat)] = (flat, tab, _optim.segment_array(tab), _optim.frozen_ranges(tab))
        return hit[1:]

    def scalars_for(self, eng: HipEngine) -> th.Tensor:
        if self.scalars is None or self.scalars.device != eng.device:
            self.scalars = th.zeros(4, device=eng.device)
        return self.scalars

    def step(self, eng: HipEngine, flat: "FlatParams", step: int, grad_scale: float = 1.0,
             counters: Optional[th.Tensor] = None) -> None:
        tab, arr, _ = self.table(flat)
        eng.optim_step(flat.params, flat.grads, flat.exp_avg, flat.exp_avg_sq, (arr, len(tab)), self.opts, step=step,
                       ema=flat.ema_buffer() if self.opts.ema_decay is not None else None, grad_scale=grad_scale,
                       counters=counters, scalars_out=self.scalars_for(eng))


def ppo_bufs_fit(bufs, out: EpisodeTensors, entropy: bool) -> bool:
    """Do the persistent ``HipEngine.new_ppo_bufs`` tensors match this episode?"""
    return (bufs is not None and len(bufs) == (8 if entropy else 7) and bufs[0].shape == out.step_preds.shape and
            (not entropy or bufs[7].shape == out.step_probs.shape))


def apply_update(eng: HipEngine, flat: "FlatParams", gp, gl, gv, g_probs, gviews, lr: float, allreduce,
                 max_grad_norm: Optional[float], repack: Callable[[], None],
                 comm: Optional[CommUpdate] = None, optim: Optional[OptimRun] = None) -> Optional[th.Tensor]:
    """One update from the output gradients a loss entry wrote - the A2C, entropy and PPO steps of ``Trainer`` and
    ``FusedA2C`` all end here: backward (bucketed hooks around it: two buckets, the heads' slice leaves while the
    reverse loop still runs) -> all-reduce -> [grad_clip, after the all-reduce and its scale: every rank clips the
    same averaged gradient] -> Adam (``flat.step`` += 1) -> ``repack()``.  ``comm`` (a live communication source
    under a ``comm_lr``): the backward also writes d_comm and the source's leaves take their Adam step after the flat
    one; None: ``episode_backward`` is called without ``d_comm``.  Returns the device scalar with the gradient norm
    (None without ``max_grad_norm``).  ``optim`` (an ``OptimRun``): ``marl_optim_step`` under its options takes the
    place of Adam, and with ``max_grad_norm`` the gradient slices of frozen groups are zeroed before the clip, so the
    clipped norm is that of the trainable parameters; None: today's sequence of calls, verbatim."""
    bucketed = hasattr(allreduce, "before_backward")  # parallel.BucketedGradAllReduce
    if bucketed:
        allreduce.before_backward(eng)
    try:
        d_comm = {} if comm is None else {"d_comm": comm.buffer(eng)}
        eng.episode_backward(gp, gl, gv, gviews, g_probs=g_probs, **d_comm)
    finally:
        if bucketed:
            allreduce.after_backward(eng)
    scale = rank_scale = 1.0 if allreduce is None else allreduce(flat.grads)
    norm = None
    if max_grad_norm is not None:
        if optim is not None:
            for begin, end in optim.table(flat)[2]:
                flat.grads[begin:end].zero_()
        norm = eng.grad_clip(flat.grads, max_grad_norm, grad_scale=scale)
        scale = 1.0
    flat.step += 1
    if optim is None:
        eng.adam(flat.params, flat.grads, flat.exp_avg, flat.exp_avg_sq, flat.step, lr, grad_scale=scale)
    else:
        optim.step(eng, flat, flat.step, grad_scale=scale)
    if comm is not None:
        comm.step(eng.comm_live, allreduce, rank_scale)
    repack()
    return norm


def ppo_epochs_loop(eng: HipEngine, flat: "FlatParams", out: EpisodeTensors, y: th.Tensor, bufs, epochs: int,
                    clip: float, beta: float, lr: float, allreduce, max_grad_norm: Optional[float], gviews,
                    replay: Callable[[], EpisodeTensors], repack: Callable[[], None],
                    comm: Optional[CommUpdate] = None, optim: Optional[OptimRun] = None) -> Optional[th.Tensor]:
    """The K update epochs of one rollout ``out`` whose advantages already sit in ``bufs`` (``HipEngine.advantages``);
    ``Trainer`` and ``FusedA2C`` both run this.  Epoch k > 0 starts with ``replay()``: the stored trajectory (same
    draws, the rollout's actions forced) under the weights the last epoch packed.  Then ppo_loss -> ``apply_update``.
    Returns the device scalar with the last epoch's gradient norm (None without ``max_grad_norm``).  ``comm``: the
    source is evaluated again by every ``replay()``, so epoch k runs under the matrix epoch k - 1 produced.
    The gradient-norm clip covers the flat buffer only."""
    gp, gl, gv, _, _, advn, ret = bufs[:7]
    gpr = bufs[7] if beta > 0 else None
    # the old log-probabilities are the rollout's own output tensor: a replay writes fresh outputs, so epoch 0 has
    # rho == 1 bit for bit and no copy is needed - as long as the replay really returns other storage
    old_logp = out.step_log_probas
    cur, norm = out, None
    for k in range(epochs):
        if k > 0:
            cur = replay()
            if cur.step_log_probas.data_ptr() == old_logp.data_ptr():
                raise RuntimeError("PPO replay wrote over the rollout's log-probabilities (persistent output "
                                   "tensors?): the ratios would all be 1")
        eng.ppo_loss(cur, y, old_logp, advn, ret, clip, bufs, entropy_coef=beta)
        norm = apply_update(eng, flat, gp, gl, gv, gpr, gviews, lr, allreduce, max_grad_norm, repack, comm, optim)
    return norm


class FusedA2C:
    """rollout + loss + backward + Adam on one GPU; ``allreduce`` hooks in data parallelism."""

    def __init__(self, engine: HipEngine, flat: FlatParams, lr: float, gamma: float,
                 allreduce: Optional[Callable[[th.Tensor], float]] = None,
                 use_graph: bool = False, entropy_coef: float = 0.0, ppo_epochs: int = 1,
                 ppo_clip: float = 0.2, gae_lambda: float = 1.0,
                 max_grad_norm: Optional[float] = None, comm_lr: Optional[float] = None,
                 temperature: Optional[float] = None, explore_eps: Optional[float] = None,
                 class_weights=None, label_smoothing: float = 0.0, error_step_weights=None,
                 weight_rewards: bool = False, optim=None) -> None:
        """``optim`` (an ``optim.OptimOptions``): every update is one ``marl_optim_step`` under these options - AdamW
        with parameter groups, a schedule whose base rate is ``lr`` (unless it names its own) and, with ``ema_decay``,
        the averaged weights in ``flat.ema``; ``iteration_graph`` captures it reading the counter block's step, so a
        schedule costs no ``counters_set`` between replays.  None: ``marl_adam_step`` exactly as before.

        ``class_weights`` / ``label_smoothing`` / ``error_step_weights`` / ``weight_rewards``: the options of the
        vote error and the rewards (``class_loss.py``) of every loss call of this object - installed on the engine
        around them and taken off behind them; all four at their defaults: the engine's own ``set_class_loss`` setting
        (none: today's sequence of calls, verbatim) applies.

        ``temperature`` / ``explore_eps``: the behaviour policy of the rollouts (``HipEngine.set_exploration``;
        replays run under the rollout's setting) - plain attributes that may be changed between iterations (a captured
        graph is keyed by the setting); None: the engine's own setting is left alone.

        ``comm_lr``: learning rate of the engine's LIVE communication source (``engine.set_comm`` with a tensor
        that requires grad or a module such as ``comm.LearnableComm``): every update also takes d_comm out of the
        backward and steps a ``torch.optim.Adam`` over the source's leaves (``CommUpdate``).  None, or a constant
        matrix: today's sequence of calls, verbatim.  ``max_grad_norm`` keeps covering the flat buffer only."""
        if use_graph and allreduce is not None:
            raise ValueError("hipGraph replay covers the single-GPU iteration (no collective inside)")
        if comm_lr is not None and not comm_lr > 0.0:
            raise ValueError(f"comm_lr must be > 0 or None, got {comm_lr}")
        if use_graph and comm_lr is not None and engine.comm_source is not None:
            raise ValueError("hipGraph replay does not cover the update of a live communication source (torch "
                             "launches between the captured calls): use_graph with comm_lr and a live source")
        from . import explore as _explore

        _explore.check(1.0 if temperature is None else temperature, 0.0 if explore_eps is None else explore_eps)
        self.temperature, self.explore_eps = temperature, explore_eps
        self._class_loss = ClassLossOptions(class_weights, label_smoothing, error_step_weights, weight_rewards)
        self._optim: Optional[OptimRun] = None if optim is None else OptimRun(optim, lr)
        self.comm_lr = None if comm_lr is None else float(comm_lr)
        self._comm_update: Optional[CommUpdate] = None
        if not entropy_coef >= 0.0:
            raise ValueError(f"entropy_coef must be >= 0, got {entropy_coef}")
        check_ppo_options(ppo_epochs, ppo_clip, gae_lambda, max_grad_norm)
        # K update epochs per rollout on the clipped surrogate (marl_advantages / marl_ppo_loss_fwd_bwd /
        # marl_grad_clip); all four at their defaults: the A2C iteration below, verbatim
        self.ppo_epochs, self.ppo_clip, self.gae_lambda = int(ppo_epochs), float(ppo_clip), float(gae_lambda)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._ppo = ppo_options_on(ppo_epochs, ppo_clip, gae_lambda, max_grad_norm)
        if use_graph and self._ppo:
            # (K epochs in one capture: the counter block would have to tick K Adam steps per generator offset)
            raise ValueError("hipGraph replay covers the one-update A2C iteration: ppo_epochs / ppo_clip / "
                             "gae_lambda / max_grad_norm must stay at their defaults with use_graph")
        self._ppo_bufs = None
        self.last_grad_norm: Optional[th.Tensor] = None  # device scalar: the norm marl_grad_clip saw last
        # beta of the entropy bonus (loss - beta * mean_{a,b} sum_t H); 0: the plain entries, verbatim.  May be
        # changed between iterations (a captured graph is keyed by it)
        self.entropy_coef = float(entropy_coef)
        self._graph = None  # (key, exec handle, stream, persistent tensors)
        self.engine = engine
        self.flat = flat
        self.lr = lr
        self.gamma = gamma
        self.allreduce = allreduce
        self._pviews = flat.param_views()
        self._gviews = flat.grad_views()
        self._loss_bufs = None
        self._packed_gen = -1  # engine.weights_generation at the last pack (-1: never packed)

    def pack(self) -> None:
        self.engine.pack(self._pviews)
        self._packed_gen = self.engine.weights_generation

    def _explore(self) -> None:
        """Hands this object's ``temperature`` / ``explore_eps`` (where not None) to the engine."""
        if self.temperature is None and self.explore_eps is None:
            return
        x0 = self.engine.exploration
        self.engine.set_exploration(x0.temperature if self.temperature is None else self.temperature,
                                    x0.eps if self.explore_eps is None else self.explore_eps, x0.greedy)

    def rollout(self, img: th.Tensor, draws: EpisodeDraws, train: bool,
                forced_actions: Optional[th.Tensor] = None, probs: bool = False) -> EpisodeTensors:
        self._explore()
        if self._packed_gen != self.engine.weights_token():  # never packed, or the workspace was re-laid-out
            self.pack()
        if self.engine.comm_source is not None:  # a live matrix: evaluated once for this forward
            self.engine.refresh_comm()
        return self.engine.episode_forward(img, draws.pos0, draws.h0, draws.c0, draws.hc0,
                                           draws.cc0, draws.noise, forced_actions, train,
                                           rng=draws.rng, probs=probs)

    def iteration_graph(self, img: th.Tensor, y: th.Tensor, seed: int,
                        offset: int, targets: Optional[th.Tensor] = None) -> Tuple[EpisodeTensors, th.Tensor]:
        """The same iteration as ONE hipGraph replay (launch-bound shapes: hundreds of small
        kernels per iteration).  The first call runs one eager iteration (one-off set-up inside
        the library), then captures draw -> rollout -> loss -> backward -> Adam -> re-pack ->
        counter tick on a side stream; later calls replay it.  What changes between iterations
        lives on the device (generator offset, Adam step: the counter block), ``img`` / ``y`` /
        ``targets`` are read from the tensors of the capturing call (same storage every call, or re-capture).
        Outputs are persistent tensors, overwritten by every replay."""
        eng = self.engine
        if self._ppo:
            raise ValueError("iteration_graph captures the one-update A2C iteration: ppo_epochs / ppo_clip / "
                             "gae_lambda / max_grad_norm must stay at their defaults")
        if self.comm_lr is not None and eng.comm_source is not None:
            raise ValueError("iteration_graph does not cover the update of a live communication source (torch "
                             "launches between the captured calls): run iteration(), or drop comm_lr")
        from . import engine as _engine_mod

        # (the tune epoch: after engine.tune() the workspaces baked into a captured graph are freed /
        # re-laid-out - the graph must be captured again)
        beta = self.entropy_coef
        self._explore()
        closs = self._class_loss.resolve(eng) if eng.cfg is not None else None
        key = (img.data_ptr(), y.data_ptr(), None if targets is None else targets.data_ptr(), eng._cfg_key, seed,
               _engine_mod._tune_epoch, beta,
               None if eng.comm is None else eng.comm.data_ptr(),  # (the captured kernels keep the matrix pointer
               eng.comm_range,                                     # and the range's radius / metric / normalize
               eng.exploration,                                    # and the exploration constants in their arguments)
               # (and the loss options, this object's or else the engine's own: their constants and the engine's device
               closs if closs is not None else eng.class_loss,  # copies of the weights, one pair per value)
               None if self._optim is None else self._optim.opts)  # (and the optimiser's constants and segment table)
        if self._graph is None or self._graph[0] != key:
            if self._graph is not None:
                eng.lib.marl_graph_destroy(self._graph[1])
                self._graph = None
            # this call runs eagerly (one-off set-up inside the library happens here) ...
            # (... and the targets' values are checked here, outside the capture: the check synchronises)
            eager = self.iteration(img, y, draw_episode_device(eng, seed, offset), targets=targets)
            offset += 1  # ... and the graph captured below starts at the NEXT iteration
            stream = th.cuda.Stream(device=eng.device)
            out = eng.new_outputs(beta > 0)
            draws = eng.draw_episode(seed, 0)  # persistent draw tensors
            cnt = eng.new_counters()
            gviews = self._gviews
            stream.wait_stream(th.cuda.current_stream(eng.device))
            with th.cuda.stream(stream):
                eng.counters_set(cnt, offset, self.flat.step + 1, self.lr)
                th.cuda.synchronize(eng.device)
                eng.graph_begin()
                try:
                    eng.draw_episode(seed, 0, into=draws, counters=cnt)
                    eng.episode_forward(img, draws[0], draws[1], draws[2], draws[3], draws[4], None,
                                        None, True, rng=(seed, 0), out=out, counters=cnt)
                    with self._class_loss.installed(eng), soft_targets_installed(eng, targets, False):
                        bufs = eng.a2c_loss(out, y, self.gamma, 0, self._loss_bufs, entropy_coef=beta)
                    gp, gl, gv, scalars = bufs[:4]
                    eng.episode_backward(gp, gl, gv, gviews, g_probs=bufs[5] if beta > 0 else None)
                    if self._optim is None:
                        eng.adam(self.flat.params, self.flat.grads, self.flat.exp_avg,
                                 self.flat.exp_avg_sq, 1, self.lr, counters=cnt)
                    else:  # (lr_t and the bias corrections come from cnt's step inside the kernel)
                        self._optim.step(eng, self.flat, 0, counters=cnt)
                    eng.pack(self._pviews)
                    eng.counters_tick(cnt, self.lr)
                except BaseException:
                    # the capture is invalid now: end it, drop whatever that reports, and let the
                    # ROOT cause propagate (no stale graph is left behind: self._graph is None)
                    try:
                        eng.graph_end()
                    except Exception:
                        pass
                    raise
                handle = eng.graph_end()
            # what the device-side counter block holds after the capture: the state the FIRST replay
            # expects (generator offset, optimiser step, learning rate)
            self._graph = (key, handle, stream, (out, draws, cnt, scalars),
                           {"offset": offset, "step": self.flat.step + 1, "cap_lr": self.lr})
            return eager
        _, handle, stream, (out, _draws, cnt, scalars), expect = self._graph
        stream.wait_stream(th.cuda.current_stream(eng.device))
        with th.cuda.stream(stream):
            # eager iterations in between, another offset or a changed learning rate: the device
            # counters are re-synchronised with the host's view before the replay
            # (the tick at the end of the captured graph recomputes the step size with the learning
            # rate of the CAPTURE: after a change of self.lr the counters are set before every replay)
            if (expect["offset"] != offset or expect["step"] != self.flat.step + 1 or
                    expect["cap_lr"] != self.lr):
                eng.counters_set(cnt, offset, self.flat.step + 1, self.lr)
            eng.graph_launch(handle)
        th.cuda.current_stream(eng.device).wait_stream(stream)
        self.flat.step += 1
        eng.fwd_generation += 1
        expect.update(offset=offset + 1, step=self.flat.step + 1)
        return out, scalars

    def iteration(self, img: th.Tensor, y: th.Tensor, draws: EpisodeDraws,
                  targets: Optional[th.Tensor] = None) -> Tuple[EpisodeTensors, th.Tensor]:
        """Returns the episode outputs and the device tensor {loss, path, error, critic} (with an entropy
        bonus: the loss includes it and a fifth scalar holds the mean entropy).  ``targets``: fp32 [Nb, nC] target
        distributions that the vote error and the rewards take in place of ``y`` (``HipEngine.set_soft_targets``),
        installed around the loss calls of this iteration - every PPO epoch among them - and cleared behind them."""
        eng = self.engine
        beta = self.entropy_coef
        if self._ppo:
            return self._iteration_ppo(img, y, draws, targets)
        out = self.rollout(img, draws, True, probs=beta > 0)
        if (self._loss_bufs is None or self._loss_bufs[0].shape != out.step_preds.shape or
                len(self._loss_bufs) != (6 if beta > 0 else 5)):
            self._loss_bufs = eng.new_loss_bufs(out, beta > 0)
        with self._class_loss.installed(eng), soft_targets_installed(eng, targets):
            bufs = eng.a2c_loss(out, y, self.gamma, 0, self._loss_bufs, entropy_coef=beta)
        gp, gl, gv, scalars = bufs[:4]
        apply_update(eng, self.flat, gp, gl, gv, bufs[5] if beta > 0 else None, self._gviews, self.lr,
                     self.allreduce, None, self.pack, self._comm(), self._optim)
        return out, scalars

    def _comm(self) -> Optional[CommUpdate]:
        from . import comm as _comm_mod

        src = self.engine.comm_source
        self._comm_update = comm_update_for(self._comm_update, src, lambda: _comm_mod.leaves(src), self.comm_lr)
        return self._comm_update

    def _iteration_ppo(self, img: th.Tensor, y: th.Tensor, draws: EpisodeDraws,
                       targets: Optional[th.Tensor] = None) -> Tuple[EpisodeTensors, th.Tensor]:
        """One rollout, ``ppo_epochs`` updates; returns the rollout's outputs and the last epoch's scalars
        {loss, surrogate, error, critic, entropy, approx_kl, clip_frac}."""
        eng, beta = self.engine, self.entropy_coef
        ent = beta > 0
        out = self.rollout(img, draws, True, probs=ent)
        bufs = self._ppo_bufs
        if not ppo_bufs_fit(bufs, out, ent):
            bufs = self._ppo_bufs = eng.new_ppo_bufs(out, ent)
        with self._class_loss.installed(eng), soft_targets_installed(eng, targets):
            eng.advantages(out, y, self.gamma, self.gae_lambda, 0, bufs)
            norm = ppo_epochs_loop(
                eng, self.flat, out, y, bufs, self.ppo_epochs, self.ppo_clip, beta, self.lr, self.allreduce,
                self.max_grad_norm, self._gviews,
                replay=lambda: self.rollout(img, draws, True, forced_actions=out.step_actions, probs=ent),
                repack=self.pack, comm=self._comm(), optim=self._optim)
        if norm is not None:
            self.last_grad_norm = norm
        return out, bufs[3]
