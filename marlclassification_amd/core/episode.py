"""EpisodeSampler (reference core/episode.py): ``run_episode`` is ONE call into the HIP
library for all ``nb_step`` steps (``marl_episode_forward``); with autograd enabled the
outputs carry a single autograd node whose backward is ``marl_episode_backward`` (BPTT
through every step), so the reference's own loss code and ``loss.backward()`` work
unchanged on top of it."""

from dataclasses import dataclass
from typing import Optional, Tuple

import torch as th

from ..engine import EpisodeTensors, HipEngine
from ..fused import EpisodeDraws, draw_episode_device
from .agent import MultiAgent
from .environment import Environment


@dataclass
class EpisodeOutput:
    prediction: th.Tensor
    actions_log_probs: th.Tensor


@dataclass
class EpisodeDetailedOutput:
    step_preds: th.Tensor
    step_log_probas: th.Tensor
    step_values: th.Tensor
    step_pos: th.Tensor
    # beyond the reference's four fields: the distribution every step sampled from, [Ns,Na,Nb,nA] (only with
    # ``EpisodeSampler.return_probs``; differentiable), and the sampled actions, int64 [Ns,Na,Nb]
    step_probs: Optional[th.Tensor] = None
    step_actions: Optional[th.Tensor] = None


@dataclass
class Trajectory:
    """What ``run_episode(img, replay=...)`` needs to walk a stored episode again: its initial draws and the
    actions it took (``EpisodeSampler.last_trajectory``)."""

    draws: EpisodeDraws
    actions: th.Tensor  # int64 [Ns,Na,Nb]


class _EpisodeFunction(th.autograd.Function):
    """Autograd boundary around the fused episode: inputs are the image batch and the model parameters,
    outputs step_preds / step_log_probas / step_values (+ non-differentiable positions and actions) and, with
    ``probs``, the differentiable step_probs as a sixth output.  ``forced`` (int64 [Ns,Na,Nb] or None) replaces
    the sampling (trajectory replay).  ``comm``: the mixing matrix as a differentiable input - the engine's live
    matrix (``HipEngine.comm_live``: its detached value is what the kernels read) or None; asked for, its gradient is
    marl_comm_grad's, two launches behind the backward pass."""

    @staticmethod
    def forward(ctx, eng: HipEngine, img: th.Tensor, draws: EpisodeDraws, names, probs: bool,
                forced: Optional[th.Tensor], comm: Optional[th.Tensor], *params):
        # every episode owns its saved activations (a training workspace from the engine's pool), so
        # several rollouts of one model can be alive at once and (loss1 + loss2).backward() works as
        # with the reference's autograd graph (reference core/episode.py:84)
        ws = eng.train_ws_acquire()
        out = eng.episode_forward(img, draws.pos0, draws.h0, draws.c0, draws.hc0, draws.cc0,
                                  draws.noise, forced, True, rng=draws.rng, ws=ws, probs=probs)
        ctx.eng, ctx.ws, ctx.img = eng, ws, img
        ctx.cfg_key = eng._cfg_key
        ctx.comm = eng.comm  # the backward goes through the transpose of THIS rollout's matrix, whatever is set by then
        ctx.comm_range = eng.comm_range  # (likewise the range: the backward rebuilds THIS rollout's gates)
        ctx.comm_dtype = None if comm is None else comm.dtype
        ctx.exploration = eng.exploration  # (and the behaviour policy THIS rollout's probabilities were saved under)
        ctx.pack_generation = eng.pack_generation
        ctx.names = names
        ctx.shapes = [p.shape for p in params]
        ctx.mark_non_differentiable(out.step_pos, out.step_actions)
        res = (out.step_preds, out.step_log_probas, out.step_values, out.step_pos, out.step_actions)
        return res + (out.step_probs,) if probs else res

    @staticmethod
    def backward(ctx, g_preds, g_logp, g_values, _g_pos, _g_act, g_probs=None):
        eng: HipEngine = ctx.eng
        if ctx.ws is None:
            raise RuntimeError("this episode's saved activations were already released by an earlier "
                               "backward (run the episode again instead of retain_graph)")
        if ctx.pack_generation != eng.pack_generation:
            raise RuntimeError("the model's weights were modified (re-packed) after this episode's rollout: "
                               "its backward needs the weights the rollout used - call backward before "
                               "the optimiser step")
        later_comm, eng.comm = eng.comm, ctx.comm
        later_range, eng.comm_range = eng.comm_range, ctx.comm_range
        later_explore, eng.exploration = eng.exploration, ctx.exploration
        try:
            if ctx.cfg_key != eng._cfg_key:  # another shape ran in between: switch the engine back
                na, nb, ns, shape, u8 = ctx.cfg_key
                eng.configure(na, nb, ns, shape, img_u8=u8)
            grads = {k: th.empty(s, device=eng.device) for k, s in zip(ctx.names, ctx.shapes)}
            # the image is a differentiable input (the reference's crop is a masked_select of it,
            # core/environment.py:95-126): asked for, its gradient comes out of the same backward pass
            d_img = th.empty(ctx.img.shape, device=eng.device) if ctx.needs_input_grad[1] else None
            d_comm = None
            if ctx.needs_input_grad[6]:  # (the matrix of THIS rollout sits in eng.comm for the call)
                d_comm = th.empty(ctx.comm.shape, device=eng.device)
            if d_comm is None:  # what this backward has always called
                eng.episode_backward(g_preds, g_logp, g_values, grads, ws=ctx.ws, img=ctx.img, d_img=d_img,
                                     g_probs=g_probs)
            else:
                eng.episode_backward(g_preds, g_logp, g_values, grads, ws=ctx.ws, img=ctx.img, d_img=d_img,
                                     g_probs=g_probs, d_comm=d_comm)
                d_comm = d_comm.to(ctx.comm_dtype)
        finally:
            eng.comm = later_comm
            eng.comm_range = later_range
            eng.exploration = later_explore
        eng.train_ws_release(ctx.ws)
        ctx.ws = None
        # (a frozen model: the parameter gradients are computed and dropped here)
        return (None, d_img, None, None, None, None, d_comm) + tuple(
            grads[k] if need else None for k, need in zip(ctx.names, ctx.needs_input_grad[7:]))


class EpisodeSampler:
    def __init__(self, agents: MultiAgent, env: Environment, nb_step: int, stream_id: int = 1) -> None:
        self.__agents = agents
        self.__env = env
        self.__nb_step = nb_step
        # parity hook: when set, these draws replace the random ones (tests inject the
        # reference's host-drawn positions / states / noise)
        self.fixed_draws: Optional[EpisodeDraws] = None
        # perf mode (default): every draw comes from the library's counter-based generator, keyed
        # by torch's seed (th.manual_seed keeps runs reproducible) and an episode counter.  False:
        # torch draws in the reference's order (positions, h, c, h^, c^, per-step Exp(1)).
        self.device_rng = True
        # True: run_episode also returns ``step_probs`` (marl_episode_forward_probs: one copy launch more; under
        # grad a differentiable output whose gradient reaches the policy head through marl_episode_backward_probs)
        self.return_probs = False
        # initial draws and actions of the latest episode: ``run_episode(img, replay=sampler.last_trajectory)``
        self.last_trajectory: Optional[Trajectory] = None
        self.__episodes = 0
        self.__rng_seed: Optional[int] = None
        # every sampler is its own stream of the generator: the key mixes torch's seed with the
        # rank (shards draw different positions / states / noise under the usual identical
        # th.manual_seed on all ranks) and `stream_id` - an explicit argument, not a
        # construction counter: same seed, same draws, whatever
        # else the process built before
        self.__stream_id = int(stream_id)

    @property
    def nb_step(self) -> int:
        return self.__nb_step

    @property
    def agents(self) -> MultiAgent:
        return self.__agents

    @property
    def env(self) -> Environment:
        return self.__env

    def rng_state(self) -> dict:
        """Position of this sampler's generator stream (``device_rng``): the torch seed that keys it and the number
        of episodes drawn under it - numbers only, so a checkpoint can hold it (``Trainer.state_dict``)."""
        seed = th.initial_seed()
        episodes = self.__episodes if seed == self.__rng_seed else 0
        return {"seed": int(seed), "episodes": int(episodes)}

    def set_rng_state(self, state: dict) -> None:
        """Continue the stream ``rng_state`` described: the next episode draws what the interrupted run's next one
        would have drawn.  The stream is keyed by torch's seed, so a process seeded otherwise is re-seeded
        (``th.manual_seed``) with the stored one."""
        seed, episodes = int(state["seed"]), int(state["episodes"])
        if episodes < 0:
            raise ValueError(f"rng state: episodes must be >= 0, got {episodes}")
        if th.initial_seed() != seed:
            th.manual_seed(seed)
        self.__rng_seed, self.__episodes = seed, episodes

    def draw_key(self, seed: int) -> int:
        """Generator key of this sampler's draws: (torch seed, rank, sampler id)."""
        import os

        from ..parallel import shard_seed

        rank = int(os.environ.get("RANK", "0"))
        return (shard_seed(seed & 0xFFFFFFFFFFFF, rank) * 1_000_003 + self.__stream_id) & ((1 << 63) - 1)

    def prepare(self, img_batch: th.Tensor,
                draws: Optional[EpisodeDraws] = None) -> Tuple[HipEngine, th.Tensor, EpisodeDraws]:
        """Everything before the kernels: device transfer, engine configuration, weight
        packing, and the reference's random draws in the reference's order (positions,
        h, c, h^, c^, per-step Exp(1) noise).  ``draws``: these instead of new ones (a replay)."""
        agents, env = self.__agents, self.__env
        model = agents.model
        device = agents.device
        img = img_batch.to(device)
        na, nb, ns = len(agents), img.shape[0], self.__nb_step
        eng = model.hip_engine(env.actions)
        # uint8 batches ([Nb,C,H,W], 0..255) stay uint8: ToTensor happens inside the gather kernel
        eng.configure(na, nb, ns, img.shape[1:], img_u8=img.dtype == th.uint8)
        model.ensure_packed(eng)
        if draws is not None:
            env.place(img, na, positions=draws.pos0)
            return eng, img, draws
        if self.fixed_draws is not None:
            env.place(img, na, positions=self.fixed_draws.pos0)
            return eng, img, self.fixed_draws
        if self.device_rng:
            seed = th.initial_seed()
            if seed != self.__rng_seed:  # th.manual_seed() restarts the episode counter
                self.__rng_seed, self.__episodes = seed, 0
            d = draw_episode_device(eng, self.draw_key(seed), self.__episodes)
            self.__episodes += 1
            env.place(img, na, positions=d.pos0)
            return eng, img, d
        pos0 = env.place(img, na)
        st = model.random_first_state(na, nb)
        noise = th.empty(ns, na, nb, env.nb_actions, device=device).exponential_(1.0)
        return eng, img, EpisodeDraws(pos0, st.h, st.c, st.h_caret, st.c_caret, noise)

    def __check_replay(self, img_batch: th.Tensor, replay: Trajectory) -> None:
        na, nb, ns = len(self.__agents), img_batch.shape[0], self.__nb_step
        d = replay.draws
        got = {"actions": (replay.actions, (ns, na, nb)), "pos0": (d.pos0, (na, nb, 2))}
        got.update({k: (getattr(d, k), (na, nb)) for k in ("h0", "c0", "hc0", "cc0")})
        for k, (t, shape) in got.items():
            if tuple(t.shape[:len(shape)]) != shape or (k in ("actions", "pos0") and t.dim() != len(shape)):
                raise ValueError(f"replay: {k} has shape {tuple(t.shape)}, this batch needs {shape} "
                                 "([steps,] agents, batch first) - a trajectory replays on a batch of its own size")

    def __episode_impl(self, img_batch: th.Tensor, replay: Optional[Trajectory] = None) -> EpisodeDetailedOutput:
        if replay is not None:
            self.__check_replay(img_batch, replay)  # (before anything is transferred or enqueued)
        eng, img, draws = self.prepare(img_batch, None if replay is None else replay.draws)
        forced = None if replay is None else replay.actions.to(img.device)
        model = self.__agents.model
        want_probs = bool(self.return_probs)
        live = eng.comm_live  # (prepare() evaluated the model's live source, if it has one, for this forward)
        if th.is_grad_enabled() and (img.requires_grad or any(p.requires_grad for p in model.parameters()) or
                                     (live is not None and live.requires_grad)):
            named = list(model.named_parameters())
            names = tuple(k for k, _ in named)
            res = _EpisodeFunction.apply(eng, img, draws, names, want_probs, forced, live, *[p for _, p in named])
            preds, logp, values, pos, act = res[:5]
            probs = res[5] if want_probs else None
        else:
            out = eng.episode_forward(img, draws.pos0, draws.h0, draws.c0, draws.hc0, draws.cc0,
                                      draws.noise, forced, False, rng=draws.rng, probs=want_probs)
            preds, logp, values, pos, act, probs = (out.step_preds, out.step_log_probas, out.step_values,
                                                    out.step_pos, out.step_actions, out.step_probs)
        self.__env._set_positions(pos[-1])
        self.last_trajectory = Trajectory(draws, act)
        return EpisodeDetailedOutput(preds, logp, values, pos, probs, act)

    def run_episode(self, img_batch: th.Tensor, replay: Optional[Trajectory] = None) -> EpisodeDetailedOutput:
        """``replay``: walk a stored trajectory again - its initial draws, its actions forced - under the
        current weights (log pi_new(a) - log pi_old(a) on stored data; differentiable as usual)."""
        return self.__episode_impl(img_batch, replay)

    def run_episode_get_last_step(self, img_batch: th.Tensor) -> EpisodeOutput:
        out = self.__episode_impl(img_batch)
        return EpisodeOutput(prediction=out.step_preds[-1],
                             actions_log_probs=out.step_log_probas[-1])

    def run_episode_raw(self, img_batch: th.Tensor, train: bool,
                        draws: Optional[EpisodeDraws] = None,
                        probs: bool = False,
                        forced: Optional[th.Tensor] = None) -> Tuple[HipEngine, EpisodeTensors]:
        """No autograd node: used by the fused Trainer (loss + backward are HIP calls).  An image that
        requires grad is ignored here - the gradient w.r.t. the image exists on the ``run_episode`` path.
        ``draws``: these instead of new ones - nothing is drawn, the sampler's episode counter stays (a replay
        leaves the generator sequence of later rollouts where it was).  ``forced`` (int64 [Ns,Na,Nb]): these actions
        replace the sampling (``draws`` + ``forced`` = the stored trajectory under the current weights)."""
        if forced is not None:
            if draws is None:
                raise ValueError("replay: forced actions need the draws of the episode they were sampled in")
            self.__check_replay(img_batch, Trajectory(draws, forced))  # (before anything is transferred or enqueued)
        eng, img, d = self.prepare(img_batch, draws)
        if forced is not None:
            forced = forced.to(img.device)
        out = eng.episode_forward(img, d.pos0, d.h0, d.c0, d.hc0, d.cc0, d.noise, forced, train,
                                  rng=d.rng, probs=probs)
        self.__env._set_positions(out.step_pos[-1])
        return eng, out
