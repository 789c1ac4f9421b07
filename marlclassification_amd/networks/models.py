"""ModelsWrapper: the reference's bundle of agent networks (networks/models.py:31-162) as a
drop-in ``nn.Module`` whose arithmetic is libmarl_hip.so.

* same constructor arguments, same ``state_dict()`` keys and shapes (name-mangled private
  attributes), so reference checkpoints load and checkpoints written here load there;
* parameters are views into one flat fp32 buffer (``flat_state``) so Adam and the
  data-parallel all-reduce are single kernels / collectives;
* ``forward`` is the reference's per-step network (MultiAgent.act uses it); whole
  episodes go through core.episode.EpisodeSampler (one call for all steps).  With autograd
  enabled a step is one autograd node (``_StepFunction``: marl_step_forward_train /
  marl_step_backward), so user loops over single steps back-propagate as in the reference.
"""

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch as th
from torch import nn

from ..engine import HipEngine, ModelSpec
from ..fused import FlatParams
from .blocks import LSTMCellWrapper, head, linear_ln_silu, mlp_two_norms
from .init import init_layers
from .vision import VisionCnnModule


class _StepLease:
    """One live step's training workspace: back to the engine's pool at backward, or when the
    autograd graph holding the step is freed without a backward."""

    def __init__(self, eng: HipEngine) -> None:
        self.eng = eng
        self.ws: Optional[th.Tensor] = eng.train_ws_acquire()

    def release(self) -> None:
        ws, self.ws = self.ws, None
        if ws is not None:
            self.eng.train_ws_release(ws)

    def __del__(self) -> None:
        try:
            self.release()
        except Exception:  # (interpreter shutdown)
            pass


def step_needs_graph(model: nn.Module, obs: th.Tensor, norm_pos: th.Tensor, *state: th.Tensor,
                     comm: Optional[th.Tensor] = None) -> bool:
    """A step becomes an autograd node when grad mode is on and a parameter, an input of the
    recurrent state (msg, h, c, h^, c^) or the live mixing matrix ``comm`` requires grad; otherwise it is
    the plain marl_step_forward call.  An observation / position that requires grad is refused rather than
    silently cut."""
    if not th.is_grad_enabled():
        return False
    for t, n in ((obs, "observation"), (norm_pos, "norm_pos")):
        if t.requires_grad:
            raise RuntimeError(
                f"the {n} requires grad: the HIP step has no gradient w.r.t. the observation or the "
                "positions (the reference crops them from an image batch that does not require grad) - "
                "pass it detached")
    return (any(p.requires_grad for p in model.parameters()) or any(t.requires_grad for t in state) or
            (comm is not None and comm.requires_grad))


class _StepFunction(th.autograd.Function):
    """Autograd boundary around ONE step (ModelsWrapper.forward / MultiAgent.act): inputs msg, h, c,
    h^, c^ and the model parameters; outputs probs, values, preds, msg, h, c, h^, c^ (+ the
    non-differentiable actions and their log-probabilities when the step samples).  ``comm``: the mixing matrix as
    a differentiable input (the engine's live matrix, or None); asked for, its gradient is marl_comm_grad's on the
    step workspace, where the message is this step's ``msg``."""

    @staticmethod
    def forward(ctx, eng: HipEngine, obs, norm_pos, noise, rng, names, comm, msg, h, c, hc, cc, *params):
        # every live step owns its saved activations (a one-step training workspace from the engine's
        # pool): an unrolled loop keeps one per step until backward, as the reference's graph does
        lease = _StepLease(eng)
        outs = eng.step_forward(obs, msg, norm_pos, h, c, hc, cc, noise, rng=rng, ws=lease.ws)
        ctx.eng, ctx.lease, ctx.obs = eng, lease, obs.contiguous()
        ctx.cfg_key = eng._cfg_key
        ctx.comm = eng.comm  # the backward goes through the transpose of THIS step's matrix, whatever is set by then
        ctx.comm_dtype = None if comm is None else comm.dtype
        ctx.exploration = eng.exploration  # (likewise the behaviour policy the step's probabilities were saved under)
        ctx.pack_generation = eng.pack_generation
        ctx.names = names
        ctx.sampled = len(outs) == 10
        ctx.save_for_backward(*params)  # (an in-place update of a parameter before backward is an error)
        ctx.set_materialize_grads(False)
        if ctx.sampled:
            ctx.mark_non_differentiable(outs[8])
        return outs

    @staticmethod
    def backward(ctx, g_probs, g_values, g_preds, g_msg, g_h, g_c, g_hc, g_cc, *rest):
        eng: HipEngine = ctx.eng
        lease: _StepLease = ctx.lease
        if lease.ws is None:
            raise RuntimeError("this step's saved activations were already released by an earlier backward "
                               "(run the step again instead of retain_graph)")
        params = ctx.saved_tensors
        if ctx.pack_generation != eng.pack_generation:
            raise RuntimeError("the model's weights were modified (re-packed) after this step's forward: its "
                               "backward needs the weights the forward used - call backward before the "
                               "optimiser step")
        later_comm, eng.comm = eng.comm, ctx.comm
        later_explore, eng.exploration = eng.exploration, ctx.exploration
        try:
            if ctx.cfg_key != eng._cfg_key:  # another shape ran in between: switch the engine back
                na, nb, ns, shape, u8 = ctx.cfg_key
                eng.configure(na, nb, ns, shape, img_u8=u8)
            g_logp = rest[1] if ctx.sampled else None
            grads = {k: th.empty(p.shape, device=eng.device) for k, p in zip(ctx.names, params)}
            want = ctx.needs_input_grad[7:12]
            d_comm = None
            if ctx.needs_input_grad[6]:
                d_comm = th.empty(ctx.comm.shape, device=eng.device)
                d_in = eng.step_backward(lease.ws, ctx.obs, grads, g_probs, g_logp, g_values, g_preds, g_msg, g_h,
                                         g_c, g_hc, g_cc, want=want, d_comm=d_comm)
                d_comm = d_comm.to(ctx.comm_dtype)
            else:  # what this backward has always called
                d_in = eng.step_backward(lease.ws, ctx.obs, grads, g_probs, g_logp, g_values, g_preds, g_msg, g_h,
                                         g_c, g_hc, g_cc, want=want)
        finally:
            eng.comm = later_comm
            eng.exploration = later_explore
        lease.release()
        return (None,) * 6 + (d_comm,) + d_in + tuple(grads[k] for k in ctx.names)


@dataclass
class ModelOutput:
    actions_probabilities: th.Tensor
    values: th.Tensor
    predictions: th.Tensor
    messages: th.Tensor


@dataclass
class RecurrentOutput:
    h: th.Tensor
    c: th.Tensor
    h_caret: th.Tensor
    c_caret: th.Tensor


class ModelsWrapper(nn.Module):
    def __init__(
        self,
        ft_extractor: VisionCnnModule,
        n_b: int,
        n_a: int,
        n_m: int,
        n_m_o: int,
        n_d: int,
        d: int,
        nb_action: int,
        nb_class: int,
        hidden_size_belief: int,
        hidden_size_action: int,
    ) -> None:
        super().__init__()
        if d != 2:
            raise ValueError("the HIP path implements 2-D images only (state_dim == 2)")
        n_in = ft_extractor.out_size + n_d + n_m_o

        self.__map_obs = ft_extractor
        self.__map_pos = linear_ln_silu(d, n_d)
        self.__encode_msg = mlp_two_norms(n_b, 2 * n_m, n_m)
        self.__decode_msg = mlp_two_norms(n_m, 2 * n_m, n_m_o)
        self.__belief_unit = LSTMCellWrapper(n_in, n_b)
        self.__action_unit = LSTMCellWrapper(n_in, n_a)
        self.__policy = head(n_a, hidden_size_action, nb_action, nn.Softmax(dim=-1))
        self.__critic = head(n_a, hidden_size_action, 1, nn.Flatten(-2, -1))
        self.__predict = head(n_b, hidden_size_belief, nb_class, nn.Identity())

        self.__dims = dict(n_b=n_b, n_a=n_a, n_m=n_m, n_m_o=n_m_o, n_d=n_d, nb_class=nb_class,
                           nlb=hidden_size_belief, nla=hidden_size_action)
        self.__nb_action = nb_action
        self.apply(init_layers)

        self.__flat: Optional[FlatParams] = None
        self.__engines: Dict[Tuple, HipEngine] = {}
        self.__packed_token: Dict[int, Tuple] = {}
        # communication graph (comm.py), None = the reference's mean over the other agents.  Non-persistent: the
        # state-dict keys stay the reference's; a buffer, so .to(device) moves it with the module.
        self.register_buffer("comm_matrix", None, persistent=False)
        # a LIVE source of the matrix (set_comm with a tensor that requires grad, a module or a callable): held by
        # reference inside a tuple, so that nn.Module registers nothing - no state-dict key, no entry in
        # parameters() / FlatParams; () = none
        self.__comm_source: Tuple = ()
        # range-limited communication (set_comm_range): a comm.CommRange, None = off
        self.__comm_range = None
        # exploration controls (set_exploration): an explore.Exploration.  A run-time choice: no state-dict key
        from .. import explore as _explore

        self.__exploration = _explore.DEFAULT

    # ---- exploration controls ------------------------------------------------------------
    @property
    def exploration(self):
        """The ``explore.Exploration`` (temperature, eps, greedy) ``set_exploration`` installed."""
        return self.__exploration

    def set_exploration(self, temperature=1.0, eps=0.0, greedy=False) -> None:
        """Every later step / episode of this model (forward, MultiAgent.act, EpisodeSampler, Trainer, the PPO
        epochs) acts under the behaviour policy pi_b = (1 - eps) softmax(z / temperature) + eps / nA
        (``explore.behaviour_probs`` is the same map in torch): it is sampled from - or, ``greedy``, its argmax is
        taken, the lowest index on a tie, without a random draw -, returned as the step's probabilities and its log
        is the step's log-probability; the backward differentiates through it.  The defaults restore the plain
        policy, bit for bit.  ValueError for a temperature that is not finite and > 0 or an eps outside [0, 0.5].
        The setting is not saved with the model."""
        from .. import explore as _explore

        self.__exploration = _explore.check(temperature, eps, greedy)

    # ---- communication graph -------------------------------------------------------------
    @property
    def comm(self) -> Optional[th.Tensor]:
        """The mixing matrix of the message exchange ([Na, Na] fp32, row = receiver), or None (the mean).  Under a
        live source: its current value, detached (evaluated here, without a graph)."""
        if self.__comm_source:
            from .. import comm as _comm

            with th.no_grad():
                return _comm.evaluate(self.__comm_source[0], None, self.device)[1]
        return self.comm_matrix

    @property
    def comm_source(self):
        """The live source ``set_comm`` was given, or None (a constant matrix / the mean)."""
        return self.__comm_source[0] if self.__comm_source else None

    def comm_parameters(self) -> List[th.Tensor]:
        """The leaves behind the live source - what an optimiser of the graph updates (``Trainer(comm_lr=...)``
        builds its Adam on them); [] without a live source.  They are not in ``parameters()`` / ``state_dict()``."""
        if not self.__comm_source:
            return []
        from .. import comm as _comm

        return _comm.leaves(self.__comm_source[0])

    def set_comm(self, matrix) -> None:
        """Every later step / episode of this model (forward, MultiAgent.act, EpisodeSampler, Trainer) aggregates
        messages with ``matrix`` ([Na, Na], row = receiver, column = sender; ``comm.ring`` ...); None restores the
        mean over the other agents.  ValueError for a non-square / non-finite matrix, more agents than the
        mixing kernel serves, or a matrix on another device than the model.

        A tensor that does not require grad is cloned: a constant.  A tensor that requires grad, a module
        (``comm.LearnableComm``) or a callable that returns the matrix is a LIVE source: held by reference, evaluated
        every time a forward fetches the engine - once per episode, once per ``forward`` / ``act`` call, twice for the
        first rollout of a PPO update - (shape, dtype and device are checked then; finiteness is not - it would synchronise the host),
        its detached fp32 value goes to the kernels, and the episode / step autograd nodes take the evaluated matrix
        as a differentiable input: ``loss.backward()`` reaches the source's leaves (``comm_parameters()``) as it
        would through torch ops.  The source is not registered: state-dict keys stay the reference's, and it does
        not move with ``.to(device)`` - keep it on the model's device."""
        from .. import comm as _comm

        if matrix is not None and self.__comm_range is not None:
            if _comm.is_live(matrix):
                raise ValueError("a live (learnable) communication source under a communication range: the gradient "
                                 "of a gated base matrix is not computed (set_comm_range(None) first)")
            _comm.check_range_base(_comm.validate(matrix, None), self.__comm_range.normalize)
        self.__comm_source = ()
        if matrix is None:
            self.comm_matrix = None
            return
        if _comm.is_live(matrix):
            with th.no_grad():
                _comm.evaluate(matrix, None, self.device)  # (a source of the wrong shape / device fails here)
            self.comm_matrix = None
            self.__comm_source = (matrix,)
            return
        m = _comm.validate(matrix, None)
        if m.device != self.device:
            raise ValueError(f"communication matrix lives on {m.device}, the model on {self.device}: "
                             "move it first (matrix.to(model.device))")
        self.comm_matrix = m.clone()  # (never the caller's storage)

    @property
    def comm_range(self):
        """The range-limited communication ``set_comm_range`` installed (a ``comm.CommRange``: radius, metric,
        normalize), or None."""
        return self.__comm_range

    def set_comm_range(self, radius, metric: str = "chebyshev", normalize: bool = True) -> None:
        """Range-limited communication: in every later fused episode of this model (EpisodeSampler, Trainer, the PPO
        epochs) an agent hears the agents within ``radius`` pixels of it (integer >= 0; ``metric`` "chebyshev" -
        max(|dy|, |dx|) on the window corners, so ``radius = f - 1`` means "windows overlap" - or "euclidean"), per
        image and per step: the message emitted in step t is exchanged under the positions of step t.  The constant
        matrix of ``set_comm`` - the complete graph without one - is the base whose out-of-range links are cut;
        ``normalize`` rescales a receiver's remaining weights to the base row's sum (the mean over the in-range agents
        for the complete graph; a receiver with nobody in range hears zeros) and needs a base >= 0.
        ``comm.range_matrices`` builds the same matrices in torch.  None switches it off.  It composes with
        ``set_comm`` in either order; with a live (learnable) source whichever call comes second raises ValueError.
        The positions exist inside the fused episode only: ``forward`` and ``MultiAgent.act`` raise under a range."""
        from .. import comm as _comm

        if radius is None:
            self.__comm_range = None
            return
        r = _comm.check_range(radius, metric, normalize)
        if self.__comm_source:
            raise ValueError("a communication range under a live (learnable) communication source: the gradient of "
                             "a gated base matrix is not computed (set_comm with a constant matrix first)")
        if self.comm_matrix is not None:
            _comm.check_range_base(self.comm_matrix, r.normalize)
        self.__comm_range = r

    def check_no_comm_range(self, who: str) -> None:
        """The single-step surface has no positions of the emission step: RuntimeError under a range."""
        if self.__comm_range is not None:
            raise RuntimeError(f"{who}: range-limited communication (set_comm_range) runs inside the fused episode "
                               "only (EpisodeSampler / Trainer): a single step has no positions to gate the exchange "
                               "with - set_comm_range(None) for the step API")

    # ---- reference surface -------------------------------------------------------------
    @property
    def nb_class(self) -> int:
        return self.__dims["nb_class"]

    @property
    def nb_action(self) -> int:
        return self.__nb_action

    @property
    def device(self) -> th.device:
        return next(self.parameters()).device

    def random_first_state(self, nb_agents: int, batch_size: int) -> RecurrentOutput:
        """h, c, h^, c^ ~ N(0, 1), drawn in that order (reference models.py:148-159)."""
        dev = self.device
        n_b, n_a = self.__dims["n_b"], self.__dims["n_a"]
        return RecurrentOutput(
            h=th.randn(nb_agents, batch_size, n_b, device=dev),
            c=th.randn(nb_agents, batch_size, n_b, device=dev),
            h_caret=th.randn(nb_agents, batch_size, n_a, device=dev),
            c_caret=th.randn(nb_agents, batch_size, n_a, device=dev),
        )

    def zero_first_message(self, nb_agents: int, batch_size: int) -> th.Tensor:
        return th.zeros(nb_agents, batch_size, self.__dims["n_m"], device=self.device)

    def forward(
        self,
        img_patch: th.Tensor,
        msg_t: th.Tensor,
        norm_pos: th.Tensor,
        recurrent_hidden: RecurrentOutput,
    ) -> Tuple[ModelOutput, RecurrentOutput]:
        """One step of every network (reference models.py:78-138) through
        ``marl_step_forward``.  With grad enabled and a parameter (or msg / state) requiring
        grad, the step is one autograd node (``_StepFunction``) whose backward is
        ``marl_step_backward``: gradients reach the parameters and msg_t / the recurrent state."""
        self.check_no_comm_range("ModelsWrapper.forward")
        na, nb = img_patch.shape[:2]
        eng = self.hip_engine(None)
        eng.configure(na, nb, 1, (img_patch.shape[2], img_patch.shape[3] + 1, img_patch.shape[4] + 1))
        self.ensure_packed(eng)
        rh = recurrent_hidden
        state = (msg_t, rh.h, rh.c, rh.h_caret, rh.c_caret)
        if step_needs_graph(self, img_patch, norm_pos, *state, comm=eng.comm_live):
            named = list(self.named_parameters())
            probs, values, preds, msg, h, c, hc, cc = _StepFunction.apply(
                eng, img_patch, norm_pos, None, None, tuple(k for k, _ in named), eng.comm_live, *state,
                *[p for _, p in named])
        else:
            probs, values, preds, msg, h, c, hc, cc = eng.step_forward(
                img_patch, msg_t, norm_pos, rh.h, rh.c, rh.h_caret, rh.c_caret)
        return ModelOutput(probs, values, preds, msg), RecurrentOutput(h, c, hc, cc)

    # ---- HIP plumbing --------------------------------------------------------------------
    def model_spec(self, actions: Optional[List[List[int]]]) -> ModelSpec:
        cnn = self.__map_obs
        if actions is None:
            actions = [[0, 0]] * self.__nb_action
        if len(actions) != self.__nb_action:
            raise ValueError(f"model has {self.__nb_action} actions, environment {len(actions)}")
        return ModelSpec(ft_extr=cnn.hip_name, window=cnn.window, actions=[list(a) for a in actions],
                         **self.__dims)

    def hip_engine(self, actions: Optional[List[List[int]]]) -> HipEngine:
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError(
                "ModelsWrapper runs on the GPU only: move it with .to('cuda') (the HIP library "
                "is the only implementation; there is no CPU fallback)"
            )
        key = (str(dev), None if actions is None else tuple(map(tuple, actions)))
        eng = self.__engines.get(key)
        if eng is None:
            eng = HipEngine(self.model_spec(actions), dev)
            self.__engines[key] = eng
        if self.__comm_source:  # a live source: evaluated here, at every fetch (a step of an act loop is a forward)
            eng.comm_source = self.__comm_source[0]
            eng.refresh_comm()
        else:
            eng.comm_source = eng.comm_live = None
            eng.comm = self.comm_matrix  # (checked by set_comm; moved with the module)
        eng.comm_range = self.__comm_range
        eng.exploration = self.__exploration
        return eng

    def flat_state(self) -> FlatParams:
        """Flat parameter / gradient / Adam buffers; the nn.Parameters become views into the
        flat parameter buffer (re-done transparently after .to(device))."""
        dev = self.device
        named = list(self.named_parameters())
        flat = self.__flat
        ok = flat is not None and flat.params.device == dev
        if ok:
            views = flat.param_views()
            ok = all(p.data_ptr() == views[k].data_ptr() for k, p in named)
        if not ok:
            fresh = FlatParams({k: tuple(p.shape) for k, p in named}, dev)
            views = fresh.param_views()
            with th.no_grad():
                for k, p in named:
                    views[k].copy_(p.data)
                    p.data = views[k]
            if flat is not None and flat.params.device == dev and flat.numel == fresh.numel:
                fresh.exp_avg.copy_(flat.exp_avg)
                fresh.exp_avg_sq.copy_(flat.exp_avg_sq)
                if flat.ema is not None:  # (the averaged weights of optim.OptimOptions.ema_decay)
                    fresh.ema = flat.ema.clone()
                fresh.step = flat.step
            self.__flat = fresh
            self.__packed_token = {}
        return self.__flat

    def _version_token(self) -> Tuple:
        return tuple(p._version for p in self.parameters())

    def ensure_packed(self, eng: HipEngine) -> None:
        """Refresh the engine's padded / transposed weight copies if any parameter changed
        through torch (load_state_dict, an optimiser, manual edits)."""
        flat = self.flat_state()
        token = self._version_token() + (eng.weights_token(),)
        if self.__packed_token.get(id(eng)) != token:
            eng.pack(flat.param_views())
            self.__packed_token[id(eng)] = token

    def mark_updated(self, eng: HipEngine) -> None:
        """Called after the HIP Adam kernel wrote the flat buffer (no torch version bump)."""
        eng.pack(self.flat_state().param_views())
        self.__packed_token = {id(eng): self._version_token() + (eng.weights_token(),)}
