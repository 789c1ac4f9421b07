"""Thin host-side driver over libmarl_hip.so: builds ``marl_config`` structs, owns the two
workspaces the C ABI asks the caller to provide, and turns torch tensors into raw device
pointers + the current HIP stream.  PyTorch is used for device memory, streams and (in
``parallel.py``) ``torch.distributed`` only - every computation happens in the HIP library.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch as th

from . import _lib
from ._lib import MARL_NPARAMS, MarlConfig, P, check

# Conv stacks of the reference's feature extractors (networks/vision.py:55-86,123-127):
# channels entering / leaving every Conv-GroupNorm-SiLU block and the GroupNorm groups.
CNN_SPECS: Dict[str, Tuple[List[int], List[int]]] = {
    "mnist": ([1, 8, 16], [2, 4]),
    "resisc45": ([3, 16, 32, 64], [2, 4, 8]),
    "aid": ([3, 16, 32, 64, 128], [2, 4, 8, 16]),
    "worldstrat": ([3, 16, 32, 64, 128, 256], [2, 4, 8, 16, 32]),
    "skin_cancer": ([3, 16, 32, 64], [2, 4, 8]),
}

_MW = "_ModelsWrapper__"
_CNN_PREFIX = _MW + "map_obs._Generic2dCnnModule__layers."
_LSTM = "._LSTMCellWrapper__lstm."


def _mlp_names(prefix: str, tag: str, two_ln: bool) -> Dict[str, int]:
    out = {
        f"{_MW}{prefix}.0.weight": P[f"{tag}_W0"],
        f"{_MW}{prefix}.0.bias": P[f"{tag}_B0"],
        f"{_MW}{prefix}.1.weight": P[f"{tag}_LN0W" if two_ln else f"{tag}_LNW"],
        f"{_MW}{prefix}.1.bias": P[f"{tag}_LN0B" if two_ln else f"{tag}_LNB"],
        f"{_MW}{prefix}.3.weight": P[f"{tag}_W1"],
        f"{_MW}{prefix}.3.bias": P[f"{tag}_B1"],
    }
    if two_ln:
        out[f"{_MW}{prefix}.4.weight"] = P[f"{tag}_LN1W"]
        out[f"{_MW}{prefix}.4.bias"] = P[f"{tag}_LN1B"]
    return out


def state_dict_slots(n_cnn_layers: int) -> Dict[str, int]:
    """Reference state-dict key (name-mangled) -> slot of the C parameter
    table (enum in include/marl_hip.h)."""
    m: Dict[str, int] = {}
    for l in range(n_cnn_layers):
        m[f"{_CNN_PREFIX}{3 * l}.weight"] = 4 * l
        m[f"{_CNN_PREFIX}{3 * l}.bias"] = 4 * l + 1
        m[f"{_CNN_PREFIX}{3 * l + 1}.weight"] = 4 * l + 2
        m[f"{_CNN_PREFIX}{3 * l + 1}.bias"] = 4 * l + 3
    m[f"{_MW}map_pos.0.weight"] = P["POS_W"]
    m[f"{_MW}map_pos.0.bias"] = P["POS_B"]
    m[f"{_MW}map_pos.1.weight"] = P["POS_LNW"]
    m[f"{_MW}map_pos.1.bias"] = P["POS_LNB"]
    m.update(_mlp_names("encode_msg", "ENC", True))
    m.update(_mlp_names("decode_msg", "DEC", True))
    for unit, tag in (("belief_unit", "LB"), ("action_unit", "LA")):
        m[f"{_MW}{unit}{_LSTM}weight_ih"] = P[f"{tag}_WIH"]
        m[f"{_MW}{unit}{_LSTM}weight_hh"] = P[f"{tag}_WHH"]
        m[f"{_MW}{unit}{_LSTM}bias_ih"] = P[f"{tag}_BIH"]
        m[f"{_MW}{unit}{_LSTM}bias_hh"] = P[f"{tag}_BHH"]
    m.update(_mlp_names("policy", "POL", False))
    m.update(_mlp_names("critic", "CRI", False))
    m.update(_mlp_names("predict", "PRE", False))
    return m


@dataclass
class ModelSpec:
    """Everything ``marl_config`` needs that does not depend on the batch."""

    ft_extr: str
    window: int
    n_b: int
    n_a: int
    n_m: int
    n_m_o: int
    n_d: int
    nb_class: int
    nlb: int
    nla: int
    actions: List[List[int]] = field(
        default_factory=lambda: [[1, 0], [-1, 0], [0, 1], [0, -1]]
    )

    def config(self, nb_agents: int, batch: int, nb_steps: int, img_c: int, h: int, w: int,
               img_u8: bool = False) -> MarlConfig:
        if self.ft_extr not in CNN_SPECS:
            raise ValueError(
                f'feature extractor "{self.ft_extr}" has no HIP implementation '
                f"(supported: {sorted(CNN_SPECS)})"
            )
        ch, groups = CNN_SPECS[self.ft_extr]
        if len(self.actions) > _lib.MARL_MAX_ACTIONS:
            raise ValueError("too many actions")
        cfg = MarlConfig()
        cfg.nb_agents, cfg.batch, cfg.nb_steps = nb_agents, batch, nb_steps
        cfg.img_c, cfg.img_h, cfg.img_w = img_c, h, w
        cfg.window = self.window
        cfg.cnn_layers = len(groups)
        for i, c in enumerate(ch):
            cfg.cnn_ch[i] = c
        for i, g in enumerate(groups):
            cfg.cnn_groups[i] = g
        cfg.n_b, cfg.n_a, cfg.n_m, cfg.n_m_o, cfg.n_d = self.n_b, self.n_a, self.n_m, self.n_m_o, self.n_d
        cfg.nb_action, cfg.nb_class = len(self.actions), self.nb_class
        cfg.nlb, cfg.nla = self.nlb, self.nla
        for j, (d0, d1) in enumerate(self.actions):
            cfg.actions[j][0], cfg.actions[j][1] = d0, d1
        cfg.img_u8 = int(img_u8)
        return cfg

    @property
    def n_cnn_layers(self) -> int:
        return len(CNN_SPECS[self.ft_extr][1])


_U64 = (1 << 64) - 1

# Layout-affecting knobs (marl_tune: tile plans, split-K targets, mfma_split ...) change the sizes
# of regions INSIDE the episode workspace.  The library recomputes the layout on every call but
# never sees the workspace size, so a buffer allocated before a knob changed must not be reused:
# ``tune`` bumps this epoch and every HipEngine drops its cached workspaces when it differs.
_tune_epoch = 0


def tune(key: str, value: int) -> None:
    """marl_tune + invalidation of every engine's cached workspaces (set knobs through this)."""
    global _tune_epoch
    check(_lib.load().marl_tune(key.encode(), int(value)))
    _tune_epoch += 1


def _nbytes(t: th.Tensor) -> int:
    return t.numel() * t.element_size()


def _ptr(t: Optional[th.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(device: th.device) -> int:
    return th.cuda.current_stream(device).cuda_stream


def _need(t: th.Tensor, dtype: th.dtype, name: str) -> th.Tensor:
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} lives on {t.device}: the HIP path only runs on a GPU "
            "(there is no CPU implementation in this package)"
        )
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


@dataclass
class EpisodeTensors:
    step_preds: th.Tensor
    step_log_probas: th.Tensor
    step_values: th.Tensor
    step_pos: th.Tensor
    step_actions: th.Tensor
    # [Ns,Na,Nb,nA]: the distribution every step sampled from (episode_forward(probs=True)), else None
    step_probs: Optional[th.Tensor] = None


class HipEngine:
    """Owns workspaces for one model on one device and issues the C ABI calls."""

    def __init__(self, spec: ModelSpec, device: th.device) -> None:
        self.lib = _lib.load()
        self.spec = spec
        self.device = th.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("HipEngine needs a GPU device (torch 'cuda' == HIP on ROCm)")
        self.slots = state_dict_slots(spec.n_cnn_layers)
        self._wws: Optional[th.Tensor] = None
        self._wws_epoch = _tune_epoch   # tune epoch the weights workspace was laid out under
        self._wws_bytes = 0
        # bumped whenever the weights workspace is (re)allocated: its packed copies are gone and whoever
        # packed last (FusedA2C, ModelsWrapper.ensure_packed) must pack again before the next call
        self.weights_generation = 0
        # what pack() last filled: the generation it packed into and the tensors it packed from (a
        # direct user doing pack -> tune -> forward used to get a freshly ZEROED weights workspace, silently)
        self._packed_generation: Optional[int] = None
        self._packed_params: Optional[Dict[str, th.Tensor]] = None
        self._ews: Dict[Tuple, th.Tensor] = {}
        self._cfg_key: Optional[Tuple] = None
        self.cfg: Optional[MarlConfig] = None
        self._packed_version: Optional[int] = None
        self._tune_seen = _tune_epoch
        # what the last training rollout left behind for backward: the episode workspace holds
        # its activations, `_fwd_img` keeps its image batch alive (the first convolution's weight
        # gradient re-gathers the patches), `fwd_generation` lets callers detect a stale backward
        self.fwd_generation = 0
        self.pack_generation = 0       # bumped by pack(): a live episode's backward needs ITS weights
        self._ws_pool: Dict[tuple, list] = {}  # released per-episode training workspaces (autograd path)
        self._fwd_img: Optional[th.Tensor] = None
        self._fwd_key: Optional[Tuple] = None
        self._clip_scratch: Optional[th.Tensor] = None  # partial sums + the norm of grad_clip
        # communication graph of the message exchange (comm.py): fp32 [Na, Na] on this device, None = the mean
        # over the other agents.  The library's matrix is per-process state: it is installed around every call
        # that aggregates and cleared behind it, so engines with different graphs never see each other's.
        self.comm: Optional[th.Tensor] = None
        # a LIVE source of that matrix (a tensor that requires grad, a module or a callable; held by reference):
        # ``refresh_comm`` evaluates it - for every forward, by whoever starts one - into ``comm`` (the detached fp32
        # value the library reads) and ``comm_live`` (the matrix as the source gave it, attached to its graph: what the
        # autograd nodes take as their input and what a trainer calls ``backward(d_comm)`` on)
        self.comm_source = None
        self.comm_live: Optional[th.Tensor] = None
        self._comm_scratch: Optional[th.Tensor] = None  # the partials of marl_comm_grad (pooled, grown on demand)
        # range-limited communication (comm.CommRange, None = off): the matrix above - or comm.full(Na) without one -
        # is the base the kernels gate per (step, image) by the agents' positions.  Installed and cleared with it.
        self.comm_range = None
        self._comm_full: Optional[th.Tensor] = None  # the base of a range without a matrix (cached per agent count)
        # exploration controls (explore.Exploration; the default = the plain policy, sampled): like the matrix,
        # per-process state of the library - installed around every call that samples or back-propagates through
        # the sampling and cleared behind it; at the default nothing is installed and nothing more is called
        from . import explore as _explore

        self.exploration = _explore.DEFAULT
        # options of the vote error and the rewards (set_class_loss: a class_loss.ClassLoss, None = the reference's
        # loss): per-process state of the library too - installed around every loss call and cleared behind it.  The
        # device copies of the class / step weights (ClassLoss -> (w, s), either None) are made once per setting and
        # kept for the engine's life - a captured graph keeps the pointers, so none is ever dropped: nC + Ns floats
        # per DISTINCT setting, which is expected to be one or a few per run (not a per-step schedule)
        self.class_loss = None
        # a target distribution per image in place of the labels (set_soft_targets: fp32 [Nb, nC] on the device, None =
        # the labels), installed and cleared around each loss call like the options above
        self.soft_targets: Optional[th.Tensor] = None
        self._class_loss_dev: Dict[object, Tuple[Optional[th.Tensor], Optional[th.Tensor]]] = {}

    # -- communication graph ----------------------------------------------------------
    def set_comm(self, matrix) -> None:
        """The mixing matrix of the message exchange (row = receiver, column = sender; ``comm.py`` builds the usual
        graphs) for every later episode / step call of this engine; None restores the mean over the other agents.
        Checked here, before anything is enqueued: fp32-convertible square finite matrix on the engine's device, at
        most ``comm.MAX_AGENTS`` agents, and the configured number of agents if the engine is configured.
        A tensor that requires grad, a module or a callable that returns the matrix is a LIVE source
        (``comm.is_live``): kept by reference and evaluated by ``refresh_comm`` (shape, dtype and device are checked
        at every evaluation; finiteness is not - that would synchronise)."""
        from . import comm as _comm

        if matrix is not None and self.comm_range is not None:
            if _comm.is_live(matrix):
                raise ValueError("a live (learnable) communication source under a communication range: the gradient "
                                 "of a gated base matrix is not computed (set_comm_range(None) first)")
            _comm.check_range_base(_comm.validate(matrix, None), self.comm_range.normalize)
        self.comm_source = self.comm_live = None
        if matrix is None:
            self.comm = None
            return
        if _comm.is_live(matrix):
            self.comm_source = matrix
            self.refresh_comm()
            return
        m = _comm.validate(matrix, None)
        if m.device != self.device:
            raise ValueError(f"communication matrix lives on {m.device}, the engine on {self.device}")
        if self.cfg is not None and m.shape[0] != self.cfg.nb_agents:
            raise ValueError(f"communication matrix is {tuple(m.shape)} but the engine is configured for "
                             f"{self.cfg.nb_agents} agents")
        self.comm = m.clone()  # (never the caller's storage)

    def set_comm_range(self, radius, metric: str = "chebyshev", normalize: bool = True) -> None:
        """Range-limited communication for every later episode call of this engine: agents hear each other within
        ``radius`` pixels (``comm.range_matrices`` has the semantics; None switches it off).  The matrix of
        ``set_comm`` - ``comm.full(Na)`` without one - is the base; a live source cannot be gated, and
        ``normalize=True`` needs a base >= 0: ValueError, from whichever call comes second.  The step calls
        (``step_forward`` / ``step_backward``) raise under a range: only the fused episode knows the positions."""
        from . import comm as _comm

        if radius is None:
            self.comm_range = None
            return
        r = _comm.check_range(radius, metric, normalize)
        if self.comm_source is not None:
            raise ValueError("a communication range under a live (learnable) communication source: the gradient of "
                             "a gated base matrix is not computed (set_comm with a constant matrix first)")
        if self.comm is not None:
            _comm.check_range_base(self.comm, r.normalize)
        self.comm_range = r

    def _range_base(self) -> th.Tensor:
        """The base matrix a range gates: this engine's matrix, or the complete graph of the configured agents."""
        if self.comm is not None:
            return self.comm
        from . import comm as _comm

        na = self.cfg.nb_agents
        if na > _comm.MAX_AGENTS:
            raise ValueError(f"communication range for {na} agents: at most {_comm.MAX_AGENTS} are supported")
        if self._comm_full is None or self._comm_full.shape[0] != na:
            self._comm_full = _comm.full(na).to(self.device)
        return self._comm_full

    def refresh_comm(self) -> Optional[th.Tensor]:
        """Evaluates the live source (if there is one) for the forward that is about to run: ``comm`` becomes its
        detached fp32 value, ``comm_live`` the graph-attached matrix, which is also returned (None: constant / mean)."""
        if self.comm_source is None:
            self.comm_live = None
            return None
        from . import comm as _comm

        # (the agent count is checked by configure() and, before anything is enqueued, by the library)
        live, value = _comm.evaluate(self.comm_source, None, self.device)
        self.comm, self.comm_live = value, live
        return live

    def comm_grad(self, ws: th.Tensor, nb_steps: int, d_comm: th.Tensor) -> th.Tensor:
        """marl_comm_grad: the gradient with respect to the mixing matrix out of the workspace a backward just
        finished on (``nb_steps`` = the steps of its layout: the episode's, 1 for a step workspace) into ``d_comm``
        ([Na, Na] fp32, overwritten).  The partials' scratch is pooled by the engine."""
        cfg = self.cfg
        assert cfg is not None
        if self.comm is None:
            raise ValueError("comm_grad: the engine has no communication matrix (the mean has no matrix to learn)")
        na = cfg.nb_agents
        if (not isinstance(d_comm, th.Tensor) or tuple(d_comm.shape) != (na, na) or d_comm.dtype != th.float32 or
                d_comm.device != self.device or not d_comm.is_contiguous()):
            raise ValueError(f"comm_grad: d_comm must be a contiguous fp32 [{na}, {na}] tensor on {self.device}")
        lay = MarlConfig.from_buffer_copy(cfg)
        lay.nb_steps = nb_steps
        need = self.lib.marl_comm_grad_scratch_bytes(C.byref(lay))
        if self._comm_scratch is None or _nbytes(self._comm_scratch) < need:
            self._comm_scratch = th.empty(need // 4 + 1, dtype=th.float32, device=self.device)
        sc, wws = self._comm_scratch, self.packed_weights_ws()
        self._agg(self.lib.marl_comm_grad, C.byref(cfg), wws.data_ptr(), _nbytes(wws), ws.data_ptr(), _nbytes(ws),
                  int(nb_steps), d_comm.data_ptr(), sc.data_ptr(), _nbytes(sc), _stream(self.device))
        return d_comm

    def set_exploration(self, temperature=1.0, eps=0.0, greedy=False) -> None:
        """The behaviour policy of every later sampling call of this engine (``explore.py``): pi_b =
        (1 - eps) softmax(z / temperature) + eps / nA, sampled or - ``greedy`` - its argmax.  ValueError for a
        temperature that is not finite and > 0 or an eps outside [0, 0.5].  A backward runs under the setting of
        ITS forward: the autograd nodes keep it; a direct caller of ``episode_backward`` / ``step_backward`` leaves
        it unchanged in between."""
        from . import explore as _explore

        self.exploration = _explore.check(temperature, eps, greedy)

    def _agg(self, fn, *args) -> None:
        """A library call that samples, back-propagates through the sampling or aggregates messages: under this
        engine's exploration controls and matrix, where it has them."""
        x = self.exploration
        if x.is_default:
            self._agg_comm(fn, *args)
            return
        check(self.lib.marl_policy_explore(x.temperature, x.eps, int(x.greedy)))
        try:
            self._agg_comm(fn, *args)
        finally:
            self.lib.marl_policy_explore(1.0, 0.0, 0)

    def set_class_loss(self, class_loss=None) -> None:
        """The options of the vote error and the rewards (a ``class_loss.ClassLoss``: class weights, label smoothing,
        step weights, cost-sensitive rewards) for every later ``a2c_loss`` / ``advantages`` / ``ppo_loss`` of this
        engine; None restores the reference's loss.  Handled like ``set_exploration``: kept here, installed in the
        library (marl_class_loss) around each of those calls and cleared behind it.  Every distinct setting keeps
        its device copy of the weights (nC + Ns floats) for the engine's life, because a captured graph may read it:
        use one or a few settings per run, not a new one per step.  ValueError for anything but a
        ``ClassLoss`` and - here if the engine is configured, else at the call - for one whose classes / steps are not
        the configured ones."""
        from . import class_loss as _cl

        if class_loss is not None and not isinstance(class_loss, _cl.ClassLoss):
            raise ValueError(f"class_loss must be a class_loss.ClassLoss or None, got {type(class_loss).__name__}")
        if class_loss is not None and self.cfg is not None:
            self._check_class_loss(class_loss)
        self.class_loss = class_loss

    def _check_class_loss(self, c) -> None:
        cfg = self.cfg
        if c.nb_class != cfg.nb_class or c.nb_steps != cfg.nb_steps:
            raise ValueError(f"class_loss is for {c.nb_class} classes / {c.nb_steps} steps, the engine is configured "
                             f"for {cfg.nb_class} / {cfg.nb_steps}")

    def set_soft_targets(self, q: Optional[th.Tensor] = None, check_values: bool = True) -> None:
        """A target distribution per image, ``q`` fp32 ``[Nb, nC]`` on this engine's device, for every later
        ``a2c_loss`` / ``advantages`` / ``ppo_loss`` of this engine in place of the labels (CutMix, Mixup, a teacher's
        distribution; include/marl_hip_softtargets.h); None restores the labels.  Kept here, installed in the library
        (marl_soft_targets) around each of those calls and cleared behind it.  The tensor is not copied: the launches
        read it, and a captured graph reads the capturing call's tensor.  Checked: dtype, device, contiguous, the
        configured sizes (here if the engine is configured, else at the call), and - ``check_values``, one host
        synchronisation - finite, >= 0, no all-zero row."""
        if q is None:
            self.soft_targets = None
            return
        if not isinstance(q, th.Tensor):
            raise TypeError(f"soft targets must be a tensor or None, got {type(q).__name__}")
        if q.dtype != th.float32:
            raise TypeError(f"soft targets must be float32, got {q.dtype}")
        if not q.is_cuda:
            raise RuntimeError(f"soft targets live on {q.device}, the engine on {self.device}: the HIP path only "
                               "reads device memory")
        if q.dim() != 2 or not q.is_contiguous():
            raise ValueError(f"soft targets must be a contiguous [Nb, nC] tensor, got {tuple(q.shape)}")
        if self.cfg is not None:
            self._check_soft_targets(q)
        if check_values:
            ok = th.isfinite(q).all() & (q >= 0).all() & (q > 0).any(dim=1).all()
            if not bool(ok):
                raise ValueError("soft targets must be finite and >= 0, and no row may be all zero")
        self.soft_targets = q

    def _check_soft_targets(self, q: th.Tensor) -> None:
        cfg = self.cfg
        if tuple(q.shape) != (cfg.batch, cfg.nb_class):
            raise ValueError(f"soft targets are {tuple(q.shape)}, the engine is configured for batch {cfg.batch} and "
                             f"{cfg.nb_class} classes")

    def _loss_call(self, fn, *args) -> None:
        """A loss entry under this engine's ``soft_targets`` and ``class_loss`` (both None: the plain call and nothing
        more).  Checked against the configured sizes before anything is enqueued."""
        q = self.soft_targets
        if q is None:
            self._class_loss_call(fn, *args)
            return
        self._check_soft_targets(q)
        check(self.lib.marl_soft_targets(q.data_ptr(), q.shape[0], q.shape[1]))
        try:
            self._class_loss_call(fn, *args)
        finally:
            self.lib.marl_soft_targets(None, 0, 0)

    def _class_loss_call(self, fn, *args) -> None:
        """A loss entry under this engine's ``class_loss`` (None, or one with nothing given: the plain call and
        nothing more).  Checked against the configured classes / steps before anything is enqueued."""
        c = self.class_loss
        if c is None or c.is_default:
            check(fn(*args))
            return
        self._check_class_loss(c)
        dev = self._class_loss_dev.get(c)
        if dev is None:
            dev = self._class_loss_dev[c] = tuple(
                None if v is None else th.tensor(v, dtype=th.float32, device=self.device)
                for v in (c.class_weights, c.step_weights))
        w, s = dev
        check(self.lib.marl_class_loss(_ptr(w), c.nb_class if w is not None else 0, C.c_float(c.label_smoothing),
                                       _ptr(s), c.nb_steps if s is not None else 0, int(c.weight_rewards)))
        try:
            check(fn(*args))
        finally:
            self.lib.marl_class_loss(None, 0, C.c_float(0.0), None, 0, 0)

    def _agg_comm(self, fn, *args) -> None:
        """A library call that aggregates messages: under this engine's matrix, if it has one."""
        r = self.comm_range
        m = self.comm if r is None else self._range_base()
        if m is None:
            check(fn(*args))
            return
        check(self.lib.marl_comm_matrix(m.data_ptr(), m.shape[0]))
        try:
            if r is not None:
                check(self.lib.marl_comm_range(r.radius, r.metric_id, int(r.normalize)))
            check(fn(*args))
        finally:
            self.lib.marl_comm_matrix(None, 0)
            self.lib.marl_comm_range(-1, 0, 1)

    def plan_query(self, key: str, train: bool = True) -> int:
        """marl_plan_query under this engine's communication matrix and exploration controls."""
        v = C.c_int(0)
        self._agg(self.lib.marl_plan_query, C.byref(self.cfg), int(train), key.encode(), C.byref(v))
        return v.value

    # -- configuration / workspaces -------------------------------------------------
    def configure(self, nb_agents: int, batch: int, nb_steps: int, img_shape: Sequence[int],
                  img_u8: bool = False) -> MarlConfig:
        if self.comm is not None and self.comm.shape[0] != nb_agents:
            raise ValueError(f"configure: {nb_agents} agents, but the communication matrix is "
                             f"{tuple(self.comm.shape)} (set_comm(None) or a matrix of that size first)")
        key = (nb_agents, batch, nb_steps, tuple(img_shape), bool(img_u8))
        if key != self._cfg_key:
            c, h, w = img_shape
            self.cfg = self.spec.config(nb_agents, batch, nb_steps, c, h, w, img_u8)
            self._cfg_key = key
            # The weights layout is a function of the MODEL and the knobs only (csrc/episode.hip,
            # g3_model_ok) - belt and braces: should a configuration ever ask for another size, the packed
            # copies of the old layout must not be read through the new one.
            if self._wws is not None and self._sizes(True)[0] != self._wws_bytes:
                self._wws = None
        assert self.cfg is not None
        return self.cfg

    def _sizes(self, train: bool) -> Tuple[int, int]:
        wb, eb = C.c_size_t(0), C.c_size_t(0)
        check(self.lib.marl_workspace_sizes(C.byref(self.cfg), int(train), C.byref(wb), C.byref(eb)))
        return wb.value, eb.value

    def weights_ws(self) -> th.Tensor:
        if self._wws is not None and self._wws_epoch != _tune_epoch:
            # a knob moved (g3, g3_min_units, mfma_split ... decide which weight images exist): the old
            # buffer has the old layout AND the old contents - drop it, and make every packer pack again
            self._wws = None
        if self._wws is None:
            wb, _ = self._sizes(True)
            self._wws = th.zeros(wb // 4 + 64, dtype=th.float32, device=self.device)
            self._wws_epoch = _tune_epoch
            self._wws_bytes = wb
            self.weights_generation += 1
        return self._wws

    def packed_weights_ws(self) -> th.Tensor:
        """The weights workspace for a compute call: if a knob change dropped the buffer pack() filled, the
        parameters of the last pack() are packed again into the new layout (their CURRENT values - they are the
        caller's live tensors); with nothing ever packed the call fails instead of running on zeros."""
        wws = self.weights_ws()
        if self._packed_generation != self.weights_generation:
            if self._packed_params is None:
                raise RuntimeError("HipEngine: no weights packed - call pack(params) before a compute call")
            self.pack(self._packed_params)
            wws = self.weights_ws()
        return wws

    def weights_token(self) -> int:
        """Generation of the weights workspace AFTER applying pending invalidations (callers compare it
        with the value they saw when they last packed)."""
        self.weights_ws()
        return self.weights_generation

    def episode_ws(self, train: bool) -> th.Tensor:
        if self._tune_seen != _tune_epoch:  # a layout knob changed: sizes may have moved
            self._ews.clear()
            self._fwd_img = None
            self._tune_seen = _tune_epoch
        key = (self._cfg_key, train)
        ws = self._ews.get(key)
        if ws is None:
            _, eb = self._sizes(train)
            # keep at most one workspace per mode: shapes rarely change
            for k in [k for k in self._ews if k[1] == train]:
                del self._ews[k]
            ws = th.zeros(eb // 4 + 64, dtype=th.float32, device=self.device)
            self._ews[key] = ws
        return ws

    def train_ws_acquire(self) -> th.Tensor:
        """A training workspace owned by ONE episode (the autograd path: several rollouts of the same
        model may be alive at once, as with the reference's autograd graph - core/episode.py:84 there).
        Released workspaces of the current configuration are reused; the fused Trainer keeps using
        the engine's own workspace (``episode_ws``)."""
        key = (self._cfg_key, _tune_epoch)
        for k in [k for k in self._ws_pool if k != key]:
            del self._ws_pool[k]  # other shape / layout: free the memory
        free = self._ws_pool.setdefault(key, [])
        if free:
            return free.pop()
        _, eb = self._sizes(True)
        ws = th.zeros(eb // 4 + 64, dtype=th.float32, device=self.device)
        ws._marl_key = key
        return ws

    def train_ws_release(self, ws: th.Tensor) -> None:
        key = getattr(ws, "_marl_key", None)
        if key == (self._cfg_key, _tune_epoch) and len(self._ws_pool.setdefault(key, [])) < 2:
            self._ws_pool[key].append(ws)

    def _table(self, tensors: Dict[str, th.Tensor]) -> "C.Array":
        arr = (C.c_void_p * MARL_NPARAMS)()
        for name, slot in self.slots.items():
            t = tensors[name]
            if not t.is_cuda or t.dtype != th.float32 or not t.is_contiguous():
                raise RuntimeError(f"parameter {name} must be a contiguous fp32 GPU tensor")
            arr[slot] = t.data_ptr()
        return arr

    def set_heads_event(self, hip_event: Optional[int]) -> None:
        """marl_backward_heads_event: the event episode_backward records once the heads' parameter gradients are
        final (parallel.BucketedGradAllReduce); None clears it."""
        check(self.lib.marl_backward_heads_event(hip_event))

    # -- calls ----------------------------------------------------------------------
    def pack(self, params: Dict[str, th.Tensor]) -> None:
        """marl_pack_weights: refresh the padded / transposed copies after an update."""
        assert self.cfg is not None, "configure() first"
        wws = self.weights_ws()
        check(self.lib.marl_pack_weights(C.byref(self.cfg), self._table(params), wws.data_ptr(), _nbytes(wws),
                                         _stream(self.device)))
        self.pack_generation += 1
        self._packed_generation = self.weights_generation
        self._packed_params = params

    def episode_forward(
        self, img: th.Tensor, pos0: th.Tensor, h0: th.Tensor, c0: th.Tensor, hc0: th.Tensor,
        cc0: th.Tensor, noise: Optional[th.Tensor], forced_actions: Optional[th.Tensor] = None,
        train: bool = True, rng: Optional[Tuple[int, int]] = None,
        out: Optional[EpisodeTensors] = None, counters: Optional[th.Tensor] = None,
        ws: Optional[th.Tensor] = None, probs: bool = False,
    ) -> EpisodeTensors:
        """``noise`` = injected Exp(1) draws [Ns,Na,Nb,nA] (parity mode); ``noise=None`` with
        ``rng=(seed, offset)`` draws them inside the sampling kernel (perf mode).  ``probs``: also
        ``step_probs`` (marl_episode_forward_probs; an ``out`` that already holds the tensor asks for it too)."""
        cfg = self.cfg
        assert cfg is not None
        na, nb, ns = cfg.nb_agents, cfg.batch, cfg.nb_steps
        dev = self.device
        img = _need(img, th.uint8 if cfg.img_u8 else th.float32, "img")
        pos0 = _need(pos0, th.int64, "pos0")
        h0, c0, hc0, cc0 = (_need(t, th.float32, n) for t, n in
                            ((h0, "h0"), (c0, "c0"), (hc0, "hc0"), (cc0, "cc0")))
        if noise is not None:
            noise = _need(noise, th.float32, "noise")
        if forced_actions is not None:
            forced_actions = _need(forced_actions, th.int64, "forced_actions")
        if noise is None and forced_actions is None and rng is None:
            raise ValueError("episode_forward needs noise, forced_actions or rng=(seed, offset)")
        seed, offset = rng if rng is not None else (0, 0)
        if out is None:  # (graph capture passes persistent output tensors: nothing may allocate)
            out = self.new_outputs(probs)
        elif probs and out.step_probs is None:
            raise ValueError("episode_forward(probs=True): `out` has no step_probs tensor (new_outputs(True))")
        wws, ews = self.packed_weights_ws(), (ws if ws is not None else self.episode_ws(train))
        head = (C.byref(cfg), wws.data_ptr(), _nbytes(wws), ews.data_ptr(), _nbytes(ews),
                img.data_ptr(), pos0.data_ptr(), h0.data_ptr(), c0.data_ptr(), hc0.data_ptr(),
                cc0.data_ptr(), _ptr(noise), _ptr(forced_actions), seed & _U64, offset & _U64,
                _ptr(counters), out.step_preds.data_ptr(), out.step_log_probas.data_ptr(), out.step_values.data_ptr(),
                out.step_pos.data_ptr(), out.step_actions.data_ptr())
        if out.step_probs is None:
            self._agg(self.lib.marl_episode_forward, *head, int(train), _stream(dev))
        else:
            self._agg(self.lib.marl_episode_forward_probs, *head, out.step_probs.data_ptr(), int(train), _stream(dev))
        if train and ws is None:  # (an episode with its own workspace does not touch the engine's)
            self.fwd_generation += 1
            self._fwd_img = img
            self._fwd_key = self._cfg_key
        return out

    def new_outputs(self, probs: bool = False) -> EpisodeTensors:
        cfg = self.cfg
        assert cfg is not None
        na, nb, ns, dev = cfg.nb_agents, cfg.batch, cfg.nb_steps, self.device
        return EpisodeTensors(
            th.empty(ns, na, nb, cfg.nb_class, device=dev),
            th.empty(ns, na, nb, device=dev),
            th.empty(ns, na, nb, device=dev),
            th.empty(ns, na, nb, 2, dtype=th.int64, device=dev),
            th.empty(ns, na, nb, dtype=th.int64, device=dev),
            th.empty(ns, na, nb, cfg.nb_action, device=dev) if probs else None,
        )

    def episode_backward(
        self, g_preds: Optional[th.Tensor], g_logp: Optional[th.Tensor],
        g_values: Optional[th.Tensor], grads: Dict[str, th.Tensor],
        generation: Optional[int] = None,
        ws: Optional[th.Tensor] = None, img: Optional[th.Tensor] = None,
        d_img: Optional[th.Tensor] = None, g_probs: Optional[th.Tensor] = None,
        d_comm: Optional[th.Tensor] = None,
    ) -> None:
        """Backward of the LAST training rollout.  `generation` (the value of
        ``fwd_generation`` right after that rollout) makes a stale call fail loudly: the saved
        activations live in the single training workspace, which a later rollout overwrites.
        ``d_img`` ([Nb,C,H,W] fp32, overwritten): also the gradient w.r.t. the image batch
        (marl_episode_backward_img); None: the plain entry, nothing extra is launched.
        ``g_probs`` ([Ns,Na,Nb,nA] fp32): dL/d(step_probs) (marl_episode_backward_probs, with or without ``d_img``);
        None: the entries above.
        ``d_comm`` ([Na,Na] fp32, overwritten): also the gradient w.r.t. the mixing matrix (marl_comm_grad, two
        launches behind the backward on the same workspace); None: nothing more is launched."""
        cfg = self.cfg
        assert cfg is not None
        if d_comm is not None and self.comm is None:
            raise ValueError("episode_backward(d_comm=...): the engine has no communication matrix")
        if d_comm is not None and self.comm_range is not None:
            raise ValueError("episode_backward(d_comm=...): under a communication range the gradient of the base "
                             "matrix is not computed")
        if g_probs is not None:
            want = (cfg.nb_steps, cfg.nb_agents, cfg.batch, cfg.nb_action)
            if not isinstance(g_probs, th.Tensor) or tuple(g_probs.shape) != want:
                raise RuntimeError(f"episode_backward: g_probs must be a tensor of shape {want}, got "
                                   f"{tuple(getattr(g_probs, 'shape', ()))}")
            if g_probs.device != self.device:
                raise RuntimeError(f"episode_backward: g_probs lives on {g_probs.device}, the episode on "
                                   f"{self.device}")
            g_probs = _need(g_probs, th.float32, "g_probs")
        if d_img is not None:
            d_img = _need(d_img, th.float32, "d_img")
            if cfg.img_u8 or tuple(d_img.shape) != (cfg.batch, cfg.img_c, cfg.img_h, cfg.img_w):
                raise RuntimeError("episode_backward: d_img needs a float image batch of the configured shape")

        if ws is not None:  # an episode that owns its workspace (autograd path)
            if getattr(ws, "_marl_key", None) != (self._cfg_key, _tune_epoch) or img is None:
                raise RuntimeError(
                    "episode_backward: the engine was re-configured (other batch size / image shape / "
                    "layout knob) since this episode's rollout - its workspace no longer fits")
        else:
            if self._fwd_img is None or self._fwd_key != self._cfg_key:
                raise RuntimeError(
                    "episode_backward without a matching training rollout: the engine was "
                    "re-configured (other batch size / image shape) or never ran episode_forward("
                    "train=True) - its workspace no longer holds this episode's activations")
            if generation is not None and generation != self.fwd_generation:
                raise RuntimeError(
                    "episode_backward for an episode whose saved activations were overwritten by a "
                    "later training rollout (one live episode per engine: call backward before the "
                    "next run_episode, or accumulate gradients across backward calls instead)")
        gp, gl, gv = (None if g is None else _need(g, th.float32, name)
                      for g, name in ((g_preds, "g_preds"), (g_logp, "g_logp"), (g_values, "g_values")))
        wws = self.packed_weights_ws()
        ews, image = (self.episode_ws(True), self._fwd_img) if ws is None else (ws, img)
        head = (C.byref(cfg), wws.data_ptr(), _nbytes(wws), ews.data_ptr(), _nbytes(ews), image.data_ptr(),
                _ptr(gp), _ptr(gl), _ptr(gv), self._table(grads))
        if g_probs is not None:
            self._agg(self.lib.marl_episode_backward_probs, *head, _ptr(d_img), g_probs.data_ptr(),
                      _stream(self.device))
        elif d_img is None:
            self._agg(self.lib.marl_episode_backward, *head, _stream(self.device))
        else:
            self._agg(self.lib.marl_episode_backward_img, *head, d_img.data_ptr(), _stream(self.device))
        if d_comm is not None:
            self.comm_grad(ews, cfg.nb_steps, d_comm)

    def a2c_loss(
        self, out: EpisodeTensors, y: th.Tensor, gamma: float, phase: int = 0,
        bufs: Optional[Tuple[th.Tensor, ...]] = None, entropy_coef: float = 0.0,
    ) -> Tuple[th.Tensor, ...]:
        """Returns (g_preds, g_logp, g_values, scalars[4], adv_stats[3] float64).
        Under ``set_class_loss`` (here, in ``advantages`` and in ``ppo_loss``): class weights, label smoothing and step
        weights of the vote error, cost-sensitive rewards.
        ``entropy_coef`` > 0 (marl_a2c_loss_entropy_fwd_bwd; ``out.step_probs`` needed): the loss minus
        ``entropy_coef * mean_{a,b} sum_t H``; returns (g_preds, g_logp, g_values, scalars[5], adv_stats, g_probs)
        with scalars[4] = the mean entropy.  0: the plain entry."""
        cfg = self.cfg
        assert cfg is not None
        dev = self.device
        if not entropy_coef >= 0.0:
            raise ValueError(f"entropy_coef must be >= 0, got {entropy_coef}")
        y = _need(y, th.int64, "y")
        ent = entropy_coef > 0.0
        if ent and out.step_probs is None:
            raise ValueError("a2c_loss(entropy_coef > 0) needs the episode's step_probs: episode_forward(probs=True)")
        if bufs is None:
            bufs = self.new_loss_bufs(out, ent)
        if ent and (len(bufs) != 6 or bufs[3].numel() != 5 or bufs[5].shape != out.step_probs.shape):
            raise ValueError("a2c_loss(entropy_coef > 0): buffers from new_loss_bufs(out, True) needed")
        gp, gl, gv, sc, st = bufs[:5] if ent else bufs
        ews = self.episode_ws(True)
        entry, bonus, g_bonus = self.lib.marl_a2c_loss_fwd_bwd, (), ()
        if ent:  # the same argument list with (probs, coef) and g_probs slotted in
            entry = self.lib.marl_a2c_loss_entropy_fwd_bwd
            bonus = (_need(out.step_probs, th.float32, "step_probs").data_ptr(), C.c_float(entropy_coef))
            g_bonus = (bufs[5].data_ptr(),)
        self._loss_call(
            entry,
            C.byref(cfg), ews.data_ptr(), _nbytes(ews), out.step_preds.data_ptr(),
            out.step_log_probas.data_ptr(), out.step_values.data_ptr(), y.data_ptr(),
            C.c_float(gamma), *bonus, gp.data_ptr(), gl.data_ptr(), gv.data_ptr(), *g_bonus,
            sc.data_ptr(), st.data_ptr(), phase, _stream(dev))
        return bufs

    def _grad_bufs(self, out: EpisodeTensors, n_scalars: int) -> Tuple[th.Tensor, ...]:
        """(g_preds, g_logp, g_values, scalars[n_scalars], adv_stats[3] float64): what both loss passes write."""
        return (
            th.empty_like(out.step_preds), th.empty_like(out.step_log_probas),
            th.empty_like(out.step_values), th.zeros(n_scalars, device=self.device),
            th.zeros(3, dtype=th.float64, device=self.device),
        )

    def new_loss_bufs(self, out: EpisodeTensors, entropy: bool = False) -> Tuple[th.Tensor, ...]:
        """The output tensors of ``a2c_loss`` (persistent ones for a trainer / a captured graph)."""
        bufs = self._grad_bufs(out, 5 if entropy else 4)
        return bufs + (th.empty_like(out.step_probs),) if entropy else bufs

    # -- PPO: GAE(lambda) advantages, clipped surrogate, global-norm clipping ---------------------------------
    def new_ppo_bufs(self, out: EpisodeTensors, entropy: bool = False) -> Tuple[th.Tensor, ...]:
        """The tensors ``advantages`` and ``ppo_loss`` write (persistent ones for a trainer):
        (g_preds, g_logp, g_values, scalars[7], adv_stats[3] float64, advn, ret) + (g_probs,) with ``entropy``."""
        if entropy and out.step_probs is None:
            raise ValueError("new_ppo_bufs(entropy=True) needs the episode's step_probs: episode_forward(probs=True)")
        bufs = self._grad_bufs(out, 7) + (th.empty_like(out.step_values), th.empty_like(out.step_values))
        return bufs + (th.empty_like(out.step_probs),) if entropy else bufs

    def _check_ppo_bufs(self, out: EpisodeTensors, bufs: Tuple[th.Tensor, ...], what: str) -> None:
        if (len(bufs) not in (7, 8) or bufs[3].numel() != 7 or bufs[5].shape != out.step_values.shape or
                bufs[6].shape != out.step_values.shape):
            raise ValueError(f"{what}: buffers from new_ppo_bufs(out, entropy) needed")

    def advantages(
        self, out: EpisodeTensors, y: th.Tensor, gamma: float, lam: float, phase: int = 0,
        bufs: Optional[Tuple[th.Tensor, ...]] = None,
    ) -> Tuple[th.Tensor, ...]:
        """marl_advantages: rewards -> GAE(``lam``) -> standardise into ``bufs`` (``new_ppo_bufs``): advn = bufs[5],
        ret = bufs[6], adv_stats = bufs[4].  ``lam`` = 1: the advantage and critic target of ``a2c_loss``, bit for
        bit.  Phases as in ``a2c_loss``."""
        cfg = self.cfg
        assert cfg is not None
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"gae_lambda must lie in [0, 1], got {lam}")
        if phase not in (0, 1, 2):
            raise ValueError(f"phase must be 0, 1 or 2, got {phase}")
        y = _need(y, th.int64, "y")
        if bufs is None:
            bufs = self.new_ppo_bufs(out, out.step_probs is not None)
        self._check_ppo_bufs(out, bufs, "advantages")
        ews = self.episode_ws(True)
        self._loss_call(
            self.lib.marl_advantages,
            C.byref(cfg), ews.data_ptr(), _nbytes(ews), out.step_preds.data_ptr(), out.step_values.data_ptr(),
            y.data_ptr(), C.c_float(gamma), C.c_float(lam), bufs[5].data_ptr(), bufs[6].data_ptr(),
            bufs[4].data_ptr(), phase, _stream(self.device))
        return bufs

    def ppo_loss(
        self, out: EpisodeTensors, y: th.Tensor, old_logp: th.Tensor, advn: th.Tensor, ret: th.Tensor,
        clip_eps: float, bufs: Optional[Tuple[th.Tensor, ...]] = None, entropy_coef: float = 0.0,
    ) -> Tuple[th.Tensor, ...]:
        """marl_ppo_loss_fwd_bwd: the clipped surrogate of ``out`` against ``old_logp`` with the standardised
        advantage ``advn`` and the critic target ``ret`` (all [Ns,Na,Nb]; ``advantages``).  Writes g_preds, g_logp,
        g_values = bufs[0:3], scalars[7] = bufs[3] = {loss, surrogate, error, critic, entropy, approx_kl, clip_frac}
        and, with ``entropy_coef`` > 0 (``out.step_probs`` needed), g_probs = bufs[7]."""
        cfg = self.cfg
        assert cfg is not None
        if not clip_eps > 0.0:
            raise ValueError(f"ppo_clip must be > 0, got {clip_eps}")
        if not entropy_coef >= 0.0:
            raise ValueError(f"entropy_coef must be >= 0, got {entropy_coef}")
        y = _need(y, th.int64, "y")
        ent = entropy_coef > 0.0
        if ent and out.step_probs is None:
            raise ValueError("ppo_loss(entropy_coef > 0) needs the episode's step_probs: episode_forward(probs=True)")
        want = tuple(out.step_log_probas.shape)
        ins = []
        for t, name in ((old_logp, "old_logp"), (advn, "advn"), (ret, "ret")):
            if not isinstance(t, th.Tensor) or tuple(t.shape) != want:
                raise ValueError(f"ppo_loss: {name} must be a tensor of shape {want}, got "
                                 f"{tuple(getattr(t, 'shape', ()))}")
            ins.append(_need(t, th.float32, name))
        if bufs is None:
            bufs = self.new_ppo_bufs(out, ent)
        self._check_ppo_bufs(out, bufs, "ppo_loss")
        if ent and (len(bufs) != 8 or bufs[7].shape != out.step_probs.shape):
            raise ValueError("ppo_loss(entropy_coef > 0): buffers from new_ppo_bufs(out, True) needed")
        probs = _need(out.step_probs, th.float32, "step_probs") if ent else None
        ews = self.episode_ws(True)
        self._loss_call(
            self.lib.marl_ppo_loss_fwd_bwd,
            C.byref(cfg), ews.data_ptr(), _nbytes(ews), out.step_preds.data_ptr(),
            out.step_log_probas.data_ptr(), out.step_values.data_ptr(), y.data_ptr(), ins[0].data_ptr(),
            ins[1].data_ptr(), ins[2].data_ptr(), C.c_float(clip_eps), _ptr(probs), C.c_float(entropy_coef),
            bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[7].data_ptr() if ent else None,
            bufs[3].data_ptr(), _stream(self.device))
        return bufs

    def grad_clip(self, grads: th.Tensor, max_norm: float, grad_scale: float = 1.0) -> th.Tensor:
        """marl_grad_clip: ``grads`` (flat fp32) *= min(1, max_norm / (norm + 1e-6)) in place; returns the device
        scalar holding the norm before clipping (overwritten by the next call - clone to keep).  ``grad_scale``
        (1 / world_size after an all-reduce sum) is applied first and stays in the buffer: Adam then takes 1."""
        if not max_norm > 0.0:
            raise ValueError(f"max_grad_norm must be > 0, got {max_norm}")
        if not grad_scale > 0.0:
            raise ValueError(f"grad_scale must be > 0, got {grad_scale}")
        if not grads.is_cuda or grads.dtype != th.float32 or not grads.is_contiguous():
            raise RuntimeError("grad_clip: the gradient buffer must be a contiguous fp32 GPU tensor")
        if self._clip_scratch is None:
            self._clip_scratch = th.zeros(_lib.MARL_GRAD_CLIP_SCRATCH_BYTES // 8 + 1, dtype=th.float64,
                                          device=self.device)
        sc = self._clip_scratch
        check(self.lib.marl_grad_clip(grads.data_ptr(), grads.numel(), C.c_float(max_norm), C.c_float(grad_scale),
                                      sc[-1:].data_ptr(),
                                      sc.data_ptr(), _lib.MARL_GRAD_CLIP_SCRATCH_BYTES, _stream(self.device)))
        return sc[-1:].view(th.float32)[0]

    def adam(
        self, params: th.Tensor, grads: th.Tensor, exp_avg: th.Tensor, exp_avg_sq: th.Tensor,
        step: int, lr: float, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
        grad_scale: float = 1.0, counters: Optional[th.Tensor] = None,
    ) -> None:
        for t in (params, grads, exp_avg, exp_avg_sq):
            if not t.is_cuda or t.dtype != th.float32 or not t.is_contiguous():
                raise RuntimeError("adam buffers must be contiguous fp32 GPU tensors")
        check(self.lib.marl_adam_step(
            params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
            params.numel(), step, lr, betas[0], betas[1], eps, grad_scale, _ptr(counters),
            _stream(self.device)))

    def optim_step(
        self, params: th.Tensor, grads: th.Tensor, exp_avg: th.Tensor, exp_avg_sq: th.Tensor, table, opts,
        step: int = 0, ema: Optional[th.Tensor] = None, grad_scale: float = 1.0,
        counters: Optional[th.Tensor] = None, scalars_out: Optional[th.Tensor] = None,
    ) -> None:
        """marl_optim_step: one AdamW step over the flat buffers under ``opts`` (an ``optim.OptimOptions`` whose
        schedule has its ``base_lr``) and ``table`` (``optim.segments``; or a ready ``optim.Segment`` array with its
        length: ``(array, n)``).  ``step``: the 1-based step, or ``counters``: the block whose step field the kernel
        reads.  ``ema``: the averaged weights, updated in the same launch.  ``scalars_out`` (fp32 [4], device):
        receives {lr_t, 1 - beta1^t, 1 - beta2^t, t}."""
        from . import optim as _optim

        for t in (params, grads, exp_avg, exp_avg_sq) + (() if ema is None else (ema,)):
            if not t.is_cuda or t.dtype != th.float32 or not t.is_contiguous() or t.numel() != params.numel():
                raise RuntimeError("optim_step buffers must be contiguous fp32 GPU tensors of one length")
        if scalars_out is not None and (not scalars_out.is_cuda or scalars_out.dtype != th.float32 or
                                        scalars_out.numel() < 4 or not scalars_out.is_contiguous()):
            raise RuntimeError("optim_step: scalars_out must be a contiguous fp32 GPU tensor of 4 elements")
        if isinstance(table, tuple) and len(table) == 2 and not isinstance(table[0], tuple):
            arr, nseg = table
        else:
            arr, nseg = _optim.segment_array(table), len(table)
        desc = opts.schedule.desc()
        check(self.lib.marl_optim_step(
            params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), _ptr(ema),
            params.numel(), grad_scale, C.cast(arr, C.c_void_p), nseg, opts.betas[0], opts.betas[1], opts.eps,
            C.cast(C.pointer(desc), C.c_void_p), step, _ptr(counters),
            0.0 if opts.ema_decay is None else opts.ema_decay, _ptr(scalars_out), _stream(self.device)))

    def step_forward(
        self, obs: th.Tensor, msg: th.Tensor, norm_pos: th.Tensor, h: th.Tensor, c: th.Tensor,
        hc: th.Tensor, cc: th.Tensor, noise: Optional[th.Tensor] = None,
        rng: Optional[Tuple[int, int]] = None, ws: Optional[th.Tensor] = None,
    ) -> Tuple[th.Tensor, ...]:
        """marl_step_forward: (probs, values, preds, new_msg, h, c, hc, cc) in [Na,Nb,..];
        with ``noise`` ([Na,Nb,nA] ~ Exp(1), parity mode) or ``rng=(seed, offset)`` (in-kernel
        draws) also (actions int64, log-probs).  ``ws`` = a training workspace of the current
        one-step configuration (``train_ws_acquire``): marl_step_forward_train, same outputs, the
        activations stay in ``ws`` for ``step_backward``."""
        cfg = self.cfg
        assert cfg is not None
        na, nb = cfg.nb_agents, cfg.batch
        dev = self.device
        ins = [_need(t, th.float32, n) for t, n in (
            (obs, "obs"), (msg, "msg"), (norm_pos, "norm_pos"), (h, "h"), (c, "c"), (hc, "hc"),
            (cc, "cc"))]
        outs = (
            th.empty(na, nb, cfg.nb_action, device=dev), th.empty(na, nb, device=dev),
            th.empty(na, nb, cfg.nb_class, device=dev), th.empty(na, nb, cfg.n_m, device=dev),
            th.empty(na, nb, cfg.n_b, device=dev), th.empty(na, nb, cfg.n_b, device=dev),
            th.empty(na, nb, cfg.n_a, device=dev), th.empty(na, nb, cfg.n_a, device=dev),
        )
        extra: Tuple[th.Tensor, ...] = ()
        nz = act = lp = None
        if noise is not None or rng is not None:
            nz = None if noise is None else _need(noise, th.float32, "noise")
            act = th.empty(na, nb, dtype=th.int64, device=dev)
            lp = th.empty(na, nb, device=dev)
            extra = (act, lp)
        seed, offset = rng if rng is not None else (0, 0)
        wws = self.packed_weights_ws()
        if ws is not None:
            if cfg.nb_steps != 1:
                raise RuntimeError("step_forward(ws=...): configure the engine with nb_steps = 1")
            self._check_ws(ws, "step_forward")
            fn, ews = self.lib.marl_step_forward_train, ws
        else:
            fn, ews = self.lib.marl_step_forward, self.episode_ws(False)
        self._agg(
            fn, C.byref(cfg), wws.data_ptr(), _nbytes(wws), ews.data_ptr(), _nbytes(ews),
            *[t.data_ptr() for t in ins], *[t.data_ptr() for t in outs], _ptr(nz), seed & _U64,
            offset & _U64, _ptr(act), _ptr(lp), _stream(dev))
        return outs + extra

    def _check_ws(self, ws: th.Tensor, what: str) -> None:
        if getattr(ws, "_marl_key", None) != (self._cfg_key, _tune_epoch):
            raise RuntimeError(
                f"{what}: the engine was re-configured (other batch size / image shape / layout knob) since "
                "this workspace was acquired - it no longer fits")

    def step_backward(
        self, ws: th.Tensor, obs: th.Tensor, grads: Dict[str, th.Tensor],
        g_probs: Optional[th.Tensor] = None, g_logp: Optional[th.Tensor] = None,
        g_values: Optional[th.Tensor] = None, g_preds: Optional[th.Tensor] = None,
        g_msg: Optional[th.Tensor] = None, g_h: Optional[th.Tensor] = None,
        g_c: Optional[th.Tensor] = None, g_hc: Optional[th.Tensor] = None,
        g_cc: Optional[th.Tensor] = None, want: Sequence[bool] = (True,) * 5,
        d_comm: Optional[th.Tensor] = None,
    ) -> Tuple[Optional[th.Tensor], ...]:
        """marl_step_backward of the step whose activations ``ws`` holds (``step_forward(ws=ws)``).
        Upstream gradients may be None (zero); ``g_logp`` only if that forward sampled.  Writes the
        parameter gradients into ``grads`` (overwritten) and returns the input gradients
        (d_msg, d_h, d_c, d_hc, d_cc) in [Na,Nb,..], None where ``want`` is False.  ``d_comm`` ([Na,Na] fp32,
        overwritten): also this step's gradient w.r.t. the mixing matrix (marl_comm_grad on the step workspace)."""
        cfg = self.cfg
        assert cfg is not None
        self._check_ws(ws, "step_backward")
        if d_comm is not None and self.comm is None:
            raise ValueError("step_backward(d_comm=...): the engine has no communication matrix")
        na, nb, dev = cfg.nb_agents, cfg.batch, self.device
        obs = _need(obs, th.float32, "obs")
        ups = [None if t is None else _need(t, th.float32, n) for t, n in (
            (g_probs, "g_probs"), (g_logp, "g_logp"), (g_values, "g_values"), (g_preds, "g_preds"),
            (g_msg, "g_msg"), (g_h, "g_h"), (g_c, "g_c"), (g_hc, "g_hc"), (g_cc, "g_cc"))]
        widths = (cfg.n_m, cfg.n_b, cfg.n_b, cfg.n_a, cfg.n_a)
        outs = tuple(th.empty(na, nb, n, device=dev) if w else None for n, w in zip(widths, want))
        wws = self.packed_weights_ws()
        self._agg(
            self.lib.marl_step_backward,
            C.byref(cfg), wws.data_ptr(), _nbytes(wws), ws.data_ptr(), _nbytes(ws), obs.data_ptr(),
            *[_ptr(t) for t in ups], self._table(grads), *[_ptr(t) for t in outs], _stream(dev))
        if d_comm is not None:
            self.comm_grad(ws, 1, d_comm)
        return outs

    def draw_episode(self, seed: int, offset: int, with_noise: bool = False,
                     into: Optional[Tuple[th.Tensor, ...]] = None,
                     counters: Optional[th.Tensor] = None):
        """marl_draw_episode: the reference's reset draws (positions, h, c, h^, c^; optionally the
        per-step Exp(1) noise) from the library's counter-based generator in ONE launch.
        Returns (pos0, h0, c0, hc0, cc0, noise-or-None); ``into`` = persistent tensors to fill."""
        cfg = self.cfg
        assert cfg is not None
        na, nb, ns, dev = cfg.nb_agents, cfg.batch, cfg.nb_steps, self.device
        if into is None:
            into = (
                th.empty(na, nb, 2, dtype=th.int64, device=dev),
                th.empty(na, nb, cfg.n_b, device=dev), th.empty(na, nb, cfg.n_b, device=dev),
                th.empty(na, nb, cfg.n_a, device=dev), th.empty(na, nb, cfg.n_a, device=dev),
                th.empty(ns, na, nb, cfg.nb_action, device=dev) if with_noise else None,
            )
        pos0, h0, c0, hc0, cc0, noise = into
        check(self.lib.marl_draw_episode(
            C.byref(cfg), seed & _U64, offset & _U64, _ptr(counters), pos0.data_ptr(),
            h0.data_ptr(), c0.data_ptr(), hc0.data_ptr(), cc0.data_ptr(), _ptr(noise), _stream(dev)))
        return into

    # -- device-side iteration counters + hipGraph capture (marl_counters_*, marl_graph_*) ------
    def new_counters(self) -> th.Tensor:
        return th.zeros(_lib.MARL_COUNTERS_BYTES // 8, dtype=th.int64, device=self.device)

    def counters_set(self, counters: th.Tensor, rng_offset: int, step: int, lr: float,
                     betas: Tuple[float, float] = (0.9, 0.999)) -> None:
        check(self.lib.marl_counters_set(counters.data_ptr(), rng_offset & _U64, step, lr, betas[0],
                                         betas[1], _stream(self.device)))

    def counters_tick(self, counters: th.Tensor, lr: float,
                      betas: Tuple[float, float] = (0.9, 0.999)) -> None:
        check(self.lib.marl_counters_tick(counters.data_ptr(), lr, betas[0], betas[1],
                                          _stream(self.device)))

    def graph_begin(self) -> None:
        check(self.lib.marl_graph_begin(_stream(self.device)))

    def graph_end(self) -> int:
        handle = C.c_void_p(0)
        check(self.lib.marl_graph_end(_stream(self.device), C.byref(handle)))
        return handle.value

    def graph_launch(self, handle: int) -> None:
        check(self.lib.marl_graph_launch(handle, _stream(self.device)))

    def debug_buffer(self, name: str, t: int, train: bool = True) -> th.Tensor:
        """View [R, ld] of a named per-step activation inside the episode workspace (tests)."""
        off, ld = C.c_int64(0), C.c_int(0)
        check(self.lib.marl_debug_buffer(C.byref(self.cfg), int(train), name.encode(), t,
                                         C.byref(off), C.byref(ld)))
        rows = self.cfg.nb_agents * self.cfg.batch
        ws = self.episode_ws(train)
        return ws[off.value: off.value + rows * ld.value].view(rows, ld.value)

    # -- standalone environment kernels ------------------------------------------------
    def patch_gather(self, img: th.Tensor, pos: th.Tensor, f: int) -> th.Tensor:
        return patch_gather(img, pos, f)

    def transition(self, pos: th.Tensor, actions: th.Tensor, table: Sequence[Sequence[int]],
                   sizes: Sequence[int], f: int) -> th.Tensor:
        return transition(pos, actions, table, sizes, f)


# Environment kernels need no model: module-level wrappers (core/environment.py uses them)
def patch_gather(img: th.Tensor, pos: th.Tensor, f: int) -> th.Tensor:
    """marl_patch_gather: obs[a,b] = img[b, :, p0:p0+f, p1:p1+f] (environment.py:95-126)."""
    lib = _lib.load()
    img = _need(img, th.float32, "img")
    pos = _need(pos, th.int64, "pos")
    na, nb, _ = pos.shape
    _, c, h, w = img.shape
    obs = th.empty(na, nb, c, f, f, device=img.device)
    check(lib.marl_patch_gather(img.data_ptr(), pos.data_ptr(), obs.data_ptr(), na, nb, c, h, w, f,
                                _stream(img.device)))
    return obs


def transition(pos: th.Tensor, actions: th.Tensor, table: Sequence[Sequence[int]],
               sizes: Sequence[int], f: int) -> th.Tensor:
    """marl_transition: bounded move (environment.py:56-66,128-150)."""
    lib = _lib.load()
    pos = _need(pos, th.int64, "pos")
    actions = _need(actions, th.int64, "actions")
    out = th.empty_like(pos)
    flat = (C.c_int32 * (2 * len(table)))(*[v for mv in table for v in mv])
    rows = pos.shape[0] * pos.shape[1]
    check(lib.marl_transition(pos.data_ptr(), actions.data_ptr(), out.data_ptr(), flat, len(table),
                              rows, sizes[0], sizes[1], f, _stream(pos.device)))
    return out


def normalize_positions(pos: th.Tensor, sizes: Sequence[int]) -> th.Tensor:
    """marl_normalize_positions: pos / size per dimension (environment.py:74-81)."""
    lib = _lib.load()
    pos = _need(pos, th.int64, "pos")
    out = th.empty(pos.shape, dtype=th.float32, device=pos.device)
    rows = pos.shape[0] * pos.shape[1]
    check(lib.marl_normalize_positions(pos.data_ptr(), out.data_ptr(), rows, sizes[0], sizes[1],
                                       _stream(pos.device)))
    return out
