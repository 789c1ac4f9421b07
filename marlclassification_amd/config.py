"""Run configuration objects and the ``marl.json`` wire format of the reference
(config.py:11-131): same field names, same JSON keys, so a ``marl.json`` written by either
side loads on the other.  ``build_marl`` is the constructor path for the hot-path objects."""

import json
from os.path import exists, isfile
from typing import List, Optional, Tuple, Union

from pydantic import BaseModel

from .core import Environment, MultiAgent
from .networks import ModelsWrapper
from .networks.vision import CNN_BY_NAME

_MODEL_KEYS = (
    "ft_extr_str", "window_size", "hidden_size_belief", "hidden_size_action", "hidden_size_msg",
    "hidden_size_msg_output", "hidden_size_state", "state_dim", "actions", "nb_class",
    "hidden_size_linear_belief", "hidden_size_linear_action",
)


class MainConfig(BaseModel):
    step: int
    run_id: str
    cuda: bool
    nb_agent: int


class ModelConfig(BaseModel):
    ft_extr_str: str
    window_size: int
    hidden_size_belief: int
    hidden_size_action: int
    hidden_size_msg: int
    hidden_size_msg_output: int
    hidden_size_state: int
    state_dim: int
    actions: List[List[int]]
    nb_class: int
    hidden_size_linear_belief: int
    hidden_size_linear_action: int
    # communication graph in the command-line spelling (comm.parse: full | none | ring[:k] | star[:hub] | grid:RxC |
    # teams:a,b,... | FILE.npy); None: the reference's mean over the other agents - and the reference's marl.json
    comm: Optional[str] = None
    # range-limited communication in the command-line spelling (comm.parse_range: R[:chebyshev|euclidean][:raw]);
    # None: off - and the key is not written
    comm_range: Optional[str] = None
    # per-image input normalisation in the command-line spelling (transforms.parse: normal | channel-normal | minmax |
    # channel-minmax | user-normal:m..:s.. | user-minmax:lo..:hi..); part of the model like comm - train, test and infer
    # must see the same pixels.  None: off - and the key is not written
    normalize: Optional[str] = None

    def save_marl_config(self, out_json_path: str) -> None:
        raw = {k: getattr(self, k) for k in _MODEL_KEYS}
        if self.comm is not None:  # (only when one was given: a default run writes the reference's file)
            raw["comm"] = self.comm
        if self.comm_range is not None:
            raw["comm_range"] = self.comm_range
        if self.normalize is not None:
            raw["normalize"] = self.normalize
        with open(out_json_path, "w", encoding="utf-8") as f:
            json.dump(raw, f)

    @classmethod
    def load_marl_config(cls, json_path: str) -> "ModelConfig":
        assert exists(json_path) and isfile(json_path), f'"{json_path}" does not exist or is not a file'
        with open(json_path, "r", encoding="utf-8") as f:
            raw = json.load(f)
        return cls(**{k: raw[k] for k in _MODEL_KEYS}, comm=raw.get("comm"), comm_range=raw.get("comm_range"),
                   normalize=raw.get("normalize"))

    def build_networks(self) -> ModelsWrapper:
        assert self.ft_extr_str in CNN_BY_NAME, (
            f'Unknown feature extractor "{self.ft_extr_str}", expected one of {sorted(CNN_BY_NAME)}'
        )
        return ModelsWrapper(
            CNN_BY_NAME[self.ft_extr_str](self.window_size),
            self.hidden_size_belief, self.hidden_size_action, self.hidden_size_msg,
            self.hidden_size_msg_output, self.hidden_size_state, self.state_dim,
            len(self.actions), self.nb_class, self.hidden_size_linear_belief,
            self.hidden_size_linear_action,
        )

    def build_environment(self) -> Environment:
        return Environment(self.actions, self.window_size)

    def build_marl(self, nb_agents: int) -> Tuple[ModelsWrapper, MultiAgent, Environment]:
        networks = self.build_networks()
        if self.comm is not None:
            from . import comm as _comm

            networks.set_comm(_comm.parse(self.comm, nb_agents))  # (moves with networks.to(device))
        if self.comm_range is not None:
            from . import comm as _comm

            networks.set_comm_range(*_comm.parse_range(self.comm_range))
        return networks, MultiAgent(nb_agents, networks), self.build_environment()


class TrainConfig(BaseModel):
    img_size: int
    nb_epoch: int
    learning_rate: float
    batch_size: int
    resources_dir: str
    output_dir: str
    gamma: float
    # beta of the entropy bonus: loss - beta * mean_{a,b} sum_t H(pi_t) (0: the reference's plain A2C loss)
    entropy_coef: float = 0.0
    # PPO on the fused path (all four at their defaults: the reference's one A2C step per rollout): update epochs per
    # rollout, the clip range of the probability ratio, lambda of GAE, and the global gradient-norm bound (None: off)
    ppo_epochs: int = 1
    ppo_clip: float = 0.2
    gae_lambda: float = 1.0
    max_grad_norm: Optional[float] = None
    # --learn-comm: the communication graph is a comm.LearnableComm on the support of ModelConfig.comm (None: full)
    # with its own Adam at comm_lr (None: learning_rate)
    learn_comm: bool = False
    comm_lr: Optional[float] = None
    # exploration schedules (explore.py): (start, end) of the sampling temperature and of the eps-soft mixture,
    # interpolated linearly over the epochs and applied at each epoch's start; None: the plain policy
    temperature: Optional[Tuple[float, float]] = None
    explore_eps: Optional[Tuple[float, float]] = None
    # --augment: device-side augmentation of the training split in the command-line spelling (augment.parse); a run-time
    # choice like the exploration controls, not written to marl.json.  None: every batch is the plain gather
    augment: Optional[str] = None
    # --mix: CutMix / Mixup of the training split in the command-line spelling (mix.parse), fused into the same batch
    # gather; the loss then takes the batch's target distributions.  A run-time choice too, not written to marl.json
    mix: Optional[str] = None
    # --color: colour jitter of the training split in the command-line spelling (color.parse), one launch behind the
    # batch gather and before the normalisation.  A run-time choice too, not written to marl.json
    color: Optional[str] = None
    # options of the vote error and the rewards (class_loss.py), run-time choices like the two above: "balanced", a
    # .npy path or one weight per class; the smoothing; all | last[:K] | linear; rewards times the class weight
    class_weights: Optional[Union[str, Tuple[float, ...]]] = None
    label_smoothing: float = 0.0
    error_steps: Optional[str] = None
    weight_rewards: bool = False
    # the flat optimiser step (optim.py), run-time choices too: all at their defaults = the plain Adam step.  lr_groups /
    # lr_schedule in the command-line spelling (optim.parse_groups / parse_schedule); ema = the decay of the averaged
    # weights; eval_ema: eval_epoch runs on them; resume = a models/trainer_epoch_{e}.pt to continue from
    weight_decay: float = 0.0
    decay_all: bool = False
    lr_groups: Optional[str] = None
    lr_schedule: Optional[str] = None
    warmup_steps: int = 0
    adam_betas: Optional[Tuple[float, float]] = None
    ema: Optional[float] = None
    eval_ema: bool = False
    resume: Optional[str] = None
    # --report: the evaluation after every epoch (and the training meter) is an episode report (report.py): per-step
    # accuracy, top-k, NLL, calibration, early exit at the exit_at confidences ("t1,t2,..."); off: the confusion meter
    report: bool = False
    report_topk: int = 5
    report_bins: int = 15
    exit_at: Optional[str] = None

    def optim_on(self) -> bool:
        return (self.weight_decay != 0.0 or self.decay_all or self.lr_groups is not None or
                self.lr_schedule is not None or self.warmup_steps != 0 or self.adam_betas is not None or
                self.ema is not None)


class EvalConfig(BaseModel):
    img_size: int
    state_dict_path: str
    batch_size: int
    json_path: str
    dataset_path: str
    output_dir: str
    comm: Optional[str] = None  # --comm: replaces the graph marl.json names (None: keep it)
    comm_range: Optional[str] = None  # --comm-range: replaces the range marl.json names (None: keep it)
    greedy: bool = False  # --greedy: deterministic acting, the argmax of the policy (a run-time choice, not in marl.json)
    temperature: float = 1.0  # --temperature: the policy is softmax(z / T)
    tta: Optional[str] = None  # --tta: test-time augmentation, the mean over the views of augment.parse(SPEC).views()
    normalize: Optional[str] = None  # --normalize: replaces the transform marl.json names ("none": off; None: keep it)
    # --report: the episode report (report.py) beside the confusion matrix - one table row per step, report.json and
    # accuracy_per_step.png; exit_at = "t1,t2,...", the confidences of the early-exit statistics.  Off: today's path
    report: bool = False
    report_topk: int = 5
    report_bins: int = 15
    exit_at: Optional[str] = None


class InferConfig(BaseModel):
    state_dict_path: str
    json_path: str
    images_path: List[str]
    output_dir: str
    class_to_idx: str
    saliency: bool = False  # also write saliency.png (|d logit / d pixel|) next to the step frames
    normalize: Optional[str] = None  # --normalize: replaces the transform marl.json names ("none": off; None: keep it)
    comm: Optional[str] = None  # --comm: replaces the graph marl.json names (None: keep it)
    comm_range: Optional[str] = None  # --comm-range: replaces the range marl.json names (None: keep it)
    greedy: bool = False  # --greedy: deterministic acting, the argmax of the policy (a run-time choice, not in marl.json)
    temperature: float = 1.0  # --temperature: the policy is softmax(z / T)
