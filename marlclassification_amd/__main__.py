"""``python -m marlclassification_amd`` - the reference's command line (__main__.py:19-417):
``[-a N --step T --cuda --run-id ID] train [options]``, same flags, defaults and action
syntax (``[[1,0],[-1,0],...]``), with the ``train``, ``test`` and ``infer`` modes."""

import argparse
import re
from os.path import abspath, dirname, join

from .augment import parse as parse_augment
from .augment import parse_tta
from .class_loss import check_label_smoothing, parse_class_weights, parse_error_steps
from .comm import check_spelling, parse_range
from .explore import check as check_exploration
from .explore import parse_eps, parse_temperature
from .optim import OptimOptions, parse_betas, parse_groups, parse_schedule
from .config import EvalConfig, InferConfig, MainConfig, ModelConfig, TrainConfig
from .networks.vision import CNN_BY_NAME

_TRAIN_FLAGS = (
    # flags, dest, type, default
    (("--action",), "action", str, "[[1, 0], [-1, 0], [0, 1], [0, -1]]"),
    (("--img-size",), "img_size", int, 28),
    (("--nb-class",), "nb_class", int, 10),
    (("-d", "--dim"), "dim", int, 2),
    (("--f",), "f", int, 7),
    (("--nb",), "n_b", int, 64),
    (("--na",), "n_a", int, 16),
    (("--nm",), "n_m", int, 16),
    (("--nmo",), "n_m_o", int, 24),
    (("--nd",), "n_d", int, 4),
    (("--nlb",), "n_l_b", int, 128),
    (("--nla",), "n_l_a", int, 128),
    (("--batch-size",), "batch_size", int, 8),
    (("--lr", "--learning-rate"), "learning_rate", float, 1e-3),
    (("--gamma",), "gamma", float, 0.99),
    (("--nb-epoch",), "nb_epoch", int, 10),
)


def parse_actions(text: str, dim: int):
    compact = text.replace(" ", "")
    if not re.match(r"^\[(\[(-?\d+,?)+\],)*\[(-?\d+,?)+\]\]$", compact):
        raise ValueError(f"Wrong action(s) : {text}")
    actions = [[int(v) for v in a.split(",")] for a in re.findall(r"\[((?:-?\d+,?)+)\]", compact)]
    for i, a in enumerate(actions):
        assert len(a) == dim, f"Wrong space for action at index {i}"
    return actions


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser("python -m marlclassification_amd")
    p.add_argument("--run-id", type=str, required=True, dest="run_id")
    p.add_argument("-a", "--agents", type=int, default=3, dest="agents")
    p.add_argument("--step", type=int, default=7)
    p.add_argument("--cuda", action="store_true", dest="cuda")
    sub = p.add_subparsers(dest="main_choice", required=True)
    t = sub.add_parser("train")
    for flags, dest, typ, default in _TRAIN_FLAGS:
        t.add_argument(*flags, type=typ, default=default, dest=dest)
    t.add_argument("--ft-extr", type=str, choices=sorted(CNN_BY_NAME), default="mnist", dest="ft_extr_str")
    t.add_argument("--res-folder", type=str, dest="res_folder",
                   default=abspath(join(dirname(abspath(__file__)), "..", "resources")))
    t.add_argument("-o", "--output-dir", type=str, required=True, dest="output_dir")
    e = sub.add_parser("test")  # reference __main__.py:217-258
    e.add_argument("--batch-size", type=int, default=8, dest="batch_size")
    e.add_argument("--dataset-path", type=str, required=True, dest="dataset_path")
    e.add_argument("--img-size", type=int, default=28, dest="img_size")
    e.add_argument("--json-path", type=str, required=True, dest="json_path")
    e.add_argument("--state-dict-path", type=str, required=True, dest="state_dict_path")
    e.add_argument("-o", "--output-dir", type=str, required=True, dest="output_dir")
    i = sub.add_parser("infer")  # reference __main__.py:263-300
    i.add_argument("--images", type=str, nargs="+", required=True, dest="infer_images")
    i.add_argument("--json-path", type=str, required=True, dest="json_path")
    i.add_argument("--state-dict-path", type=str, required=True, dest="state_dict_path")
    i.add_argument("--class2idx", type=str, required=True, dest="class_to_idx")
    i.add_argument("-o", "--output-image-dir", type=str, required=True, dest="output_image_dir")
    i.add_argument("--saliency", action="store_true", dest="saliency",
                   help="also write saliency.png (|d logit / d pixel| of the predicted class) per image")
    t.add_argument("--exact-standardize", action="store_true", dest="exact_standardize",
                   help="multi-GPU: global advantage statistics (update == single-GPU big batch)")
    t.add_argument("--entropy-coef", type=float, default=0.0, dest="entropy_coef",
                   help="entropy bonus: loss - X * mean_{agents,batch} sum_t H(policy_t) (0: the reference's loss)")
    t.add_argument("--ppo-epochs", type=int, default=1, dest="ppo_epochs",
                   help="policy updates per rollout: epochs after the first replay the stored trajectory under the "
                        "new weights on the clipped surrogate (1 with the other PPO flags at their defaults: plain A2C)")
    t.add_argument("--ppo-clip", type=float, default=0.2, dest="ppo_clip",
                   help="clip range of the probability ratio: clamp(ratio, 1 - X, 1 + X)")
    t.add_argument("--gae-lambda", type=float, default=1.0, dest="gae_lambda",
                   help="lambda of the generalised advantage estimate (1: the reference's full returns - values)")
    t.add_argument("--max-grad-norm", type=float, default=None, dest="max_grad_norm",
                   help="clip the global gradient norm to X before every Adam step (default: no clipping)")
    t.add_argument("--learn-comm", action="store_true", dest="learn_comm",
                   help="learn the communication graph: row-softmax weights over the support of --comm (default "
                        "support: full), updated by their own Adam; every checkpoint epoch also writes "
                        "models/comm_epoch_{e}.npy, which test / infer load with --comm FILE.npy")
    t.add_argument("--comm-lr", type=float, default=None, dest="comm_lr", metavar="LR",
                   help="learning rate of the graph's logits with --learn-comm (default: --lr)")
    t.add_argument("--temperature", type=_arg(parse_temperature), default=None, dest="temperature",
                   metavar="T[:T_end]",
                   help="sampling temperature: actions are drawn from softmax(z / T); T:T_end is interpolated "
                        "linearly over the epochs and applied at each epoch's start (default: 1)")
    t.add_argument("--explore-eps", type=_arg(parse_eps), default=None, dest="explore_eps", metavar="E[:E_end]",
                   help="eps-soft behaviour policy (1 - E) softmax(z / T) + E / nb_action, E in [0, 0.5], with the "
                        "same per-epoch schedule spelling (default: 0)")
    t.add_argument("--augment", type=_arg(_augment_arg), default=None, dest="augment", metavar="SPEC",
                   help="device-side augmentation of the training split, fused into the batch gather: a comma-separated "
                        "list of hflip, vflip, rot90, d4, shift:T[:reflect|zero], erase:S[:p] (rot90 / d4 need square "
                        "images) and, resampled bilinearly in the same launch, rotate:DEG (any angle in [-DEG, DEG]), "
                        "scale:LO:HI (zoom, log-uniform) and stretch:R (aspect in [1/R, R]); default: none")
    t.add_argument("--mix", type=_arg(_mix_arg), default=None, dest="mix", metavar="SPEC",
                   help="CutMix / Mixup of the training split, fused into the batch gather: a comma-separated list of "
                        "cutmix[:alpha[:p]] and mixup[:alpha[:p]] (lam ~ Beta(alpha, alpha), per-image probability p; "
                        "defaults 1 and 0.5, the probabilities sum to at most 1); the loss takes the mixed target "
                        "distributions (default: none)")
    t.add_argument("--color", type=_arg(_color_arg), default=None, dest="color", metavar="SPEC",
                   help="colour jitter of the training split, one per-image colour matrix applied in one launch behind "
                        "the batch gather: a comma-separated list of brightness:B, contrast:C, saturation:S (factor "
                        "uniform in [max(0, 1 - v), 1 + v], 0 < v <= 3), hue:H (angle uniform in [-H, H] turns, "
                        "0 < H <= 0.5) and gray:p (a grey image with probability p); default: none")
    t.add_argument("--class-weights", type=_arg(parse_class_weights), default=None, dest="class_weights",
                   metavar="balanced|FILE.npy|w0,w1,...",
                   help="class weights of the vote error: balanced = N / (nb_class * n_c) from the whole training "
                        "split, a .npy vector, or one weight per class (default: all 1)")
    t.add_argument("--label-smoothing", type=_arg(_label_smoothing), default=0.0, dest="label_smoothing", metavar="E",
                   help="label smoothing of the vote error, E in [0, 1): the target is (1 - E) onehot + E / nb_class "
                        "(default: 0)")
    t.add_argument("--error-steps", type=_arg(parse_error_steps), default=None, dest="error_steps",
                   metavar="all|last[:K]|linear",
                   help="which steps' votes the error term asks to be right: all, the last K (last = last:1), or "
                        "weights ramping linearly to 1 at the last step (default: all)")
    t.add_argument("--weight-rewards", action="store_true", dest="weight_rewards",
                   help="cost-sensitive rewards: every agent's reward is multiplied by its image's class weight")
    t.add_argument("--weight-decay", type=_arg(_weight_decay), default=0.0, dest="weight_decay", metavar="W",
                   help="decoupled (AdamW) weight decay of the matrices: conv and linear weights; biases and "
                        "LayerNorm / GroupNorm gains do not decay (default: 0)")
    t.add_argument("--decay-all", action="store_true", dest="decay_all",
                   help="--weight-decay reaches every tensor, biases and norm gains included")
    t.add_argument("--lr-groups", type=_arg(_lr_groups), default=None, dest="lr_groups",
                   metavar="NAME=MULT[:WD],...",
                   help="learning-rate multiplier (0 freezes) and optionally a weight decay per module: map_obs (= "
                        "cnn), map_pos, encode_msg, decode_msg, belief_unit, action_unit, policy, critic, predict; "
                        "e.g. cnn=0.1,policy=0,critic=1:0.01")
    t.add_argument("--lr-schedule", type=_arg(_lr_schedule), default=None, dest="lr_schedule",
                   metavar="constant|linear|cosine[:FINAL_RATIO]",
                   help="learning rate after the warm-up: constant, or a linear / cosine decay to FINAL_RATIO * "
                        "--learning-rate (default 0) at the run's last optimiser step = nb_epoch * iterations per "
                        "epoch * ppo_epochs (default: constant)")
    t.add_argument("--warmup-steps", type=int, default=0, dest="warmup_steps", metavar="N",
                   help="linear warm-up of the learning rate over the first N optimiser steps (default: 0)")
    t.add_argument("--adam-betas", type=_arg(parse_betas), default=None, dest="adam_betas", metavar="B1,B2",
                   help="Adam's betas (default: 0.9,0.999)")
    t.add_argument("--ema", type=_arg(_ema), default=None, dest="ema", metavar="D",
                   help="keep an exponential moving average of the weights with decay D in (0, 1); every checkpoint "
                        "epoch also writes models/nn_models_ema_epoch_{e}.pt, loadable by test / infer")
    t.add_argument("--eval-ema", action="store_true", dest="eval_ema",
                   help="with --ema: the evaluation after every epoch runs on the averaged weights")
    t.add_argument("--resume", type=str, default=None, dest="resume", metavar="FILE",
                   help="continue an interrupted run bit for bit from models/trainer_epoch_{e}.pt (written every "
                        "checkpoint epoch next to nn_models_epoch_{e}.pt, which is loaded with it): Adam moments, "
                        "averaged weights, optimiser step, generator position; same flags as the interrupted run")
    t.add_argument("--normalize", type=_arg(_normalize_arg), default=None, dest="normalize", metavar="SPEC",
                   help="per-image input normalisation on the device, part of the model (written to marl.json; test "
                        "and infer read it): normal | channel-normal | minmax | channel-minmax | "
                        "user-normal:m0,m1,..:s0,s1,.. | user-minmax:lo0,..:hi0,.. | dataset (the mean / std of the "
                        "training split, stored as user-normal:...); default: off")
    for sp in (e, i):
        sp.add_argument("--normalize", type=_arg(_normalize_override), default=None, dest="normalize",
                        metavar="SPEC|none",
                        help="replaces the input normalisation marl.json names (none: off; default: keep it)")
    e.add_argument("--tta", type=_arg(_tta_arg), default=None, dest="tta", metavar="SPEC",
                   help="test-time augmentation: every batch runs once per flip / rotation the spec allows (hflip, "
                        "vflip, rot90, d4), with zoom:Z1/Z2/... once per flip / rotation and zoom factor (multi-scale "
                        "views, resampled bilinearly), and the predictions are averaged (default: one run)")
    for sp in (t, e):
        sp.add_argument("--report", action="store_true", dest="report",
                        help="episode report on the device: vote accuracy, top-k, NLL and agreement per step, every "
                             "agent's accuracy, calibration (ECE) and early-exit statistics; writes report*.json and "
                             "accuracy_per_step*.png beside the confusion matrix (default: the confusion matrix only)")
        sp.add_argument("--report-topk", type=int, default=5, dest="report_topk", metavar="K",
                        help="with --report: ranks reported, 1 .. 16 (default: 5)")
        sp.add_argument("--report-bins", type=int, default=15, dest="report_bins", metavar="B",
                        help="with --report: confidence bins of the calibration, 1 .. 64 (default: 15)")
        sp.add_argument("--exit-at", type=_arg(_exit_at), default=None, dest="exit_at", metavar="t1,t2,...",
                        help="with --report: up to 8 confidences in [0, 1]; reports the steps an episode needs and its "
                             "accuracy when it stops at the first step whose vote is that confident")
    for sp in (e, i):
        sp.add_argument("--greedy", action="store_true", dest="greedy",
                        help="deterministic acting: every agent takes the argmax of its policy (no random draw)")
        sp.add_argument("--temperature", type=_arg(_temperature), default=1.0, dest="temperature", metavar="T",
                        help="the policy is softmax(z / T) (default: 1)")
    for sp in (t, e, i):
        sp.add_argument("--comm", type=_comm_arg, default=None, dest="comm", metavar="GRAPH",
                        help="communication graph of the message exchange: full | none | ring[:k] | star[:hub] | "
                             "grid:RxC | teams:a,b,... | FILE.npy ([Na,Na], row = receiver); default: the mean over "
                             "the other agents (test / infer: what marl.json names)")
        sp.add_argument("--comm-range", type=_comm_range_arg, default=None, dest="comm_range",
                        metavar="R[:METRIC][:raw]",
                        help="range-limited communication: an agent hears the agents within R pixels of it, per "
                             "image and step (METRIC chebyshev - the default - or euclidean; --comm, default full, is "
                             "the base whose out-of-range links are cut; a receiver's remaining weights are rescaled "
                             "to the base row's sum unless :raw); default: off (test / infer: what marl.json names)")
    return p


def _arg(parse):
    """argparse type from a parser that raises ValueError."""
    def convert(text: str):
        try:
            return parse(text)
        except ValueError as err:
            raise argparse.ArgumentTypeError(str(err))
    return convert


def _augment_arg(text: str) -> str:
    return parse_augment(text).spec


def _normalize_arg(text: str) -> str:
    from .transforms import parse as parse_normalize

    return parse_normalize(text).spelling  # ("dataset" stays: train resolves it against the training split)


def _normalize_override(text: str) -> str:
    from .transforms import resolve

    spec = resolve(text)  # ("dataset" has nothing to be resolved against here: refused)
    return "none" if spec is None else spec.spelling


def _color_arg(text: str) -> str:
    from .color import parse as parse_color

    return parse_color(text).spec


def _mix_arg(text: str) -> str:
    from .mix import parse as parse_mix

    return parse_mix(text).spec


def _exit_at(text: str) -> str:
    from .report import ReportOptions, parse_exit_at

    ReportOptions(exit_thresholds=parse_exit_at(text))
    return text


def _tta_arg(text: str) -> str:
    return parse_tta(text).spec


def _label_smoothing(text: str) -> float:
    return check_label_smoothing(float(text))


def _weight_decay(text: str) -> float:
    OptimOptions(weight_decay=float(text))
    return float(text)


def _ema(text: str) -> float:
    OptimOptions(ema_decay=float(text))
    return float(text)


def _lr_groups(text: str) -> str:
    OptimOptions(groups=parse_groups(text))
    return text


def _lr_schedule(text: str) -> str:
    parse_schedule(text)
    return text


def _temperature(text: str) -> float:
    return check_exploration(temperature=float(text)).temperature


def _comm_arg(text: str) -> str:
    try:
        return check_spelling(text)
    except ValueError as err:
        raise argparse.ArgumentTypeError(str(err))


def _comm_range_arg(text: str) -> str:
    try:
        return parse_range(text).spelling()
    except ValueError as err:
        raise argparse.ArgumentTypeError(str(err))


def check_report(parser: argparse.ArgumentParser, args) -> None:
    """--report-topk / --report-bins / --exit-at need --report and values the kernel serves."""
    if args.main_choice not in ("train", "test"):
        return
    if not args.report:
        if args.report_topk != 5 or args.report_bins != 15 or args.exit_at is not None:
            parser.error("--report-topk / --report-bins / --exit-at need --report")
        return
    from .report import ReportOptions, parse_exit_at

    try:
        ReportOptions(args.report_topk, args.report_bins, parse_exit_at(args.exit_at))
    except ValueError as err:
        parser.error(str(err))


def check_learn_comm(parser: argparse.ArgumentParser, args) -> None:
    """--learn-comm needs a graph with at least one link (its support is fixed); --comm-lr needs --learn-comm."""
    if args.main_choice != "train":
        return
    if args.comm_lr is not None and not args.learn_comm:
        parser.error("--comm-lr needs --learn-comm")
    if args.comm_lr is not None and not args.comm_lr > 0.0:
        parser.error("--comm-lr must be > 0")
    if args.learn_comm and args.comm == "none":
        parser.error("--learn-comm needs a graph with links to learn on: --comm none has no support")
    if args.learn_comm and args.comm_range is not None:
        parser.error("--learn-comm with --comm-range: the gradient of a gated base matrix is not computed")


def main(argv=None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    check_learn_comm(parser, args)
    check_report(parser, args)
    main_config = MainConfig(step=args.step, run_id=args.run_id, cuda=args.cuda, nb_agent=args.agents)
    if args.main_choice == "train":
        from .train import train_main

        if args.learn_comm and args.comm is None:
            args.comm = "full"  # (the default support)
        model_config = ModelConfig(
            ft_extr_str=args.ft_extr_str, window_size=args.f, hidden_size_belief=args.n_b,
            hidden_size_action=args.n_a, hidden_size_msg=args.n_m,
            hidden_size_msg_output=args.n_m_o, hidden_size_state=args.n_d, state_dim=args.dim,
            actions=parse_actions(args.action, args.dim), nb_class=args.nb_class,
            hidden_size_linear_belief=args.n_l_b, hidden_size_linear_action=args.n_l_a,
            comm=args.comm, comm_range=args.comm_range, normalize=args.normalize,
        )
        train_config = TrainConfig(
            img_size=args.img_size, nb_epoch=args.nb_epoch, learning_rate=args.learning_rate,
            batch_size=args.batch_size, resources_dir=args.res_folder, output_dir=args.output_dir,
            gamma=args.gamma, entropy_coef=args.entropy_coef, ppo_epochs=args.ppo_epochs,
            ppo_clip=args.ppo_clip, gae_lambda=args.gae_lambda, max_grad_norm=args.max_grad_norm,
            learn_comm=args.learn_comm, comm_lr=args.comm_lr,
            temperature=args.temperature, explore_eps=args.explore_eps, augment=args.augment, mix=args.mix, color=args.color,
            class_weights=args.class_weights, label_smoothing=args.label_smoothing, error_steps=args.error_steps,
            weight_rewards=args.weight_rewards,
            weight_decay=args.weight_decay, decay_all=args.decay_all, lr_groups=args.lr_groups,
            lr_schedule=args.lr_schedule, warmup_steps=args.warmup_steps, adam_betas=args.adam_betas, ema=args.ema,
            eval_ema=args.eval_ema, resume=args.resume,
            report=args.report, report_topk=args.report_topk, report_bins=args.report_bins, exit_at=args.exit_at,
        )
        train_main(main_config, model_config, train_config, exact_standardize=args.exact_standardize)
    elif args.main_choice == "test":
        from .eval import eval_main

        eval_main(main_config, EvalConfig(
            img_size=args.img_size, state_dict_path=args.state_dict_path, batch_size=args.batch_size,
            json_path=args.json_path, dataset_path=args.dataset_path, output_dir=args.output_dir,
            comm=args.comm, comm_range=args.comm_range, greedy=args.greedy, temperature=args.temperature,
            tta=args.tta, normalize=args.normalize, report=args.report, report_topk=args.report_topk, report_bins=args.report_bins,
            exit_at=args.exit_at))
    elif args.main_choice == "infer":
        import os

        from .infer import infer_main

        if os.path.exists(args.output_image_dir) and not os.path.isdir(args.output_image_dir):
            raise NotADirectoryError(f'"{args.output_image_dir}" is not a directory.')
        os.makedirs(args.output_image_dir, exist_ok=True)
        infer_main(main_config, InferConfig(
            state_dict_path=args.state_dict_path, json_path=args.json_path, images_path=args.infer_images,
            output_dir=args.output_image_dir, class_to_idx=args.class_to_idx, saliency=args.saliency,
            comm=args.comm, comm_range=args.comm_range, greedy=args.greedy, temperature=args.temperature,
            normalize=args.normalize))


if __name__ == "__main__":
    main()
