"""optim.py on the host: the float64 definition against torch.optim.AdamW, the schedule, the segment table, the two
command-line grammars, every guard, and the trainer-state file format (no GPU)."""
import math
import os
import re

import pytest
import torch as th

from marlclassification_amd import _lib
from marlclassification_amd import optim as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = "_ModelsWrapper__"
SHAPES = {
    _P + "map_obs.layers.0.weight": (4, 3, 3, 3),   # 108 floats
    _P + "map_obs.layers.0.bias": (4,),
    _P + "map_obs.layers.1.weight": (4,),           # a norm gain
    _P + "map_pos.0.weight": (5, 2),                # 10 floats: 2 of padding behind it
    _P + "map_pos.0.bias": (5,),
    _P + "policy.0.weight": (6, 5),
    _P + "policy.0.bias": (6,),
    _P + "critic.0.weight": (3, 5),                 # 15 floats
    _P + "critic.0.bias": (3,),
    _P + "predict.0.weight": (7, 5),
}


class Flat:
    """The host side of fused.FlatParams (names, offsets, shapes, numel: 16-byte aligned slices)."""

    def __init__(self, shapes):
        self.names, self.shapes, self.offsets = list(shapes), dict(shapes), {}
        off = 0
        for k, s in shapes.items():
            self.offsets[k] = off
            off += (math.prod(s) + 3) & ~3
        self.numel = off


def _sched(kind="cosine", base=1e-2, warm=2, total=10, fr=0.1):
    return O.Schedule(kind, base, warm, total, fr)


# ---- reference_step against torch.optim.AdamW ---------------------------------------------------------------------
@pytest.mark.parametrize("decay", ["matrices", "all"])
def test_reference_step_is_adamw_with_parameter_groups(decay):
    flat = Flat(SHAPES)
    opts = O.OptimOptions(weight_decay=0.05, decay=decay, groups={"cnn": 0.1, "critic": 0.0, "policy": (2.0, 0.3)},
                          betas=(0.8, 0.95), eps=1e-6, schedule=_sched())
    table = O.segments(flat, opts)
    assert any(m == 0.0 for _, _, m, _ in table), "one group must be frozen"
    g = th.Generator().manual_seed(3)
    params = {k: th.randn(s, generator=g, dtype=th.float64).requires_grad_() for k, s in SHAPES.items()}
    start = {k: p.detach().clone() for k, p in params.items()}
    # torch: one group per tensor, weight decay from the options, lr set to lr_at(step) * mult before every step
    # (a frozen tensor gets lr 0 AND no decay: AdamW at lr 0 leaves the weights alone, but we also leave the moments)
    groups = []
    for k, p in params.items():
        mult, wd = opts.tensor_options(k, SHAPES[k])
        groups.append({"params": [p], "weight_decay": wd, "mult": mult})
    live = [gr for gr in groups if gr["mult"] != 0.0]
    adamw = th.optim.AdamW(live, lr=1.0, betas=opts.betas, eps=opts.eps)
    p = th.zeros(flat.numel, dtype=th.float64)
    for k in flat.names:
        p[flat.offsets[k]: flat.offsets[k] + start[k].numel()] = start[k].flatten()
    m, v = th.zeros_like(p), th.zeros_like(p)
    for step in (1, 2, 3):
        grad = th.zeros_like(p)
        for k, q in params.items():
            q.grad = th.randn(SHAPES[k], generator=g, dtype=th.float64)
            grad[flat.offsets[k]: flat.offsets[k] + q.numel()] = q.grad.flatten()
        for gr in live:
            gr["lr"] = O.lr_at(opts.schedule, step) * gr["mult"]
        adamw.step()
        O.reference_step(p, grad, m, v, None, table, opts, step)
        for k, q in params.items():
            mine = p[flat.offsets[k]: flat.offsets[k] + q.numel()].view(SHAPES[k])
            assert th.allclose(mine, q.detach(), rtol=1e-12, atol=1e-14), (step, k)
    for k in flat.names:
        moved = not th.equal(params[k].detach(), start[k])
        assert moved == (O.group_name(k) != "critic"), k
        lo, n = flat.offsets[k], start[k].numel()
        if O.group_name(k) == "critic":  # frozen: weights and moments keep every bit
            assert th.equal(p[lo: lo + n], start[k].flatten()) and not m[lo: lo + n].any() and not v[lo: lo + n].any()
    # decay filter: a bias decays only under "all"
    bias = _P + "predict.0.weight", _P + "map_pos.0.bias"
    assert opts.tensor_options(bias[0], (7, 5))[1] == 0.05
    assert opts.tensor_options(bias[1], (5,))[1] == (0.05 if decay == "all" else 0.0)


def test_reference_step_ema_and_grad_scale():
    opts = O.OptimOptions(ema_decay=0.75, schedule=_sched("constant", 1e-2, 0, 0, 0.0))
    p = th.tensor([1.0, -2.0, 0.5, 3.0], dtype=th.float64)
    g = th.tensor([0.3, -0.1, 0.2, 1.0], dtype=th.float64)
    p2, m2, v2 = p.clone(), th.zeros(4, dtype=th.float64), th.zeros(4, dtype=th.float64)
    ema = p.clone()
    m, v = th.zeros(4, dtype=th.float64), th.zeros(4, dtype=th.float64)
    O.reference_step(p, g * 4, m, v, ema, [(0, 4, 1.0, 0.0)], opts, 1, grad_scale=0.25)
    O.reference_step(p2, g, m2, v2, None, [(0, 4, 1.0, 0.0)], opts, 1)
    assert th.allclose(p, p2, rtol=1e-15) and th.allclose(m, m2, rtol=1e-15)
    start = th.tensor([1.0, -2.0, 0.5, 3.0], dtype=th.float64)
    assert th.allclose(ema, 0.75 * start + 0.25 * p, rtol=1e-15)


# ---- the schedule ---------------------------------------------------------------------------------------------------
def test_lr_at_points():
    base = 3e-3
    for kind in ("linear", "cosine"):
        s = O.Schedule(kind, base, 4, 20, 0.1)
        assert O.lr_at(s, 1) == base * 1.0 / 4.0
        assert O.lr_at(s, 4) == base
        x = 1.0 / 16.0
        want = base * (1 - 0.9 * x) if kind == "linear" else base * (0.1 + 0.9 * 0.5 * (1 + math.cos(math.pi * x)))
        assert O.lr_at(s, 5) == want and want < base
        assert O.lr_at(s, 20) == pytest.approx(0.1 * base, rel=1e-15)
        assert O.lr_at(s, 21) == O.lr_at(s, 20) == O.lr_at(s, 10 ** 9)
        # no warm-up: the first step already decays
        s0 = O.Schedule(kind, base, 0, 20, 0.1)
        assert O.lr_at(s0, 1) < base and O.lr_at(s0, 20) == pytest.approx(0.1 * base, rel=1e-15)
        # final_ratio 0 and 1
        assert O.lr_at(O.Schedule(kind, base, 4, 20, 0.0), 20) == pytest.approx(0.0, abs=1e-18)
        assert all(O.lr_at(O.Schedule(kind, base, 4, 20, 1.0), t) == pytest.approx(base, rel=1e-15)
                   for t in (4, 5, 12, 20, 30))
        # total_steps == warmup_steps: the final rate right behind the warm-up
        assert O.lr_at(O.Schedule(kind, base, 4, 4, 0.5), 5) == pytest.approx(0.5 * base, rel=1e-15)
    c = O.Schedule("constant", base, 3, 0, 0.0)
    assert [O.lr_at(c, t) for t in (3, 4, 1000)] == [base, base, base]
    assert O.lr_at(c, 1) == pytest.approx(base / 3.0, rel=1e-15) and O.lr_at(c, 2) == pytest.approx(2 * base / 3.0, rel=1e-15)
    assert O.lr_at(O.Schedule("constant", base), 1) == base
    with pytest.raises(ValueError):
        O.lr_at(c, 0)
    with pytest.raises(ValueError, match="base_lr"):
        O.lr_at(O.Schedule("cosine", None, 0, 5), 1)
    assert O.Schedule("cosine", None, 0, 5).with_base(0.5).base_lr == 0.5
    assert O.Schedule("cosine", 0.25, 0, 5).with_base(0.5).base_lr == 0.25


# ---- the segment table ----------------------------------------------------------------------------------------------
def test_segments_merge_cover_and_align():
    flat = Flat(SHAPES)
    neutral = O.segments(flat, O.OptimOptions())
    assert neutral == [(0, flat.numel, 1.0, 0.0)], "equal options merge into one segment"
    opts = O.OptimOptions(weight_decay=0.01, groups={"cnn": 0.1, "critic": 0.0})
    table = O.segments(flat, opts)
    assert table[0][0] == 0 and table[-1][1] == flat.numel
    for (b0, e0, m0, w0), (b1, e1, m1, w1) in zip(table, table[1:]):
        assert e0 == b1 and (m0, w0) != (m1, w1)
    assert all(b % 4 == 0 and e > b for b, e, _, _ in table)
    # map_obs bias + norm gain merge (mult 0.1, no decay); critic weight + bias merge (frozen: decay irrelevant?  no -
    # the weight keeps its decay value in the table, so the two stay apart unless it is zero)
    by_start = {b: (e, m, w) for b, e, m, w in table}
    o = flat.offsets
    assert by_start[o[_P + "map_obs.layers.0.weight"]] == (o[_P + "map_obs.layers.0.bias"], 0.1, 0.01)
    assert by_start[o[_P + "map_obs.layers.0.bias"]] == (o[_P + "map_pos.0.weight"], 0.1, 0.0)
    assert O.frozen_ranges(table) == [(b, e) for b, e, m, _ in table if m == 0.0] != []
    assert sum(e - b for b, e in O.frozen_ranges(table)) == 16 + 4
    assert O.segments(flat, O.OptimOptions(weight_decay=0.01, decay="all")) == [(0, flat.numel, 1.0, 0.01)]
    arr = O.segment_array(table)
    assert (arr[1].begin, arr[1].end) == table[1][:2] and arr[0].lr_mult == pytest.approx(0.1)


def test_segments_cap():
    assert O.MAX_SEGMENTS == 128
    hdr = open(os.path.join(ROOT, "include", "marl_hip_optim.h"), encoding="utf-8").read()
    assert int(re.search(r"#define MARL_OPTIM_MAX_SEGMENTS (\d+)", hdr).group(1)) == O.MAX_SEGMENTS
    many = {}
    for i in range(O.MAX_SEGMENTS // 2 + 1):  # weight / bias alternate: two segments per pair under a decay
        many[f"{_P}policy.{i}.weight"] = (2, 2)
        many[f"{_P}policy.{i}.bias"] = (2,)
    assert len(O.segments(Flat(many), O.OptimOptions())) == 1
    with pytest.raises(ValueError, match="at most 128"):
        O.segments(Flat(many), O.OptimOptions(weight_decay=0.1))
    many.popitem()
    many.popitem()
    assert len(O.segments(Flat(many), O.OptimOptions(weight_decay=0.1))) == O.MAX_SEGMENTS


def test_entry_point_is_declared_beside_the_versioned_abi():
    hdr = open(os.path.join(ROOT, "include", "marl_hip_optim.h"), encoding="utf-8").read()
    assert set(re.findall(r"\b(marl_[a-z0-9_]+)\(", hdr)) == {"marl_optim_step"} == set(_lib.OPTIM_ENTRIES)
    assert len(_lib.EXPORTS) == 57 and _lib.MARL_ABI_VERSION == 5 and "marl_optim_step" not in _lib.EXPORTS
    assert set(_lib.OPTIM_ENTRIES) <= set(_lib._HOOKS)
    import ctypes as C

    assert C.sizeof(O.Segment) == 24 and C.sizeof(O.ScheduleDesc) == 40


# ---- grammars and guards --------------------------------------------------------------------------------------------
def test_grammars():
    assert O.parse_groups("cnn=0.1,policy=0,critic=1:0.01") == {"cnn": 0.1, "policy": 0.0, "critic": (1.0, 0.01)}
    assert O.parse_groups("") == {} and O.parse_groups(" predict = 2 ") == {"predict": 2.0}
    o = O.OptimOptions(groups=O.parse_groups("cnn=0.1,critic=1:0.01"))
    assert dict(o.groups) == {"map_obs": (0.1, None), "critic": (1.0, 0.01)}
    assert o.tensor_options(_P + "critic.0.bias", (3,)) == (1.0, 0.0), "a group's decay obeys the filter too"
    assert o.tensor_options(_P + "critic.0.weight", (3, 5)) == (1.0, 0.01)
    for bad in ("cnn", "cnn=", "=1", "cnn=x", "cnn=1:y", "cnn=1,cnn=2", "nope=1"):
        with pytest.raises(ValueError):
            O.parse_groups(bad)
    with pytest.raises(ValueError, match="twice"):
        O.OptimOptions(groups={"cnn": 1.0, "map_obs": 2.0})
    s = O.parse_schedule("cosine:0.1")
    assert (s.kind, s.final_ratio, s.base_lr) == ("cosine", 0.1, None)
    assert O.parse_schedule("linear", 3, 9, 1e-3) == O.Schedule("linear", 1e-3, 3, 9, 0.0)
    assert O.parse_schedule("constant").kind == "constant"
    for bad in ("cosine:x", "step", "cosine:1.5", "cosine:-0.1", ""):
        with pytest.raises(ValueError):
            O.parse_schedule(bad)
    assert O.parse_betas("0.8,0.95") == (0.8, 0.95)
    for bad in ("0.8", "a,b", "0.8,0.9,0.99"):
        with pytest.raises(ValueError):
            O.parse_betas(bad)


def test_guards():
    with pytest.raises(ValueError, match="weight_decay"):
        O.OptimOptions(weight_decay=-0.1)
    with pytest.raises(ValueError, match="weight_decay"):
        O.OptimOptions(groups={"critic": (1.0, -0.5)})
    with pytest.raises(ValueError, match="lr_mult"):
        O.OptimOptions(groups={"critic": -1.0})
    for betas in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.9), (0.9,), (0.9, float("nan"))):
        with pytest.raises(ValueError, match="betas"):
            O.OptimOptions(betas=betas)
    for d in (0.0, 1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            O.OptimOptions(ema_decay=d)
    with pytest.raises(ValueError, match="unknown parameter group") as err:
        O.OptimOptions(groups={"heads": 0.5})
    assert all(name in str(err.value) for name in O.GROUP_NAMES) and "cnn" in str(err.value)
    with pytest.raises(ValueError, match="total_steps"):
        O.Schedule("cosine", 1e-3, 10, 9)
    O.Schedule("constant", 1e-3, 10, 0)  # (a constant schedule never reads total_steps)
    with pytest.raises(ValueError, match="kind"):
        O.Schedule("step")
    with pytest.raises(ValueError, match="eps"):
        O.OptimOptions(eps=0.0)
    with pytest.raises(ValueError, match="decay"):
        O.OptimOptions(decay="biases")
    with pytest.raises(ValueError, match="schedule"):
        O.OptimOptions(schedule="cosine")
    a = O.OptimOptions(weight_decay=0.01, groups={"cnn": 0.1}).with_lr(1e-3)
    b = O.OptimOptions(weight_decay=0.01, groups={"map_obs": 0.1}).with_lr(1e-3)
    assert a == b and hash(a) == hash(b) and a.fingerprint() == b.fingerprint()
    assert a.fingerprint() != O.OptimOptions(weight_decay=0.01, groups={"cnn": 0.1}).with_lr(2e-3).fingerprint()


def test_cli_flags_reach_the_train_config():
    from marlclassification_amd.__main__ import build_parser

    src = open(os.path.join(ROOT, "marlclassification_amd", "__main__.py"), encoding="utf-8").read()
    for flag in ("--weight-decay", "--decay-all", "--lr-groups", "--lr-schedule", "--warmup-steps", "--adam-betas",
                 "--ema", "--eval-ema", "--resume"):
        assert flag in src, flag
    assert callable(build_parser)


# ---- the trainer-state file -----------------------------------------------------------------------------------------
def test_state_dict_file_holds_tensors_numbers_and_strings(tmp_path):
    """What Trainer.state_dict() writes (tests/test_gpu_optim.py round-trips a real one): per-parameter tensors under
    exp_avg. / exp_avg_sq. / ema., numbers and one string - th.load(weights_only=True) must read it back."""
    opts = O.OptimOptions(weight_decay=0.01, ema_decay=0.9).with_lr(1e-3)
    state = {"format": 1, "optim_step": 7, "curr_step": 5, "fingerprint": opts.fingerprint(), "rng_seed": 2 ** 40 + 3,
             "rng_episodes": 11}
    g = th.Generator().manual_seed(0)
    for k, s in SHAPES.items():
        for tag in ("exp_avg", "exp_avg_sq", "ema"):
            state[f"{tag}.{k}"] = th.randn(s, generator=g)
    adam = th.optim.Adam([th.zeros(3, requires_grad=True)], lr=1e-3)
    adam.param_groups[0]["params"][0].grad = th.ones(3)
    adam.step()
    state["comm_adam"] = adam.state_dict()
    path = tmp_path / "trainer.pt"
    th.save(state, path)
    back = th.load(path, weights_only=True)
    assert set(back) == set(state)
    for k, v in state.items():
        if isinstance(v, th.Tensor):
            assert th.equal(back[k], v), k
        elif k != "comm_adam":
            assert back[k] == v and type(back[k]) is type(v), k
    assert th.equal(back["comm_adam"]["state"][0]["exp_avg"], state["comm_adam"]["state"][0]["exp_avg"])


def test_trainer_state_dict_round_trip(tmp_path):
    """A real Trainer.state_dict() (the model on the CPU: no kernel runs) through th.save / th.load(weights_only=True)
    into a fresh trainer; another update rule or another shape is a ValueError."""
    from marlclassification_amd.training import Trainer
    from tests.cases import Case

    k = Case("g1")
    opts = O.OptimOptions(weight_decay=0.01, groups={"critic": 0.0}, ema_decay=0.9)
    model = k.model(th.device("cpu"))
    trainer = Trainer(model, k.cfg.nb_class, 1e-3, 0.99, optim=opts)
    flat = model.flat_state()
    g = th.Generator().manual_seed(5)
    for buf in (flat.exp_avg, flat.exp_avg_sq, flat.ema_buffer()):
        for v in flat._views(buf).values():
            v.copy_(th.randn(v.shape, generator=g))
    flat.step = 5
    th.save(trainer.state_dict(), tmp_path / "trainer.pt")
    state = th.load(tmp_path / "trainer.pt", weights_only=True)
    assert state["optim_step"] == 5 and state["fingerprint"] == trainer.optim_options.fingerprint()
    assert {n.split(".", 1)[0] for n, v in state.items() if isinstance(v, th.Tensor)} == {"exp_avg", "exp_avg_sq", "ema"}
    model2 = k.model(th.device("cpu"))
    trainer2 = Trainer(model2, k.cfg.nb_class, 1e-3, 0.99, optim=opts)
    trainer2.load_state_dict(state)
    flat2 = model2.flat_state()
    assert flat2.step == 5
    for a, b in ((flat.exp_avg, flat2.exp_avg), (flat.exp_avg_sq, flat2.exp_avg_sq), (flat.ema, flat2.ema)):
        assert th.equal(a, b)
    with pytest.raises(ValueError, match="another update rule"):
        Trainer(k.model(th.device("cpu")), k.cfg.nb_class, 1e-3, 0.99).load_state_dict(state)
    with pytest.raises(ValueError, match="another update rule"):
        Trainer(k.model(th.device("cpu")), k.cfg.nb_class, 2e-3, 0.99, optim=opts).load_state_dict(state)
    key = next(n for n in state if n.startswith("ema."))
    state[key] = th.zeros(2, 2)
    with pytest.raises(ValueError, match="needs"):
        trainer2.load_state_dict(state)
