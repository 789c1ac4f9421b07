"""marl_optim_step on the GPU: the kernel on synthetic flat buffers against optim.reference_step in float64 (every
tolerance derived: see ``_bounds``), frozen segments, the trainer paths (A2C, entropy, PPO, two ranks), the hipGraph
replay under a schedule, bit-exact resume, the averaged weights, the defaults, the C guards and the command line.

Per step the float64 reference starts from the GPU's own fp32 state before that step, so each bound is that of ONE
step: parameters 1e-3 of the step (the project's Adam bound, tests/test_gpu_episode.py) plus one ulp of the stored
value; moments and the average three fp32 roundings plus one of slack."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch as th

from marlclassification_amd import _lib
from marlclassification_amd import optim as O
from tests.cases import NS, Case, _golden_sampler, _sampler
from tests.dp import run_ranks
from tests.util import CASES, Golden, model_spec, record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4  # floats before and behind every buffer (16 bytes: the interior stays 16-byte aligned)
GRID_CAP = 4096  # launch_adam's grid cap, 256 threads, one float4 per lane and trip
_ERRORS = {}


def _engine(device):
    from marlclassification_amd.engine import HipEngine

    return HipEngine(model_spec(CASES["g1_conftest"]), device)


def _fenced(src, device):
    """``src`` (fp32, host) between guard floats on the device: (whole buffer, interior view)."""
    whole = th.full((src.numel() + 2 * GUARD,), 12345.5, device=device)
    whole[GUARD: GUARD + src.numel()] = src.to(device)
    return whole, whole[GUARD: GUARD + src.numel()]


def _table(sizes, opts):
    out, at = [], 0
    for n, (mult, wd) in zip(sizes, opts):
        out.append((at, at + n, mult, wd))
        at += n
    return out


def _state(n, seed):
    g = th.Generator().manual_seed(seed)
    p = th.randn(n, generator=g)
    m = 0.1 * th.randn(n, generator=g)
    v = 0.01 * th.rand(n, generator=g)
    return p, m, v


def _bounds(ref, g64, lr_t, table):
    """Per-element bounds from the float64 results ``ref`` = (p, m, v, ema-or-None) of one step."""
    p, m, v, ema = ref
    mult = th.zeros_like(p)
    for b, e, mu, _ in table:
        mult[b:e] = mu
    u = 2.0 ** -24
    out = {"p": 1e-3 * lr_t * mult + 2 * u * p.abs(), "m": 4 * u * (m.abs() + g64.abs()), "v": 4 * u * (v + g64 * g64)}
    if ema is not None:
        out["ema"] = 4 * u * (ema.abs() + p.abs())
    return out


def _check_step(tag, got, ref, g64, lr_t, table, live):
    """``got`` fp32 device tensors against ``ref``; ``live``: a mask of the elements a step touches (not frozen)."""
    bounds = _bounds(ref, g64, lr_t, table)
    for name, r, t in zip(("p", "m", "v", "ema"), ref, got):
        if r is None:
            continue
        err = (t.double().cpu() - r).abs()
        ratio = (err[live] / bounds[name][live].clamp_min(1e-300)).max().item()
        key = f"{tag}/{name}"
        _ERRORS[key] = {"max_err_over_bound": max(ratio, _ERRORS.get(key, {}).get("max_err_over_bound", 0.0)),
                        "margin": 1.0 / max(ratio, _ERRORS.get(key, {}).get("max_err_over_bound", 0.0), 1e-30)}
        print(f"[optim] {key}: max err / bound {ratio:.3e}")
        assert ratio <= 1.0, f"{key}: err / bound {ratio:.3e}"


# sizes in floats, with (lr_mult, weight_decay) in mixed order.  "issue": boundaries inside a wave and inside a workgroup,
# a partial last workgroup.  "edges" adds a boundary on a wave edge (256 floats = 64 float4) and one on a workgroup edge
# (1024 floats): the five sizes alone cannot put one there (their sums are 4 .. 24 mod 256).
LAYOUTS = {
    "issue": ([260, 4, 2052, 8, 1028], [(1.0, 0.1), (0.5, 0.0), (0.1, 0.01), (2.0, 0.3), (1.0, 0.0)]),
    "edges": ([256, 768, 260, 4, 1028, 8, 2052],
              [(1.0, 0.0), (0.25, 0.2), (1.0, 0.1), (0.5, 0.0), (1.0, 0.0), (2.0, 0.3), (0.1, 0.01)]),
}


@pytest.mark.parametrize("with_ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_three_steps_match_float64(device, layout, with_ema):
    eng = _engine(device)
    sizes, so = LAYOUTS[layout]
    table = _table(sizes, so)
    n = table[-1][1]
    assert (n + 3) // 4 % 256 != 0, "the last workgroup must be partial"
    opts = O.OptimOptions(betas=(0.9, 0.99), eps=1e-8, schedule=O.Schedule("cosine", 1e-2, 2, 5, 0.1),
                          ema_decay=0.9 if with_ema else None)
    p0, m0, v0 = _state(n, 1)
    bufs = [_fenced(t, device) for t in (p0, th.zeros(n), m0, v0, p0 + 0.01)]
    (pw, p), (gw, g), (mw, m), (vw, v), (ew, e) = bufs
    scal_w, scal = _fenced(th.zeros(4), device)
    live = th.ones(n, dtype=th.bool)
    gen = th.Generator().manual_seed(2)
    for step in (1, 2, 3):
        g.copy_(th.randn(n, generator=gen) * 0.5)
        before = [t.double().cpu() for t in (p, m, v)] + [e.double().cpu() if with_ema else None]
        g64 = g.double().cpu() * 0.5
        O.reference_step(before[0], g.double().cpu(), before[1], before[2], before[3], table, opts, step,
                         grad_scale=0.5)
        eng.optim_step(p, g, m, v, table, opts, step=step, ema=e if with_ema else None, grad_scale=0.5,
                       scalars_out=scal)
        lr_t = O.lr_at(opts.schedule, step)
        _check_step(f"{layout}/{'ema' if with_ema else 'plain'}", (p, m, v, e), before, g64, lr_t, table, live)
        want = [lr_t, 1 - opts.betas[0] ** step, 1 - opts.betas[1] ** step, float(step)]
        for j, w in enumerate(want):
            assert abs(scal[j].item() - w) <= 2.0 ** -23 * abs(w), (step, j, scal[j].item(), w)
    for whole, _ in bufs + [(scal_w, scal)]:
        assert bool((whole[:GUARD] == 12345.5).all()) and bool((whole[-GUARD:] == 12345.5).all()), "a guard moved"
    if not with_ema:
        assert th.equal(e.cpu(), p0 + 0.01), "no ema buffer was passed"
    record("optim_errors", _ERRORS)


def test_second_pass_of_the_grid_stride_loop(device):
    """n just above 4 * 256 * (grid cap): the first workgroups run a second trip, one of them on a partial float4."""
    eng = _engine(device)
    n = 4 * 256 * GRID_CAP + 4 * 300 + 3
    first = 4 * 256 * GRID_CAP - 1024
    table = [(0, first, 1.0, 0.01), (first, first + 1024 + 512, 0.5, 0.0), (first + 1536, n, 2.0, 0.1)]
    opts = O.OptimOptions(schedule=O.Schedule("linear", 1e-2, 0, 4, 0.0), ema_decay=0.99)
    p0, m0, v0 = _state(n, 5)
    g0 = th.randn(n, generator=th.Generator().manual_seed(6))
    bufs = [_fenced(t, device) for t in (p0, g0, m0, v0, p0 * 0.5)]
    (pw, p), (gw, g), (mw, m), (vw, v), (ew, e) = bufs
    ref = [t.double() for t in (p0, m0, v0, p0 * 0.5)]
    O.reference_step(ref[0], g0.double(), ref[1], ref[2], ref[3], table, opts, 2)
    eng.optim_step(p, g, m, v, table, opts, step=2, ema=e)
    _check_step("second_pass", (p, m, v, e), ref, g0.double(), O.lr_at(opts.schedule, 2), table,
                th.ones(n, dtype=th.bool))
    for whole, _ in bufs:
        assert bool((whole[:GUARD] == 12345.5).all()) and bool((whole[-GUARD:] == 12345.5).all()), "a guard moved"
    record("optim_errors", _ERRORS)


@pytest.mark.parametrize("n", [3, 7, 1030])
def test_lengths_that_are_no_multiple_of_four(device, n):
    """The last, partial float4 is walked per element (n = 3: there is no whole one - the launcher's tiny instance)."""
    eng = _engine(device)
    table = [(0, n, 0.5, 0.1)] if n < 1030 else [(0, 512, 1.0, 0.0), (512, n, 0.5, 0.1)]
    opts = O.OptimOptions(schedule=O.Schedule("linear", 1e-2, 1, 3, 0.5), ema_decay=0.9)
    p0, m0, v0 = _state(n, 20 + n)
    g0 = th.randn(n, generator=th.Generator().manual_seed(n))
    bufs = [_fenced(t, device) for t in (p0, g0, m0, v0, p0 * 0.5)]
    (pw, p), (gw, g), (mw, m), (vw, v), (ew, e) = bufs
    ref = [t.double() for t in (p0, m0, v0, p0 * 0.5)]
    O.reference_step(ref[0], g0.double(), ref[1], ref[2], ref[3], table, opts, 2)
    eng.optim_step(p, g, m, v, table, opts, step=2, ema=e)
    _check_step(f"ragged/{n}", (p, m, v, e), ref, g0.double(), O.lr_at(opts.schedule, 2), table,
                th.ones(n, dtype=th.bool))
    for whole, _ in bufs:
        assert bool((whole[:GUARD] == 12345.5).all()) and bool((whole[-GUARD:] == 12345.5).all()), "a guard moved"
    assert not th.equal(p.cpu(), p0)


def _bits(t):
    return t.view(th.int32).clone()


def test_frozen_segment_keeps_every_bit(device):
    eng = _engine(device)
    sizes, so = [260, 1028, 8, 516], [(1.0, 0.1), (0.0, 0.5), (0.0, 0.0), (0.5, 0.0)]
    table = _table(sizes, so)
    n = table[-1][1]
    opts = O.OptimOptions(schedule=O.Schedule("constant", 1e-2), ema_decay=0.9)
    p0, m0, v0 = _state(n, 7)
    g0 = th.randn(n, generator=th.Generator().manual_seed(8))
    lo, hi = 260, 260 + 1028 + 8
    g0[lo:hi] = float("nan")
    p0[lo + 5] = float("nan")
    p0[lo + 8: lo + 40] = -0.0
    p0[hi - 3] = -0.0
    m0[lo + 9] = -0.0
    p, g, m, v, e = (t.to(device) for t in (p0, g0, m0, v0, p0.clone()))
    e[lo + 17] = float("nan")
    before = [_bits(t) for t in (p, m, v, e)]
    for step in (1, 2):
        eng.optim_step(p, g, m, v, table, opts, step=step, ema=e)
    for name, t, b in zip("pmve", (p, m, v, e), before):
        assert th.equal(_bits(t)[lo:hi], b[lo:hi]), f"{name}: the frozen segment changed"
        for a, z in ((0, lo), (hi, n)):
            assert bool(th.isfinite(t[a:z]).all()), f"{name}: a neighbour is not finite"
            assert not th.equal(_bits(t)[a:z], b[a:z]), f"{name}: a neighbour was not updated"
    assert int((_bits(p)[: lo] != before[0][: lo]).sum()) == lo, "every neighbouring parameter moves"


def test_neutral_options_are_adam(device):
    eng = _engine(device)
    n = 3352
    p0, m0, v0 = _state(n, 9)
    g0 = th.randn(n, generator=th.Generator().manual_seed(10))
    opts = O.OptimOptions(schedule=O.Schedule("constant", 1e-3))
    a = [t.to(device) for t in (p0, g0, m0, v0)]
    b = [t.to(device) for t in (p0, g0, m0, v0)]
    for step in (1, 2, 3):
        eng.adam(*a, step, 1e-3)
        eng.optim_step(*b, [(0, n, 1.0, 0.0)], opts, step=step)
        tol = 1e-3 * 1e-3 + 2.0 ** -23 * a[0].abs()
        assert bool(((a[0] - b[0]).abs() <= tol).all()), step
        b[0].copy_(a[0]), b[2].copy_(a[2]), b[3].copy_(a[3])  # (each step is compared from a common state)


# ---- guards through ctypes ------------------------------------------------------------------------------------------
def test_guards_return_einval_and_touch_nothing(device):
    eng = _engine(device)
    lib = eng.lib
    n = 1024
    p0, m0, v0 = _state(n, 11)
    bufs = [t.to(device) for t in (p0, th.ones(n), m0, v0, p0.clone())]
    before = [t.clone() for t in bufs]
    sched = O.Schedule("cosine", 1e-2, 1, 4, 0.0).desc()
    cnt = eng.new_counters()

    def call(table, ptrs=None, step=1, counters=None, nn=n, betas=(0.9, 0.999), ema_decay=0.9, nseg=None, sd=sched):
        ptrs = [t.data_ptr() for t in bufs] if ptrs is None else ptrs
        arr = O.segment_array(table)
        return lib.marl_optim_step(*ptrs, nn, 1.0, C.cast(arr, C.c_void_p), len(table) if nseg is None else nseg,
                                   betas[0], betas[1], 1e-8, C.cast(C.pointer(sd), C.c_void_p), step, counters,
                                   ema_decay, None, None)

    good = [(0, 512, 1.0, 0.0), (512, n, 0.5, 0.1)]
    ptrs = [t.data_ptr() for t in bufs]
    bad = {
        "misaligned begin": lambda: call([(0, 510, 1.0, 0.0), (510, n, 0.5, 0.1)]),
        "gap": lambda: call([(0, 508, 1.0, 0.0), (512, n, 0.5, 0.1)]),
        "overlap": lambda: call([(0, 516, 1.0, 0.0), (512, n, 0.5, 0.1)]),
        "unordered": lambda: call([(512, n, 0.5, 0.1), (0, 512, 1.0, 0.0)]),
        "short": lambda: call([(0, 512, 1.0, 0.0)]),
        "too many": lambda: call([(4 * i, 4 * i + 4, 1.0, 0.0) for i in range(O.MAX_SEGMENTS + 1)],
                                 nn=4 * (O.MAX_SEGMENTS + 1)),
        "step 0": lambda: call(good, step=0),
        "null params": lambda: call(good, ptrs=[None] + ptrs[1:]),
        "null grads": lambda: call(good, ptrs=ptrs[:1] + [None] + ptrs[2:]),
        "null exp_avg": lambda: call(good, ptrs=ptrs[:2] + [None] + ptrs[3:]),
        "null exp_avg_sq": lambda: call(good, ptrs=ptrs[:3] + [None] + ptrs[4:]),
        "misaligned buffer": lambda: call(good, ptrs=[ptrs[0] + 4] + ptrs[1:], nn=n),
        "beta1 = 1": lambda: call(good, betas=(1.0, 0.999)),
        "ema_decay = 1": lambda: call(good, ema_decay=1.0),
        "negative multiplier": lambda: call([(0, 512, -1.0, 0.0), (512, n, 0.5, 0.1)]),
        "total < warmup": lambda: call(good, sd=O.ScheduleDesc(2, 0, 1e-2, 5, 4, 0.0)),
        "unknown kind": lambda: call(good, sd=O.ScheduleDesc(3, 0, 1e-2, 0, 4, 0.0)),
    }
    for what, fn in bad.items():
        assert fn() == -1, what  # MARL_EINVAL
        assert lib.marl_last_error().decode().startswith("optim_step"), what
    th.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert th.equal(t, b), "a refused call wrote"
    # the same table is accepted: with a step, and with a counter block in its place
    assert call(good) == 0
    eng.counters_set(cnt, 0, 2, 1e-2)
    assert call(good, step=0, counters=cnt.data_ptr()) == 0
    th.cuda.synchronize()
    assert not th.equal(bufs[0], before[0])
    with pytest.raises(RuntimeError, match="ema_decay"):  # (an ema buffer under options without a decay)
        eng.optim_step(*bufs[:4], good, O.OptimOptions(schedule=O.Schedule("constant", 1e-2)), step=1, ema=bufs[4])


# ---- trainer level --------------------------------------------------------------------------------------------------
TRAIN_OPTS = dict(weight_decay=0.01, groups={"cnn": 0.1, "critic": 0.0}, ema_decay=0.9)


def _train_opts(total):
    return O.OptimOptions(schedule=O.Schedule("cosine", None, 1, total, 0.0), **TRAIN_OPTS)


class G4Case:
    """The G4 shape (g4_resisc_b2: the flagship widths at batch 2) with Case's interface."""

    def __init__(self):
        g = Golden("g4_resisc_b2")
        self.cfg, self.na, self.nb, self.params, self.img, self.inp = g.cfg, g.na, g.nb, g.params, g.img, g.inp
        assert g.ns >= NS

    def model(self, device):
        from marlclassification_amd.networks import ModelsWrapper
        from marlclassification_amd.networks.vision import Resisc45Cnn

        c = self.cfg
        m = ModelsWrapper(Resisc45Cnn(c.window), c.n_b, c.n_a, c.n_m, c.n_m_o, c.n_d, 2, c.nb_action, c.nb_class,
                          c.nlb, c.nla)
        m.load_state_dict(self.params)
        return m.to(device)


def _case(name):
    return G4Case() if name == "g4" else Case(name)


def _y(k):
    return th.randint(0, k.cfg.nb_class, (k.nb,), generator=th.Generator().manual_seed(77))


def _checked_optim_step(monkeypatch, tag, flat_of, opts_of, steps_seen):
    """Wraps HipEngine.optim_step: every call is compared with reference_step in float64, fed the state before the
    call and the gradient buffer the kernel reads (the GPU's own gradients)."""
    from marlclassification_amd.engine import HipEngine

    real = HipEngine.optim_step

    def wrapped(self, params, grads, exp_avg, exp_avg_sq, table, opts, step=0, ema=None, grad_scale=1.0,
                counters=None, scalars_out=None):
        flat = flat_of()
        tab = O.segments(flat, opts)
        ref = [t.double().cpu() for t in (params, exp_avg, exp_avg_sq)] + [None if ema is None else ema.double().cpu()]
        g64 = grads.double().cpu()
        O.reference_step(ref[0], g64, ref[1], ref[2], ref[3], tab, opts, step, grad_scale=grad_scale)
        real(self, params, grads, exp_avg, exp_avg_sq, table, opts, step=step, ema=ema, grad_scale=grad_scale,
             counters=counters, scalars_out=scalars_out)
        live = th.zeros(flat.numel, dtype=th.bool)
        for b, e, mu, _ in tab:
            live[b:e] = mu != 0.0
        _check_step(tag, (params, exp_avg, exp_avg_sq, ema), ref, g64 * grad_scale, O.lr_at(opts.schedule, step), tab,
                    live)
        assert abs(scalars_out[0].item() - O.lr_at(opts.schedule, step)) <= 2.0 ** -23 * O.lr_at(opts.schedule, step)
        steps_seen.append(step)

    monkeypatch.setattr(HipEngine, "optim_step", wrapped)


@pytest.mark.parametrize("variant", ["a2c", "entropy", "ppo2"])
@pytest.mark.parametrize("name", ["g1", "g4"])
def test_train_steps_match_float64(device, monkeypatch, name, variant):
    from marlclassification_amd.training import Trainer

    k = _case(name)
    y = _y(k)
    model = k.model(device)
    sampler = _sampler(k, model, device, probs=False)
    kw = {"a2c": {}, "entropy": {"entropy_coef": 0.05}, "ppo2": {"ppo_epochs": 2, "ppo_clip": 0.1}}[variant]
    per = 2 if variant == "ppo2" else 1
    trainer = Trainer(model, k.cfg.nb_class, 1e-3, 0.99, optim=_train_opts(2 * per), **kw)
    seen = []
    _checked_optim_step(monkeypatch, f"train/{name}/{variant}", model.flat_state, lambda: trainer.optim_options, seen)
    start = {n: v.clone() for n, v in model.state_dict().items()}
    for _ in range(2):
        trainer.train_step(k.img, y, sampler)
    assert seen == list(range(1, 2 * per + 1)), "the schedule advances once per optimiser step"
    sd = model.state_dict()
    moved = 0
    for n in sd:
        if O.group_name(n) == "critic":
            assert th.equal(_bits(sd[n]), _bits(start[n])), f"{n}: a frozen tensor changed"
        else:
            moved += int(not th.equal(sd[n], start[n]))
    assert moved > 0
    assert trainer.metrics()["lr"] == th.tensor(O.lr_at(trainer.optim_options.schedule, 2 * per)).float().item()
    flat = model.flat_state()
    assert flat.ema is not None and not th.equal(flat.ema, flat.params)
    record("optim_errors", _ERRORS)


# ---- hipGraph -------------------------------------------------------------------------------------------------------
def test_graph_replay_under_a_schedule_equals_eager_bit_for_bit(device):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.fused import FlatParams, FusedA2C, draw_episode_device
    from oracle import marl_oracle as mo

    g = Golden("g2_mnist_c1")
    img, y = g.img.to(device), g.y.to(device)
    opts = O.OptimOptions(weight_decay=0.01, groups={"cnn": 0.5}, schedule=O.Schedule("cosine", None, 2, 6, 0.1),
                          ema_decay=0.9)
    finals, sets = [], []
    for use_graph in (False, True):
        eng = HipEngine(model_spec(g.cfg), device)
        eng.configure(g.na, g.nb, g.ns, g.img.shape[1:])
        flat = FlatParams(mo.param_shapes(g.cfg), device)
        flat.load(g.params)
        fa = FusedA2C(eng, flat, 1e-3, g.gamma, use_graph=use_graph, optim=opts)
        real, calls = eng.counters_set, []
        eng.counters_set = lambda *a, **kw: (calls.append(a), real(*a, **kw))[1]
        lrs = []
        for it in range(6):
            if use_graph:
                fa.iteration_graph(img, y, 77, it)
                if it == 0:
                    after_capture = len(calls)
            else:
                fa.iteration(img, y, draw_episode_device(eng, 77, it))
            lrs.append(fa._optim.scalars[0].item())
        th.cuda.synchronize()
        if use_graph:
            assert len(calls) == after_capture == 1, "no counters_set may run between the replays"
        want = [th.tensor(O.lr_at(fa._optim.opts.schedule, t)).float().item() for t in range(1, 7)]
        assert lrs == want, (lrs, want)
        finals.append([t.clone() for t in (flat.params, flat.exp_avg, flat.exp_avg_sq, flat.ema)] + [flat.step])
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema"), finals[0], finals[1]):
        assert th.equal(a, b), f"{name}: the replays and the eager iterations differ"
    assert finals[0][4] == finals[1][4] == 6


# ---- resume ---------------------------------------------------------------------------------------------------------
def _fresh(k, device, weights=None, opts=None):
    from marlclassification_amd.core import Environment, EpisodeSampler, MultiAgent
    from marlclassification_amd.training import Trainer

    model = k.model(device)
    if weights is not None:
        model.load_state_dict(weights)
    sampler = EpisodeSampler(MultiAgent(k.na, model), Environment(k.cfg.actions, k.cfg.window), NS)
    assert sampler.device_rng
    trainer = Trainer(model, k.cfg.nb_class, 1e-3, 0.99, optim=_train_opts(4) if opts is None else opts)
    return model, sampler, trainer


def _flat_bits(model):
    f = model.flat_state()
    return [t.clone() for t in (f.params, f.exp_avg, f.exp_avg_sq, f.ema) if t is not None]


def test_resume_continues_bit_for_bit(device, tmp_path):
    k = Case("g1")
    y = _y(k)
    batches = [(k.img + 0.01 * i, y.roll(i)) for i in range(4)]
    th.manual_seed(4242)
    model, sampler, trainer = _fresh(k, device)
    acts = [trainer.train_step(x, t, sampler)[0].step_actions.clone() for x, t in batches]
    whole = _flat_bits(model)

    th.manual_seed(4242)
    model, sampler, trainer = _fresh(k, device)
    for x, t in batches[:2]:
        trainer.train_step(x, t, sampler)
    th.save(trainer.state_dict(sampler), tmp_path / "trainer.pt")
    th.save(model.state_dict(), tmp_path / "model.pt")
    del model, sampler, trainer
    th.manual_seed(1)  # (a process seeded otherwise: the state names the seed of its generator stream)
    state = th.load(tmp_path / "trainer.pt", weights_only=True)
    assert state["optim_step"] == 2 and state["curr_step"] == 0 and state["rng_episodes"] == 2
    assert all(isinstance(v, (th.Tensor, int, float, str)) for v in state.values())
    weights = th.load(tmp_path / "model.pt", weights_only=True)
    model, sampler, trainer = _fresh(k, device, weights)
    trainer.load_state_dict(state, sampler)
    assert th.initial_seed() == 4242
    acts2 = [trainer.train_step(x, t, sampler)[0].step_actions.clone() for x, t in batches[2:]]
    assert model.flat_state().step == 4
    for a, b in zip(acts[2:], acts2):
        assert th.equal(a, b), "the resumed run sampled other actions"
    assert not th.equal(acts[2], acts[3])
    for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "ema"), whole, _flat_bits(model)):
        assert th.equal(a, b), f"{name}: the resumed run differs"
    # another update rule, a missing entry, another shape
    _, _, other = _fresh(k, device, weights, O.OptimOptions(weight_decay=0.02, ema_decay=0.9))
    with pytest.raises(ValueError, match="another update rule"):
        other.load_state_dict(state)
    _, _, plain = _fresh(k, device, weights)
    broken = dict(state)
    key = next(n for n in state if n.startswith("exp_avg_sq."))
    broken[key] = th.zeros(3, 3)
    with pytest.raises(ValueError, match="needs"):
        plain.load_state_dict(broken)
    del broken[key]
    with pytest.raises(ValueError, match="missing"):
        plain.load_state_dict(broken)


# ---- the averaged weights -------------------------------------------------------------------------------------------
def test_ema_weights_context(device):
    from marlclassification_amd.training import Trainer

    k = Case("g1")
    y = _y(k)
    runs = []
    for use_context in (True, False):
        model = k.model(device)
        sampler = _sampler(k, model, device, probs=False)
        trainer = Trainer(model, k.cfg.nb_class, 1e-2, 0.99, optim=_train_opts(3))
        for _ in range(2):
            trainer.train_step(k.img, y, sampler)
        if use_context:
            trained = {n: v.clone() for n, v in model.state_dict().items()}
            with trainer.ema_weights():
                inside = sampler.run_episode(k.img)
                ema_sd = {n: v.clone() for n, v in model.state_dict().items()}  # (nn_models_ema-style weights)
            assert all(th.equal(_bits(v), _bits(trained[n])) for n, v in model.state_dict().items())
            assert any(not th.equal(ema_sd[n], trained[n]) for n in trained)
            twin = k.model(device)
            twin.load_state_dict(ema_sd)
            out2 = _sampler(k, twin, device, probs=False).run_episode(k.img)
            for f in ("step_preds", "step_log_probas", "step_values", "step_pos"):
                assert th.equal(getattr(inside, f), getattr(out2, f)), f
            plain = sampler.run_episode(k.img)
            assert not th.equal(plain.step_preds, inside.step_preds), "the context must change the weights in use"
        trainer.train_step(k.img, y, sampler)
        runs.append(_flat_bits(model))
    for a, b in zip(*runs):
        assert th.equal(a, b), "the step after the context differs from one without it"
    with pytest.raises(ValueError, match="ema_decay"):
        with Trainer(k.model(device), k.cfg.nb_class, 1e-2, 0.99).ema_weights():
            pass


# ---- defaults -------------------------------------------------------------------------------------------------------
def test_defaults_call_adam_only(device, monkeypatch):
    from marlclassification_amd.engine import HipEngine
    from marlclassification_amd.training import Trainer

    calls = {"adam": 0, "optim_step": 0}
    for name in calls:
        real = getattr(HipEngine, name)

        def counted(self, *a, _real=real, _name=name, **kw):
            calls[_name] += 1
            return _real(self, *a, **kw)

        monkeypatch.setattr(HipEngine, name, counted)
    k = Case("g1")
    y = _y(k)
    finals = []
    for kw in ({}, {"optim": None}):
        model = k.model(device)
        sampler = _sampler(k, model, device, probs=False)
        trainer = Trainer(model, k.cfg.nb_class, 1e-3, 0.99, **kw)
        for _ in range(2):
            trainer.train_step(k.img, y, sampler)
        assert "lr" not in trainer.metrics() and model.flat_state().ema is None
        finals.append(_flat_bits(model)[:3])
    assert calls == {"adam": 4, "optim_step": 0}
    for a, b in zip(*finals):
        assert th.equal(a, b)
    model = k.model(device)
    Trainer(model, k.cfg.nb_class, 1e-3, 0.99, optim=O.OptimOptions()).train_step(
        k.img, y, _sampler(k, model, device, probs=False))
    assert calls == {"adam": 4, "optim_step": 1}


# ---- two ranks ------------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, out_q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from marlclassification_amd.fused import EpisodeDraws
    from marlclassification_amd.parallel import GradAllReduce, broadcast_parameters, shard_bounds
    from marlclassification_amd.training import Trainer

    device = th.device("cuda:0")  # both ranks share the one GPU of the test box
    g = Golden("g2_mnist_c1")
    model, sampler = _golden_sampler(g, device)
    flat = model.flat_state()
    broadcast_parameters(flat.params)
    lo, hi = shard_bounds(g.nb, rank, world)
    i = g.inp
    sampler.fixed_draws = EpisodeDraws(*(t.to(device) for t in (
        i.pos0[:, lo:hi].contiguous(), i.h0[:, lo:hi].contiguous(), i.c0[:, lo:hi].contiguous(),
        i.hc0[:, lo:hi].contiguous(), i.cc0[:, lo:hi].contiguous(), i.q[:, :, lo:hi].contiguous())))
    inner, reduced = GradAllReduce(world), []  # (one bucket)

    def hook(grads):
        scale = inner(grads)
        reduced.append(grads.double().cpu() * scale)
        return scale

    opts = O.OptimOptions(weight_decay=0.01, groups={"cnn": 0.1, "critic": 0.0},
                          schedule=O.Schedule("cosine", None, 1, 2, 0.0), ema_decay=0.9)
    trainer = Trainer(model, g.cfg.nb_class, g.lr, g.gamma, allreduce=hook, max_grad_norm=0.05, optim=opts)
    table = O.segments(flat, trainer.optim_options)
    live = th.zeros(flat.numel, dtype=th.bool)
    for b, e, mu, _ in table:
        live[b:e] = mu != 0.0
    norms = []
    for _ in range(2):
        trainer.train_epoch([(g.img[lo:hi], g.y[lo:hi])], 0, sampler)
        full = reduced[-1]
        norms.append((trainer._Trainer__grad_norm.item(), full[live].norm().item(), full[~live].norm().item()))
    th.cuda.synchronize()
    out_q.put((rank, flat.params.cpu().numpy(), flat.ema.cpu().numpy(), norms, flat.step))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_identical_parameters_and_ema(device):
    import numpy as np

    res = sorted(run_ranks(_dp_worker, 2, results=2), key=lambda r: r[0])
    (_, p0, e0, n0, s0), (_, p1, e1, n1, s1) = res
    assert s0 == s1 == 2
    assert np.array_equal(p0, p1), "parameters differ between the ranks"
    assert np.array_equal(e0, e1) and not np.array_equal(e0, p0), "the averaged weights differ between the ranks"
    for got, trainable, frozen in n0 + n1:
        assert frozen > 0.0, "the frozen group must have a gradient to ignore"
        assert abs(got - trainable) <= 1e-6 * trainable, (got, trainable)  # (marl_grad_clip's own bound)
        assert got > 0.05, "the bound must bite"


# ---- command line ---------------------------------------------------------------------------------------------------
_CLI = """
import sys
from marlclassification_amd.__main__ import main
common = ("-a 3 --step 3 --cuda --run-id opt train --ft-extr mnist --f 6 --img-size 28 --nb-class 10 --nb 16 --na 16 "
          "--nm 8 --nmo 12 --nd 4 --nlb 24 --nla 24 --batch-size 16 --nb-epoch 3 --lr 1e-3 --res-folder synthetic "
          "--weight-decay 0.01 --lr-groups cnn=0.1,critic=0 --lr-schedule cosine:0.1 --warmup-steps 2 "
          "--adam-betas 0.9,0.99 --ema 0.9 --eval-ema ")
main((common + "-o " + sys.argv[1]).split())
print("=== resumed ===", flush=True)
main((common + "-o " + sys.argv[2] + " --resume " + sys.argv[1] + "/models/trainer_epoch_1.pt").split())
"""


def test_command_line_trains_and_resumes(device, tmp_path):
    """One fresh child: a three-epoch run, then its third epoch again from the checkpoint of the second (--resume with
    the interrupted run's flags: the schedule's length is part of the update rule).  The resumed epoch writes the bits
    the uninterrupted one wrote."""
    import json
    import re

    a, b = tmp_path / "run", tmp_path / "resumed"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), MARL_SEED="11")
    for v in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(v, None)
    r = subprocess.run([sys.executable, "-c", _CLI, str(a), str(b)], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    first, _, second = r.stdout.partition("=== resumed ===")
    for e in range(3):
        for f in (f"nn_models_epoch_{e}.pt", f"trainer_epoch_{e}.pt", f"nn_models_ema_epoch_{e}.pt"):
            assert (a / "models" / f).exists(), f
    assert "resumed from epoch 1" in second and "\nepoch 0:" not in second and "\nepoch 1:" not in second
    cfg = json.loads((a / "marl.json").read_text())
    assert not any(w in key for key in cfg for w in ("decay", "schedule", "ema", "warmup", "resume", "lr_groups"))
    state = th.load(a / "models" / "trainer_epoch_1.pt", weights_only=True)
    per_epoch = state["optim_step"] // 2
    assert per_epoch >= 2 and state["epoch"] == 1
    sched = O.Schedule("cosine", 1e-3, 2, 3 * per_epoch, 0.1)
    lr_line = re.search(r"epoch 2: .*\blr=([0-9.e+-]+)", second)
    assert lr_line, second[-2000:]
    want = O.lr_at(sched, 3 * per_epoch)  # (the epoch line logs the rate of the epoch's last step)
    assert abs(float(lr_line.group(1)) - want) <= 2.0 ** -23 * want, (lr_line.group(1), want)
    assert re.search(r"epoch 2: .*\blr=([0-9.e+-]+)", first).group(1) == lr_line.group(1)
    for f in ("nn_models_epoch_2.pt", "nn_models_ema_epoch_2.pt"):
        x = th.load(a / "models" / f, map_location="cpu", weights_only=True)
        z = th.load(b / "models" / f, map_location="cpu", weights_only=True)
        assert set(x) == set(z) and all(th.equal(x[n], z[n]) for n in x), f"{f}: the resumed epoch differs"
    ema = th.load(a / "models" / "nn_models_ema_epoch_2.pt", map_location="cpu", weights_only=True)
    plain = th.load(a / "models" / "nn_models_epoch_2.pt", map_location="cpu", weights_only=True)
    assert set(ema) == set(plain) and any(not th.equal(ema[n], plain[n]) for n in plain)
