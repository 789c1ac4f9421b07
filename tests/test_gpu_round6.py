"""GPU, round 6: (a) a direct HipEngine user survives a knob change between pack() and the compute calls (ADVICE r5,
medium); (b) the two-bucket gradient all-reduce; (c) every remaining tuning knob at every non-default value against the
reference goldens (the knob surface was halved - 61 + 12 environment switches -> 24 + 5 - and what is
left is pinned here).  Everything goes through the C ABI."""
import pytest
import torch as th

from tests.cases import _golden_sampler
from tests.dp import run_ranks
from tests.util import KNOB_DEFAULTS, Golden, library_knobs, model_spec
from tests.util import run_update as _run

pytestmark = pytest.mark.gpu


def test_direct_engine_user_survives_a_knob_change_after_pack(device):
    """`eng.pack(...)` -> `engine.tune(...)` -> `eng.episode_forward(...)` used to hand the
    kernels a freshly ZEROED weights workspace (the tune epoch drops the buffer; only FusedA2C / ModelsWrapper
    re-packed).  The engine now remembers what it packed and packs again by itself; an engine that never packed
    fails loudly instead of running on zeros."""
    from marlclassification_amd import engine as E

    g = Golden("g4_resisc_b2")
    params = {k: v.to(device) for k, v in g.params.items()}
    eng = E.HipEngine(model_spec(g.cfg), device)
    eng.configure(g.na, g.nb, g.ns, g.img.shape[1:])
    eng.pack(params)
    ref_out, ref_grads = _run(eng, g, device, g.nb)
    try:
        E.tune("g3_safe", 0)  # a non-layout knob: same value, new tune epoch -> the workspace is dropped
        gen = eng.weights_generation
        out, grads = _run(eng, g, device, g.nb)
        assert eng.weights_generation == gen + 1  # (it WAS re-allocated, and re-packed behind the caller's back)
        for name in ("step_pos", "step_actions", "step_preds", "step_log_probas", "step_values"):
            assert th.equal(getattr(out, name), getattr(ref_out, name)), name
        for k in grads:
            assert th.equal(grads[k], ref_grads[k]), k
        E.tune("g3", 0)  # a layout knob between forward and backward-less calls: other kernels, same numbers
        out2, _ = _run(eng, g, device, g.nb)
        assert th.equal(out2.step_pos, ref_out.step_pos)
        assert (out2.step_preds - ref_out.step_preds).abs().max().item() <= 2e-5
    finally:
        E.tune("g3", 1)
    fresh = E.HipEngine(model_spec(g.cfg), device)
    fresh.configure(g.na, g.nb, g.ns, g.img.shape[1:])
    with pytest.raises(RuntimeError, match="no weights packed"):
        _run(fresh, g, device, g.nb)


def _dp_bucket_worker(rank, world, port, bucketed, out_q):
    import os

    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from marlclassification_amd.fused import EpisodeDraws
    from marlclassification_amd.parallel import BucketedGradAllReduce, GradAllReduce, broadcast_parameters, shard_bounds
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
    hook = BucketedGradAllReduce(world, None, flat.offsets, flat.numel, device) if bucketed else GradAllReduce(world)
    if bucketed:
        assert hook.split is not None and 0 < hook.split < flat.numel
    trainer = Trainer(model, g.cfg.nb_class, g.lr, g.gamma, allreduce=hook)
    for _ in range(2):  # (two steps: the event is re-recorded, the side stream is re-joined)
        trainer.train_step(g.img[lo:hi], g.y[lo:hi], sampler)
    th.cuda.synchronize()
    if rank == 0:
        out_q.put((model.flat_state().params.cpu().numpy(), model.flat_state().grads.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_bucket_allreduce_gives_the_one_bucket_update(device):
    """the heads' gradient slice is all-reduced on a side stream from the event the library
    records ahead of the reverse loop (marl_backward_heads_event), the rest behind the backward pass - two HIP
    Trainer processes over gloo: parameters and summed gradients after two steps are BIT-equal to the single
    all-reduce of the flat buffer."""
    res = {bucketed: run_ranks(_dp_bucket_worker, 2, bucketed)[0] for bucketed in (False, True)}
    import numpy as np

    assert np.array_equal(res[False][0], res[True][0]), "parameters differ"
    assert np.array_equal(res[False][1], res[True][1]), "summed gradients differ"


# ---- (c) the knob surface: every remaining knob, every non-default value, against the REFERENCE goldens ------------
# (forced tile plans that need a shape the fixture does not have still run: the launchers clamp; what is checked is that
# the numbers stay the reference's whatever family / plan / dispatch order produced them)
KNOB_CASES = [("g3", 0), ("g3_lstm", 0), ("g3_tn", 0), ("g3_tn", 2), ("g3_min_units", 128), ("g3_safe", 1), ("mfma_split", 0),
              ("g3_lstm_variant", 1), ("g3_lstm_variant", 2), ("g3_lstm_variant", 3), ("g3_lstm_variant", 4),
              ("g3_lstm_variant", 5), ("g3_lstm_variant", 6),
              ("g3_nt_variant", 1), ("g3_nt_variant", 2), ("g3_nt_variant", 3), ("g3_nt_variant", 7), ("g3_nt_variant", 11),
              ("g3_nt_variant", 12), ("g3_nt_variant", 21), ("g3_nt_variant", 22),
              ("g3_tn_variant", 1), ("g3_tn_variant", 2), ("g3_tn_variant", 3), ("g3_tn_variant", 4),
              ("g3_tn_cell", 0), ("g3_tn_pipe", 0), ("g3_tn_wgs", 64), ("nt_xcd", 0), ("tn_xcd", 0), ("panel_chain", 0),
              ("red_defer", 0), ("red_defer", 1), ("red_defer", 2), ("tn_split_waves", 4), ("wgrad3", 0), ("cnn_fwd2", 0),
              ("cnn_fwd3", 0), ("dgrad_wgs", 5), ("dgrad_min_chunks", 1)]


@pytest.mark.parametrize("knob,value", KNOB_CASES, ids=[f"{k}={v}" for k, v in KNOB_CASES])
def test_every_knob_value_keeps_reference_parity(device, knob, value):
    """G2 (MNIST C1: 64-unit cells, the fp32-operand / small-shape families) and G4 (RESISC45 dims: the image kernels)
    with ONE knob moved off its default: positions / actions bit-exact, logits / log-probs / values 1e-5, loss
    scalars, every gradient 1e-4 of its tensor's scale, the Adam update - the checks of tests/test_gpu_episode.py."""
    from marlclassification_amd import engine as E
    from tests import episode_checks as E0

    assert set(k for k, _ in KNOB_CASES) <= set(KNOB_DEFAULTS)
    try:
        E.tune(knob, value)
        if knob == "g3_tn_variant":  # (the row-contraction plans only run where the image weight gradients do)
            E.tune("g3_tn", 2)
        for tag in ("g2_mnist_c1", "g4_resisc_b2"):
            E0.rollout_matches_reference(device, tag, True)
        E0.backward_and_adam_match_reference(device, "g2_mnist_c1")
        E0.backward_resisc_dims_gradient_samples(device)
    finally:
        E.tune(knob, KNOB_DEFAULTS[knob])
        E.tune("g3_tn", 1)


def test_knob_table_matches_the_library_sources():
    """the cases above cover every knob the library reads (a new tune_get() must come with its parity case), and the
    table marl_tune accepts keys from (csrc/rowops.hip, kKnownKnobs) is exactly that set: three lists, one content"""
    found, table = library_knobs()
    debug_only = {"g3_clk", "g3_tn_abl"}  # read in MARL_G3_ABLATE builds only
    assert found - debug_only == set(KNOB_DEFAULTS), (found - debug_only) ^ set(KNOB_DEFAULTS)
    assert len(table) == len(set(table)) and set(table) == found, set(table) ^ found
