"""GPU: oracle parity on DISTINCT shuffled images at the row counts where the row-gated CNN plans engage.  Every other
oracle comparison of the model shapes below runs at R <= 192 rows, where launch_cnn_fwd takes one patch per workgroup,
the cnn_fwd2 grid never walks and the layer backward is single-patch: a wrong multi-patch LDS offset, a cross-image read
in a persistent walk or a ragged last chunk would ship green.  Each case first asserts - from marl_plan_query, i.e. from
the launchers' own plan routines - that it really is on the plan it is there for (tests/util.py: PLAN_CASES,
PLAN_WITNESS), then runs tests/util.py::distinct_image_parity, the method and tolerances of
tests/test_gpu_round5.py::test_full_size_parity_on_distinct_shuffled_images.

The inputs (uniform_params seed 7; image / label / draw seeds 21 / 22 / 23) keep the REFERENCE well inside the
tolerances: the fp32 oracle against a float64 run of its own step loop (tests/cases.py::_oracle_loop,
teacher-forced to the fp32 oracle's actions; positions identical, |logit| <= 2.4) differs by at most
                        logits    log-probs  values
  mnist6_b1024          1.00e-06  7.41e-07   5.85e-07
  mnist12_odd_ragged    8.94e-07  3.60e-07   4.93e-07
  mnist10_general       6.83e-07  5.49e-07   6.31e-07
  resisc16_general      1.39e-06  8.43e-07   7.48e-07
  resisc16_general_g3   1.68e-06  1.19e-06   8.76e-07
  worldstrat16          1.03e-06  6.84e-07   7.60e-07
  c3_partial_batch      1.92e-06  1.17e-06   9.76e-07
  ckpt768_b64           1.57e-06  7.95e-07   1.02e-06
- every case within ATOL / 4 = 2.5e-6 on all three outputs (the condition a changed case has to meet again)."""
import pytest

from tests.util import PLAN_CASES, PLAN_INVARIANTS, PLAN_WITNESS, assert_witness, distinct_image_parity, plan_witness

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", list(PLAN_CASES))
def test_distinct_image_parity_where_the_row_gated_plans_engage(device, tag):
    cfg, na, nd, rep, ns, shape = PLAN_CASES[tag]
    w = plan_witness(cfg, na, nd * rep, ns, shape)
    assert_witness(w, PLAN_WITNESS[tag] + PLAN_INVARIANTS)
    distinct_image_parity(device, cfg, na, nd, ns, shape, rep, f"plan_coverage_{tag}",
                          extra={"witness": w, "asserted": PLAN_WITNESS[tag]})
