"""The case table of the sampler-loop tests (tests/sampler_cases.py), checked with the oracle alone: every row makes the
calls and draws it says, `multi` and `graph_eligible` follow from them by the library's rules, every branch the module
lists is reached, and every row has a finite float64 answer -- so a failure of tests/test_gpu_sampler_cases.py is the
loop's."""
import numpy as np
import pytest

from oracle import gencast_oracle as O
from tests import sampler_cases as SC

IDS = [c.id for c in SC.CASES]


@pytest.mark.parametrize("case_id", IDS)
def test_row_counts_and_result(case_id):
  case = SC.BY_ID[case_id]
  out, calls, draws = SC.reference(case)
  assert (calls, draws) == (case.calls, case.draws)
  assert SC.trace(case)[:2] == (case.calls, case.draws)                    # the restated control flow counts the same
  assert case.multi == (calls <= SC.MAX_SIGMA_LIST)
  churned = case.rates is not None and any(r > 0 for r in case.rates)
  assert draws == (sum(r > 0 for r in case.rates) if churned else 0)
  assert case.graph_eligible == (case.multi and not churned)
  G, B = SC.setup(case.setup)[3].shape[:2]
  assert out.shape == (G, B, SC.setup(case.setup)[1].c_out) and out.dtype == np.float64 and np.isfinite(out).all()
  print(f"{case_id}: calls {calls}, draws {draws}, max |ref| {np.abs(out).max():.4g}")


@pytest.mark.parametrize("case_id", IDS)
def test_row_reaches_what_it_says(case_id):
  case = SC.BY_ID[case_id]
  taken = SC.trace(case)[2]
  assert case.reaches and set(case.reaches) <= set(SC.BRANCHES)
  assert set(case.reaches) <= taken, (case_id, sorted(set(case.reaches) - taken))


def test_the_table_covers_every_branch_and_the_rows_the_schedules_demand():
  reached = set().union(*(SC.trace(c)[2] for c in SC.CASES))
  assert reached == set(SC.BRANCHES)
  named = set().union(*(c.reaches for c in SC.CASES))
  assert named == set(SC.BRANCHES)                                           # and some row is there FOR each of them
  for c in SC.CASES:
    sig = np.asarray(c.sigmas)
    assert (sig[:-1] > 0).all() and (np.diff(sig) < 0).all() and sig[-1] >= 0   # what gc_sample_resident accepts
    assert c.rates is None or len(c.rates) == c.n
    assert c.setup in SC.SETUPS
  by = SC.BY_ID
  assert by["calls_96"].calls == SC.MAX_SIGMA_LIST and by["calls_97"].calls == SC.MAX_SIGMA_LIST + 1
  assert by["calls_96"].graph_eligible and not by["calls_97"].multi
  assert by["no_trailing_zero"].sigmas[-1] > 0 and by["one_step_live"].sigmas[-1] > 0
  assert 0 < by["below_clamp"].sigmas[1] < SC.CLAMP
  assert by["churn_97"].draws == 3 and by["churn_zero_rates"].graph_eligible


def test_zero_rates_and_the_dead_call_leave_the_sample_alone():
  """All-zero rates are the plain sampler bit for bit, and the dead call is discarded: the oracle says so too."""
  plain = SC.sample_oracle(SC.plain("T", SC.SIX))[0]
  np.testing.assert_array_equal(SC.reference(SC.BY_ID["churn_zero_rates"])[0], plain)
  np.testing.assert_array_equal(SC.reference(SC.BY_ID["one_step_skip"])[0], SC.reference(SC.BY_ID["one_step_dead"])[0])
  assert np.abs(SC.reference(SC.BY_ID["churn_all"])[0] - plain).max() > 1e-2    # churn does change the trajectory


def test_the_fields_are_the_streams_of_one_key():
  """`field(setup, k)` is stream k of SEED: distinct per stream, unit variance, and a row started at another stream draws
  other fields."""
  f0, f1 = SC.field("T", 0), SC.field("T", 1)
  assert f0.shape == SC.setup("T")[7].shape and not np.array_equal(f0, f1)
  assert abs(float((f0 ** 2).mean()) - 1.0) < 0.1
  case = SC.BY_ID["churn_first"]
  a = SC.sample_oracle(case, stream0=0)[0]
  np.testing.assert_array_equal(a, SC.reference(case)[0])
  assert np.abs(SC.sample_oracle(case, stream0=1)[0] - a).max() > 1e-3
  assert O.noise_schedule(80.0, 0.03, 6, 7.0)[-1] == 0.0


def test_plain_samples_outside_the_table_count_as_the_oracle_does():
  for sigmas, skip_dead in ((SC.SIX, True), (SC.SIX, False), (SC.karras(1), True), (SC.SIX[:-1], True)):
    case = SC.plain("T", sigmas, skip_dead)
    assert case.calls == SC.sample_oracle(case)[1] and case.draws == 0 and not case.reaches
    assert case.multi and case.graph_eligible and case.id not in SC.BY_ID
  long = SC.plain("S", SC.karras(49))
  assert long.calls == 97 and not long.multi and not long.graph_eligible
