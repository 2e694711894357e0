"""Order statistics through the sampler and the ensemble rollout (EnsembleRollout.run(order=...), GenCast.ensemble_order;
DESIGN.md section 8h) against the float64 definition (tests/order_reference.py) on the members the device itself kept.
Quantile fields ==, sums within (G + 8) 2^-53 sum|term|, counts ==.  Size: the tiny model of
tests/test_gpu_ensemble_rollout.py (9 x 16 grid, G = 144, batch 2, 82 channels), horizon 2, M = 3."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import EnsembleSampler, rollout, verification
from tests import order_reference as R
from tests.test_gpu_ensemble_rollout import _Setup, B, C
from tests.test_gpu_order import _check
from tests.test_gpu_verification import _small_model, _stack

pytestmark = pytest.mark.gpu

HORIZON, M = 2, 3
PROBS = (0.1, 0.5, 0.9)


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  for lane in getattr(s.gc.denoiser, "_lanes", None) or []:
    lane.close()
  s.gc.denoiser.native.close()


@pytest.fixture(scope="module")
def runs(setup):
  """One run with order statistics and one without, the same members: computed once and left unchanged."""
  out = {}
  for which in ("wrapper", "none"):
    er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
    kw = dict(init_noise=setup.noises[:M], keep_members=True, spectra=True)
    plain = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, **kw)
    with_order = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, order=PROBS, keep_quantiles=True, **kw)
    out[which] = (plain, with_order)
  return out


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_order_and_quantiles_per_lead_equal_the_reference_on_the_kept_members(setup, runs, which):
  _, res = runs[which]
  w = verification.node_weights(setup.template0)
  scale, _ = setup.stats_per_channel(which)
  assert len(res.order) == len(res.order_normalized) == len(res.quantiles) == HORIZON
  for k in range(HORIZON):
    members = np.stack(res.members[k])
    ref = R.reference(members, setup.truth(setup.targets, k, which), w, PROBS)
    raw = res.order_normalized[k]
    assert raw.n_members == M and raw.probs == PROBS
    _check(f"{which} lead {k}", (raw.bins, raw.extra, raw.pinball, raw.counts, ref["invalid"]), ref, setup.G)
    assert len(res.quantiles[k]) == len(PROBS)
    for q in range(len(PROBS)):
      np.testing.assert_array_equal(res.quantiles[k][q], ref["fields"][q], err_msg=f"{which} lead {k} quantile {q}")
    np.testing.assert_array_equal(res.quantiles[k][1], np.sort(members, axis=0)[1])      # M = 3: the median is a member
    phys = res.order[k]
    np.testing.assert_array_equal(phys.bins, raw.bins * scale[None, :, None, None])
    np.testing.assert_array_equal(phys.pinball, raw.pinball * scale[None, :, None])
    np.testing.assert_array_equal(phys.counts, raw.counts)
    np.testing.assert_allclose(phys.crps_ensemble, res.scores[k].crps_ensemble, rtol=1e-9, atol=0.0)
    np.testing.assert_allclose(phys.reliability + phys.crps_potential, phys.crps_ensemble, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_a_run_without_order_is_byte_identical(runs, which):
  plain, res = runs[which]
  assert plain.order is None and plain.order_normalized is None and plain.quantiles is None
  for k in range(HORIZON):
    for a, b in ((plain.scores[k], res.scores[k]), (plain.scores_normalized[k], res.scores_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes() and a.rank_histogram.tobytes() == b.rank_histogram.tobytes()
    for a, b in ((plain.spectra[k], res.spectra[k]), (plain.spectra_normalized[k], res.spectra_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes()
    for m in range(M):
      assert plain.members[k][m].tobytes() == res.members[k][m].tobytes()
  merged = res.merge(res)
  np.testing.assert_array_equal(merged.order[0].bins, 2.0 * res.order[0].bins)
  with pytest.raises(ValueError, match="order"):
    res.merge(plain)


def test_derived_entries_carry_their_own_order_statistics(setup):
  spec = verification.DerivedSpec([("norm2", "wind10", "10m_u_component_of_wind", "10m_v_component_of_wind")])
  er = rollout.EnsembleRollout(setup.gc, setup.norm("wrapper"))
  res = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, init_noise=setup.noises[:M], keep_members=True,
               derived={"wind": spec}, order=(0.5,), keep_quantiles=True)
  d = res.derived["wind"]
  w = verification.node_weights(setup.template0)
  assert len(d.order) == len(d.quantiles) == HORIZON
  for k in range(HORIZON):
    members = np.stack(d.members[k])                              # the device's own derived members
    raw = d.order_normalized[k]
    assert raw.bins.shape == (B, 1, M + 1, 2)
    for q, f in enumerate(d.quantiles[k]):
      np.testing.assert_array_equal(f, R.quantile_fields(members, (0.5,))[q])
    np.testing.assert_allclose(raw.crps_ensemble, d.scores_normalized[k].crps_ensemble, rtol=1e-9, atol=0.0)
    np.testing.assert_array_equal(raw.counts[..., -1], d.scores_normalized[k].rank_histogram.sum(-1))
    assert np.all(np.abs(raw.extra[..., 0] - w.astype(np.float64).sum()) <= (setup.G + 8) * 2.0 ** -53 * w.astype(np.float64).sum())


def test_single_step_ensemble_order_equals_the_reference_on_the_samplers_own_members():
  gc, inp, tgt, frc = _small_model()
  try:
    n = 4
    ens = EnsembleSampler(gc._sampler, base_seed=5)
    fields = [_stack(d) for _, d in sorted(ens(inp, tgt.map(np.zeros_like), frc, n), key=lambda t: t[0])]
    truth, w = _stack(tgt), verification.node_weights(tgt)
    ref = R.reference(np.stack(fields), truth, w, PROBS)
    sc, qf = gc.ensemble_order(inp, tgt, frc, num_members=n, probs=PROBS, quantile_fields=True, rngs=5)
    _check("ensemble_order", (sc.bins, sc.extra, sc.pinball, sc.counts, ref["invalid"]), ref, truth.shape[0])
    assert sc.n_members == n and sc.probs == PROBS and len(qf) == len(PROBS)
    for q in range(len(PROBS)):
      np.testing.assert_array_equal(_stack(qf[q]), ref["fields"][q])
    only = gc.ensemble_order(inp, tgt, frc, num_members=n, probs=PROBS, rngs=5)
    assert only.bins.tobytes() == sc.bins.tobytes() and only.counts.tobytes() == sc.counts.tobytes()
    crps = gc.ensemble_scores(inp, tgt, frc, num_members=n, rngs=5).crps_ensemble
    np.testing.assert_allclose(sc.crps_ensemble, crps, rtol=1e-9, atol=0.0)
    with pytest.raises(ValueError, match="ens_push_host"):
      EnsembleSampler(gc._sampler, rank=0, world_size=2).order(inp, tgt, frc, n, PROBS)
  finally:
    gc.denoiser.native.close()
