"""Skill against a climatology through the ensemble rollout and the sampler (EnsembleRollout.run(climatology=...),
GenCast.ensemble_climatology) against the float64 definition (tests/clim_reference.py) on the members
the device itself kept.  Sums within (G + max(M, K)^2 + 8) 2^-53 sum|term|, counts ==.  Size: the tiny model of
tests/test_gpu_ensemble_rollout.py (9 x 16 grid, G = 144, batch 2, 82 channels), horizon 2, M = 3, K = 4."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import EnsembleSampler, datasets, rollout, verification
from gencast_flax_nnx_amd.verification import ClimatologyScores
from tests import clim_reference as R
from tests.helpers import graph_handle
from tests.test_gpu_clim import _check, _push_all
from tests.test_gpu_ensemble_rollout import _Setup, B, C
from tests.test_gpu_verification import _small_model, _stack

pytestmark = pytest.mark.gpu

HORIZON, M, K = 2, 3, 4


def _like(ds, rng, hole=None):
  """A Dataset shaped like `ds` with other values (a climatological sample); `hole`: one NaN in the first variable."""
  out = {}
  for i, (k, v) in enumerate(ds.items()):
    a = (np.asarray(v.data, np.float32) + rng.standard_normal(np.shape(v.data)).astype(np.float32))
    if hole is not None and i == 0:
      a.reshape(-1)[hole] = np.nan
    out[k] = datasets.Variable(v.dims, a)
  return datasets.Dataset(out, ds.coords)


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  rng = np.random.default_rng(17)
  # K samples per lead time, shaped like that lead's targets; one of them has a hole at lead 1
  s.climatology = [[_like(rollout.isel_time(s.targets, slice(k, k + 1)), rng, hole=5 if (k, j) == (1, 2) else None)
                    for j in range(K)] for k in range(HORIZON)]
  yield s
  s.gc.denoiser.close()


@pytest.fixture(scope="module")
def runs(setup):
  """One run with a climatology and one without, the same members: computed once and left unchanged."""
  out = {}
  for which in ("wrapper", "none"):
    er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
    kw = dict(init_noise=setup.noises[:M], keep_members=True, order=(0.5,))
    plain = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, **kw)
    with_clim = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, climatology=setup.climatology, **kw)
    out[which] = (plain, with_clim)
  return out


def _samples(setup, k, which):
  """Lead k's samples in the members' units: the map of the truth."""
  ones = [setup.truth(c, 0, which) for c in setup.climatology[k]]
  return np.stack(ones)


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_climatology_scores_per_lead_equal_the_reference_on_the_kept_members(setup, runs, which):
  _, res = runs[which]
  w = verification.node_weights(setup.template0)
  scale, _ = setup.stats_per_channel(which)
  assert len(res.climatology) == len(res.climatology_normalized) == HORIZON
  for k in range(HORIZON):
    members, clim, truth = np.stack(res.members[k]), _samples(setup, k, which), setup.truth(setup.targets, k, which)
    ref = R.reference(members, clim, truth, w)
    raw = res.climatology_normalized[k]
    assert (raw.n_members, raw.n_climatology) == (M, K) and raw.invalid == ref["invalid"]
    _check(f"{which} lead {k}", (raw.sums, raw.counts, raw.invalid), ref, setup.G)
    assert (ref["invalid"] > 0) == (k == 1)                          # the hole in a sample: points that do not count
    # a direct ens_clim_score on the downloaded members and the same samples: the same bytes
    nd, cl = graph_handle(setup.gc.denoiser.graph, B, C), graph_handle(setup.gc.denoiser.graph, B, C)
    try:
      _push_all(nd, members, w)
      _push_all(cl, clim)
      direct = nd.ens_clim_score(cl, truth)
      assert direct[0].tobytes() == raw.sums.tobytes() and direct[1].tobytes() == raw.counts.tobytes()
    finally:
      nd.close()
      cl.close()
    phys = res.climatology[k]
    np.testing.assert_array_equal(phys.sums, raw.scaled(scale).sums)
    np.testing.assert_array_equal(phys.counts, raw.counts)
    np.testing.assert_allclose(phys.acc, raw.acc, rtol=1e-12)          # a ratio of sums that scale alike
    np.testing.assert_allclose(phys.crpss, raw.crpss, rtol=1e-9, atol=1e-12)
    if k == 0:                                                       # (no invalid point: the same points as ens_score)
      np.testing.assert_allclose(phys.crps, res.scores[k].crps, rtol=1e-9, atol=0.0)
      np.testing.assert_allclose(phys.rmse, res.scores[k].rmse, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_a_run_without_climatology_is_byte_identical(runs, which):
  plain, res = runs[which]
  assert plain.climatology is None and plain.climatology_normalized is None
  for k in range(HORIZON):
    for a, b in ((plain.scores[k], res.scores[k]), (plain.scores_normalized[k], res.scores_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes() and a.rank_histogram.tobytes() == b.rank_histogram.tobytes()
    for a, b in ((plain.order[k], res.order[k]), (plain.order_normalized[k], res.order_normalized[k])):
      assert a.bins.tobytes() == b.bins.tobytes() and a.counts.tobytes() == b.counts.tobytes()
    for m in range(M):
      assert plain.members[k][m].tobytes() == res.members[k][m].tobytes()
  merged = res.merge(res)                                            # two start dates
  np.testing.assert_array_equal(merged.climatology[0].sums, 2.0 * res.climatology[0].sums)
  np.testing.assert_array_equal(merged.climatology[1].counts, 2 * res.climatology[1].counts)
  np.testing.assert_allclose(merged.climatology[0].acc, res.climatology[0].acc, rtol=1e-12)
  with pytest.raises(ValueError, match="climatology"):
    res.merge(plain)


def test_a_callable_gives_the_samples_of_a_lead_time(setup, runs):
  _, res = runs["none"]
  er = rollout.EnsembleRollout(setup.gc, None)
  again = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, init_noise=setup.noises[:M],
                 climatology=lambda k: setup.climatology[k])
  for k in range(HORIZON):
    assert again.climatology[k].sums.tobytes() == res.climatology[k].sums.tobytes()
  with pytest.raises(ValueError, match="lead times"):
    er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, init_noise=setup.noises[:M], climatology=setup.climatology[:1])


def test_a_derived_wind_speed_view_is_scored_against_the_derived_climatology(setup):
  spec = verification.DerivedSpec([("norm2", "wind10", "10m_u_component_of_wind", "10m_v_component_of_wind")])
  er = rollout.EnsembleRollout(setup.gc, setup.norm("wrapper"))
  res = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, init_noise=setup.noises[:M], keep_members=True,
               derived={"wind": spec}, climatology=setup.climatology)
  d = res.derived["wind"]
  w = verification.node_weights(setup.template0)
  assert len(d.climatology) == len(d.climatology_normalized) == HORIZON
  cview = setup.gc.denoiser.climatology_handle(1, view=True)
  for k in range(HORIZON):
    raw = d.climatology_normalized[k]
    assert raw.sums.shape == (B, 1, 12) and (raw.n_members, raw.n_climatology) == (M, K)
    # F4, F5, A7 and the counts against what ens_score made of the same derived members and truth
    s = d.scores_normalized[k]
    if k == 0:
      np.testing.assert_array_equal(raw.counts, s.rank_histogram.sum(-1))
      np.testing.assert_allclose(raw.crps, s.crps, rtol=1e-9, atol=0.0)
      np.testing.assert_allclose(raw.rmse, s.rmse, rtol=1e-9, atol=0.0)
    else:
      assert np.all(raw.counts <= s.rank_histogram.sum(-1))
    np.testing.assert_array_equal(d.climatology[k].sums, raw.scaled(np.ones(1)).sums)   # wind speed is in physical units already
  # the last lead against the definition, on the derived members and the derived samples the device kept
  k = HORIZON - 1
  members = np.stack(d.members[k])
  clim = np.stack([cview.ens_download_member(j) for j in range(K)])
  view = setup.gc.denoiser.view_handle(1)
  sums, counts, invalid = view.ens_clim_score(cview, None)
  assert sums.tobytes() == d.climatology_normalized[k].sums.tobytes()
  # the sums that do not depend on the truth (A0, A4, A6, F5, C5) against the definition, on the derived members and the
  # derived samples the device kept; those that do (F4, A7) were held against ens_score above
  ref = R.reference(members, clim, np.zeros((setup.G, B, 1), np.float32), w)
  tol = R.tolerance(ref, setup.G)
  for j in (0, 4, 6, 9, 11):
    assert np.all(np.abs(sums[..., j] - ref["sums"][..., j]) <= tol[..., j]), R.NAMES[j]
  np.testing.assert_array_equal(counts, ref["counts"])
  assert invalid == ref["invalid"]


def test_single_step_ensemble_climatology_equals_the_reference_on_the_samplers_own_members():
  gc, inp, tgt, frc = _small_model()
  try:
    n, rng = 4, np.random.default_rng(23)
    clim = [_like(tgt, rng, hole=7 if j == 1 else None) for j in range(K)]
    ens = EnsembleSampler(gc._sampler, base_seed=5)
    fields = [_stack(d) for _, d in sorted(ens(inp, tgt.map(np.zeros_like), frc, n), key=lambda t: t[0])]
    truth, w = _stack(tgt), verification.node_weights(tgt)
    ref = R.reference(np.stack(fields), np.stack([_stack(c) for c in clim]), truth, w)
    sc = gc.ensemble_climatology(inp, tgt, frc, num_members=n, climatology=clim, rngs=5)
    assert isinstance(sc, ClimatologyScores) and (sc.n_members, sc.n_climatology) == (n, K) and sc.invalid == 1
    _check("ensemble_climatology", (sc.sums, sc.counts, sc.invalid), ref, truth.shape[0])
    with pytest.raises(ValueError, match="ens_push_host"):
      EnsembleSampler(gc._sampler, rank=0, world_size=2).climatology(inp, tgt, frc, n, clim)
  finally:
    gc.denoiser.close()
