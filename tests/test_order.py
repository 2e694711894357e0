"""Order statistics without a GPU: the identities of the float64 definition (tests/order_reference.py), `OrderScores`, the
argument checks of the binding, and the wiring of `ScoredStore(order=...)` and of the rollout results."""
import warnings

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, rollout, verification
from gencast_flax_nnx_amd.verification import EnsembleScores, OrderScores
from tests import order_reference as R
from tests.helpers import RecordingHandle

PROBS = (0.0, 0.1, 0.5, 0.9, 1.0)


def _data(M, G=60, B=2, C=3, seed=0, ties=True):
  rng = np.random.default_rng(seed)
  scale = np.logspace(-2, 3, C)
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  if ties:
    members[1, :10] = members[0, :10]
    truth[10:20] = members[M - 1, 10:20]
    truth[20:25] = (members.max(0) + scale.astype(np.float32))[20:25]          # outliers on both sides
    truth[25:30] = (members.min(0) - scale.astype(np.float32))[25:30]
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  return members, truth, w


def _scores(M, seed=0, probs=PROBS, **kw):
  members, truth, w = _data(M, seed=seed, **kw)
  ref = R.reference(members, truth, w, probs)
  return OrderScores(ref["bins"], ref["extra"], ref["pinball"], ref["counts"], M, probs), ref, (members, truth, w)


# ---- the reference's identities -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 8, 33, 50, 64])
def test_reliability_plus_potential_is_the_ensemble_crps_and_the_pairwise_form(M):
  sc, ref, (members, truth, w) = _scores(M, seed=M)
  want = R.scores(ref, M)
  np.testing.assert_allclose(want["reliability"] + want["crps_potential"], want["crps_ensemble"], rtol=1e-9, atol=0.0)
  np.testing.assert_allclose(want["crps_ensemble"], R.crps_pairwise(members, truth, w), rtol=1e-9, atol=0.0)
  for name in ("reliability", "crps_potential", "crps_ensemble", "bin_width", "bin_frequency"):
    np.testing.assert_allclose(getattr(sc, name), want[name], rtol=1e-12, atol=0.0, err_msg=name)
  np.testing.assert_allclose(sc.reliability + sc.crps_potential, sc.crps_ensemble, rtol=1e-9, atol=0.0)
  assert np.all(sc.reliability >= 0.0) and np.all(sc.crps_potential >= 0.0)


@pytest.mark.parametrize("M", [2, 3, 8, 50])
def test_probabilities_zero_and_one_give_the_minimum_and_the_maximum(M):
  members, _, _ = _data(M, seed=3)
  members[0, 7, 1, 2] = np.nan
  f = R.quantile_fields(members, (0.0, 0.5, 1.0))
  ok = np.isfinite(members).all(0)
  np.testing.assert_array_equal(f[0][ok], members.min(0)[ok])
  np.testing.assert_array_equal(f[2][ok], members.max(0)[ok])
  assert np.isnan(f[:, 7, 1, 2]).all() and np.isfinite(f[:, ok]).all()
  lo, hi, frac = R.plan((0.0, 0.5, 1.0), M)
  assert (lo[0], hi[0], frac[0]) == (0, min(1, M - 1), 0.0) and (lo[2], hi[2], frac[2]) == (M - 1, M - 1, 0.0)
  # the median against NumPy's own rule, computed in double
  np.testing.assert_array_equal(f[1][ok], np.quantile(members.astype(np.float64), 0.5, axis=0)[ok].astype(np.float32))


def test_the_reference_counts_what_the_definition_counts():
  members, truth, w = _data(8, seed=5)
  truth[40] = np.nan
  members[2, 41, 0, 1] = np.inf
  ref = R.reference(members, truth, w, (0.5,))
  assert ref["invalid"] == 2 * 3 + 1
  np.testing.assert_array_equal(ref["counts"][..., -1].sum(), 60 * 6 - 7)
  assert np.isnan(ref["fields"][0, 41, 0, 1]) and np.isfinite(ref["fields"][0, 40]).all()


# ---- OrderScores ------------------------------------------------------------------------------------------------------------
def test_merge_is_additive_and_checks_its_parts():
  a, _, _ = _scores(8, seed=1)
  b, _, _ = _scores(8, seed=2)
  m = OrderScores.merge([a, b])
  for name in ("bins", "extra", "pinball", "counts"):
    np.testing.assert_array_equal(getattr(m, name), getattr(a, name) + getattr(b, name))
  assert m.n_members == 8 and m.probs == PROBS
  # the same points in two halves give the sums of the whole, up to the order of addition
  members, truth, w = _data(8, seed=4)
  whole = R.reference(members, truth, w, PROBS)
  parts = [R.reference(members[:, s], truth[s], w[s], PROBS) for s in (slice(0, 25), slice(25, None))]
  merged = OrderScores.merge([OrderScores(p["bins"], p["extra"], p["pinball"], p["counts"], 8, PROBS) for p in parts])
  np.testing.assert_allclose(merged.bins, whole["bins"], rtol=1e-12, atol=1e-300)
  np.testing.assert_array_equal(merged.counts, whole["counts"])
  with pytest.raises(ValueError, match="differ"):
    OrderScores.merge([a, _scores(3, seed=1)[0]])
  with pytest.raises(ValueError, match="differ"):
    OrderScores.merge([a, _scores(8, seed=1, probs=(0.5,))[0]])
  with pytest.raises(ValueError, match="nothing"):
    OrderScores.merge([])


def test_scaled_is_linear():
  M = 8
  members, truth, w = _data(M, seed=6, ties=False)
  a = np.array([0.5, 4.0, 1024.0])                              # powers of two: the scaled inputs are exact
  b = np.float32(3.0)
  base = R.reference(members, truth, w, PROBS)
  moved = R.reference(members * a.astype(np.float32), truth * a.astype(np.float32), w, PROBS)
  sc = OrderScores(base["bins"], base["extra"], base["pinball"], base["counts"], M, PROBS).scaled(a)
  np.testing.assert_allclose(sc.bins, moved["bins"], rtol=1e-13, atol=0.0)
  np.testing.assert_allclose(sc.pinball, moved["pinball"], rtol=1e-13, atol=0.0)
  np.testing.assert_array_equal(sc.extra, moved["extra"])
  np.testing.assert_array_equal(sc.counts, moved["counts"])
  np.testing.assert_allclose(sc.crps_ensemble, a[None] * OrderScores(base["bins"], base["extra"], base["pinball"],
                                                                    base["counts"], M, PROBS).crps_ensemble, rtol=1e-13)
  del b
  for bad in ([1.0, 2.0], [1.0, 0.0, 1.0], [1.0, -1.0, 1.0], [1.0, np.nan, 1.0]):
    with pytest.raises(ValueError):
      sc.scaled(bad)


def test_per_variable_splits_the_channels():
  from gencast_flax_nnx_amd import datasets
  sc, _, _ = _scores(8, seed=7)
  dims = ("batch", "time", "level", "lat", "lon")
  template = datasets.Dataset({"a": datasets.Variable(dims, np.zeros((2, 1, 2, 4, 5), np.float32)),
                               "b": datasets.Variable(("batch", "time", "lat", "lon"), np.zeros((2, 1, 4, 5), np.float32))},
                              {"lat": np.linspace(-90, 90, 4), "lon": np.arange(5) * 72.0, "level": np.array([500, 850])})
  out = sc.per_variable(template)
  assert out["reliability"]["a"].shape == (2, 2) and out["reliability"]["b"].shape == (2, 1)
  assert out["bin_width"]["a"].shape == (2, 2, 9) and out["quantile_score"]["b"].shape == (2, 1, 5)
  np.testing.assert_array_equal(out["crps_ensemble"]["b"], sc.crps_ensemble[:, 2:3])
  with pytest.raises(ValueError, match="channels"):
    sc.per_variable(datasets.Dataset({"b": template["b"]}, template.coords))


def test_a_zero_width_ensemble_gives_zero_widths_and_no_nan_or_warning():
  M, G = 8, 40
  x = (np.rint(np.random.default_rng(9).standard_normal((G, 2, 3)) * 8.0) / 8.0).astype(np.float32)   # x + 1 is exact
  members = np.broadcast_to(x, (M, G, 2, 3)).copy()
  truth = x.copy()
  truth[:10] += np.float32(1.0)
  w = np.ones(G, np.float32)
  ref = R.reference(members, truth, w, (0.5,))
  sc = OrderScores(ref["bins"], ref["extra"], ref["pinball"], ref["counts"], M, (0.5,))
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    g, o = sc.bin_width, sc.bin_frequency
    rel, pot, crps = sc.reliability, sc.crps_potential, sc.crps_ensemble
    cov, qs = sc.quantile_coverage, sc.quantile_score
  assert not g[..., 1:M].any() and not g[..., 0].any()            # no interior width, nothing below the members
  assert np.all(g[..., M] == 1.0)                                 # an outlier above lies 1.0 away on average
  for v in (g, o, rel, pot, crps, cov, qs):
    assert np.isfinite(v).all()
  np.testing.assert_allclose(rel + pot, crps, rtol=1e-12)
  np.testing.assert_allclose(crps, 0.25, rtol=1e-12)              # 10 of 40 points, |y - x| = 1


def test_constructor_checks_shapes():
  sc, ref, _ = _scores(8, seed=1)
  with pytest.raises(ValueError, match="bins"):
    OrderScores(ref["bins"], ref["extra"], ref["pinball"], ref["counts"], 9, PROBS)
  with pytest.raises(ValueError, match="extra"):
    OrderScores(ref["bins"], ref["extra"][..., :2], ref["pinball"], ref["counts"], 8, PROBS)
  with pytest.raises(ValueError, match="pinball"):
    OrderScores(ref["bins"], ref["extra"], ref["pinball"], ref["counts"], 8, PROBS[:2])
  with pytest.raises(ValueError, match="n_members"):
    OrderScores(ref["bins"][:, :, :2], ref["extra"], ref["pinball"], ref["counts"], 1, PROBS)
  np.testing.assert_array_equal(sc.valid_points, ref["counts"][..., -1])
  np.testing.assert_allclose(sc.outlier_low + sc.outlier_high, (ref["extra"][..., 1] + ref["extra"][..., 2]) / ref["extra"][..., 0])


# ---- the binding's own checks: before the C call, so without a device -------------------------------------------------------
class _NoCall:
  def __getattr__(self, name):
    raise AssertionError(f"{name} must not be reached")


def _bare_binding():
  nd = object.__new__(_lib.NativeDenoiser)
  nd._lib, nd._h = _NoCall(), None
  nd.cfg = _lib.GcConfig(128, 128, 2, 256, 1, 10, 6, 2, 32, 32, 16.0)
  nd.num_grid_nodes, nd._ens_members, nd._order_quantiles = 312, 0, None
  return nd


def test_binding_rejects_bad_probabilities_before_the_c_call():
  nd = _bare_binding()
  for bad in ([0.5, np.nan], [-0.1], [1.01], np.zeros(9), np.zeros((2, 2)), [np.inf]):
    with pytest.raises(ValueError):
      nd.ens_order_set(bad)
  with pytest.raises(_lib.GencastHipError, match="ens_order_set"):
    nd.ens_order_score(None)
  with pytest.raises(_lib.GencastHipError, match="ens_order_set"):
    nd.ens_order_fields()
  with pytest.raises(_lib.GencastHipError, match="ens_order_set"):
    nd.ens_order_quantile(0)
  nd._order_quantiles = 2
  with pytest.raises(_lib.GencastHipError, match="ens_reserve"):
    nd.ens_order_score(None)
  nd._ens_members = 8
  with pytest.raises(ValueError, match="truth must be"):
    nd.ens_order_score(np.zeros((312, 2, 5), np.float32))


# ---- ScoredStore(order=...) with a handle that records ----------------------------------------------------------------------
def test_scored_store_sets_the_probabilities_and_scores_the_order():
  h = RecordingHandle("h", [], M=8)
  st = verification.ScoredStore(h, 8, np.ones(4, np.float32), order=[0.1, 0.9])
  st.setup()
  assert h.calls == [("h", "reserve", 8), ("h", "weight"), ("h", "order_set", (0.1, 0.9))]
  out = st.score_order("truth")
  assert isinstance(out, OrderScores) and out.n_members == 8 and out.probs == (0.1, 0.9)
  assert h.calls[-1] == ("h", "order_score", False)
  assert [f[0, 0, 0] for f in st.quantile_fields()] == [0.0, 1.0]
  # without `order` nothing of it is touched
  h2 = RecordingHandle("h2", [], M=8)
  plain = verification.ScoredStore(h2, 8, np.ones(4, np.float32))
  plain.setup()
  assert plain.score_order(None) is None and plain.order is None
  assert all(c[1] not in ("order_set", "order_score") for c in h2.calls)
  # set per score: the setting is made again by every scoring call, not by setup
  h3 = RecordingHandle("h3", [], M=8)
  per = verification.ScoredStore(h3, 8, np.ones(4, np.float32), order=(), set_per_score=True)
  per.setup()
  assert ("h3", "order_set", ()) not in h3.calls
  assert per.score_order(None).pinball.shape == (2, 3, 0)
  assert h3.calls[-2:] == [("h3", "order_set", ()), ("h3", "order_score", True)]
  # a derived view: filled by `score`, then sorted on the truth already there
  h4 = RecordingHandle("h4", [], M=8)
  view = verification.ScoredStore(h4, 8, np.ones(4, np.float32), plan={"op": [0]}, source=object(), order=(0.5,))
  view.setup()
  view.score("source truth")
  view.score_order(None)
  assert [c[1] for c in h4.calls] == ["reserve", "weight", "derive_set", "order_set", "derive", "score", "order_score"]
  assert h4.calls[-1] == ("h4", "order_score", True)


# ---- rollout results --------------------------------------------------------------------------------------------------------
def _ens(M=8, B=2, C=3, seed=0):
  rng = np.random.default_rng(seed)
  return EnsembleScores(rng.uniform(1, 2, (B, C, 6)), rng.integers(0, 9, (B, C, M + 1)).astype(np.uint64), M)


def test_rollout_results_merge_with_and_without_order():
  o = [[_scores(8, seed=10 * d + k)[0] for k in range(2)] for d in range(2)]
  with_order = [rollout.EnsembleRolloutResult([_ens(seed=k) for k in range(2)], n_members=8, order=o[d],
                                              order_normalized=o[d], quantiles=[["q"]] * 2) for d in range(2)]
  merged = with_order[0].merge(with_order[1])
  for k in range(2):
    np.testing.assert_array_equal(merged.order[k].bins, o[0][k].bins + o[1][k].bins)
    np.testing.assert_array_equal(merged.order_normalized[k].counts, o[0][k].counts + o[1][k].counts)
  assert merged.quantiles is None                                 # fields belong to one date
  without = rollout.EnsembleRolloutResult([_ens(seed=k) for k in range(2)], n_members=8)
  assert without.order is None and without.quantiles is None
  assert without.merge(without).order is None
  with pytest.raises(ValueError, match="order"):
    with_order[0].merge(without)
  with pytest.raises(ValueError, match="order"):
    without.merge(with_order[0])
  with pytest.raises(ValueError, match="lead times"):
    rollout.EnsembleRolloutResult([_ens()], n_members=8, order=o[0])
  # the derived part
  d = [rollout.DerivedRolloutResult([_ens(seed=k) for k in range(2)], [_ens(seed=k) for k in range(2)], order=o[i],
                                    order_normalized=o[i]) for i in range(2)]
  dm = d[0].merge(d[1])
  np.testing.assert_array_equal(dm.order[1].extra, o[0][1].extra + o[1][1].extra)
  plain = rollout.DerivedRolloutResult([_ens(seed=k) for k in range(2)], [_ens(seed=k) for k in range(2)])
  assert plain.merge(plain).order is None
  with pytest.raises(ValueError, match="order"):
    d[0].merge(plain)


def test_sampler_and_rollout_refuse_more_than_one_rank():
  from gencast_flax_nnx_amd import ensemble

  class _S:
    _denoiser = None
  with pytest.raises(ValueError, match="one rank"):
    ensemble.EnsembleSampler(_S(), rank=0, world_size=2).order(None, None, None, 4, (0.5,))
  with pytest.raises(ValueError, match="one rank"):
    rollout.EnsembleRollout(None, world_size=2).run(None, None, None, 2, 4, order=(0.5,))
