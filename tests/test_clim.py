"""Skill against a climatology without a GPU: `ClimatologyScores` on sums made by the float64 definition
(tests/clim_reference.py), the two forms of the mean absolute difference, the argument checks of the binding, and the wiring
of `ScoredStore(climatology=...)` and of the rollout results."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, datasets, rollout, verification
from gencast_flax_nnx_amd.verification import ClimatologyScores, EnsembleScores
from tests import clim_reference as R
from tests.helpers import RecordingHandle


def _data(M, K, G=60, B=2, C=3, seed=0, offset=0.0):
  rng = np.random.default_rng(seed)
  scale = np.logspace(-1, 2, C)
  clim = (offset + rng.standard_normal((K, G, B, C)) * scale).astype(np.float32)
  truth = (offset + rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  members = (truth + 0.5 * rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  return members, clim, truth, w


def _scores(ref):
  return ClimatologyScores(ref["sums"], ref["counts"], ref["n_members"], ref["n_climatology"], ref["invalid"])


# ---- ClimatologyScores on sums of the definition ----------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(2, 2), (8, 3), (5, 33)])
def test_derived_scores_are_the_written_out_formulas(M, K):
  members, clim, truth, w = _data(M, K, seed=M + K)
  truth[3, 1, 2] = np.nan
  clim[1, 4, 0, 0] = np.inf
  ref = R.reference(members, clim, truth, w)
  sc, want = _scores(ref), R.scores(ref)
  for name, v in want.items():
    np.testing.assert_allclose(getattr(sc, name), v, rtol=1e-13, atol=0.0, err_msg=name)
  np.testing.assert_array_equal(sc.valid_weight, ref["sums"][..., 0])
  np.testing.assert_array_equal(sc.valid_points, ref["counts"])
  assert sc.invalid == 2 and int(sc.valid_points.sum()) == truth.size - 2
  assert np.all(sc.acc > 0.5) and np.all(sc.acc <= 1.0) and np.all(sc.crpss > 0.0) and np.all(sc.msss > 0.0)
  assert np.all(sc.acc_members <= sc.acc + 1e-12)           # A6 >= A4: the mean of squares is no less than the square of the mean
  # the fair forms are what EnsembleScores makes of S4, S5 on the same members
  np.testing.assert_allclose(sc.crps, (ref["sums"][..., 8] - 0.5 * ref["sums"][..., 9]) / ref["sums"][..., 0], rtol=1e-15)


def test_a_perfect_forecast_has_unit_skill():
  M, K = 4, 6
  _, clim, truth, w = _data(M, K, seed=1)
  members = np.broadcast_to(truth, (M,) + truth.shape).copy()
  sc = _scores(R.reference(members, clim, truth, w))
  np.testing.assert_array_equal(sc.acc, 1.0)
  np.testing.assert_array_equal(sc.msss, 1.0)
  np.testing.assert_array_equal(sc.crpss, 1.0)
  np.testing.assert_array_equal(sc.crps, 0.0)
  np.testing.assert_array_equal(sc.rmse, 0.0)
  assert np.all(sc.crps_climatology > 0.0) and np.all(sc.rmse_climatology > 0.0)


def test_the_climatology_as_the_forecast_has_no_skill():
  K = 7
  _, clim, truth, w = _data(K, K, seed=2)
  sc = _scores(R.reference(clim.copy(), clim, truth, w))
  np.testing.assert_array_equal(sc.crpss, 0.0)              # F4 == C4 and F5 == C5, bit for bit
  np.testing.assert_array_equal(sc.crpss_ensemble, 0.0)
  assert np.isnan(sc.acc).all() and np.isnan(sc.acc_members[..., :0]).size == 0     # fa == 0 at every point: 0 / 0
  assert np.isnan(sc.acc_centred).all()
  np.testing.assert_array_equal(sc.sums[..., 1], 0.0)
  np.testing.assert_array_equal(sc.sums[..., 4], 0.0)
  np.testing.assert_array_equal(sc.msss, 0.0)               # (m - y)^2 == (cbar - y)^2


def test_zero_denominators_give_nan_not_an_error():
  sc = ClimatologyScores(np.zeros((1, 2, 12)), np.zeros((1, 2), np.uint64), 4, 4, 9)
  for name in ("acc", "acc_centred", "acc_members", "crps", "crps_climatology", "crpss", "msss", "rmse", "rmse_climatology"):
    assert np.isnan(getattr(sc, name)).all(), name
  with pytest.raises(ValueError, match=">= 2"):
    ClimatologyScores(np.zeros((1, 2, 12)), np.zeros((1, 2), np.uint64), 1, 4)
  with pytest.raises(ValueError, match="sums must be"):
    ClimatologyScores(np.zeros((1, 2, 6)), np.zeros((1, 2), np.uint64), 4, 4)
  with pytest.raises(ValueError, match="counts must be"):
    ClimatologyScores(np.zeros((1, 2, 12)), np.zeros((2, 2), np.uint64), 4, 4)


def test_merge_is_scoring_the_concatenation():
  M, K = 5, 4
  members, clim, truth, w = _data(M, K, G=80, seed=3)
  truth[50, 0, 1] = np.nan
  whole = R.reference(members, clim, truth, w)
  parts = [R.reference(members[:, a:b], clim[:, a:b], truth[a:b], w[a:b]) for a, b in ((0, 30), (30, 80))]
  merged = ClimatologyScores.merge([_scores(p) for p in parts])
  np.testing.assert_allclose(merged.sums, whole["sums"], rtol=1e-13, atol=1e-13)
  np.testing.assert_array_equal(merged.counts, whole["counts"])
  assert merged.invalid == 1 and merged.n_members == M and merged.n_climatology == K
  np.testing.assert_allclose(merged.acc, _scores(whole).acc, rtol=1e-12)
  with pytest.raises(ValueError, match="nothing"):
    ClimatologyScores.merge([])
  with pytest.raises(ValueError, match="differ"):
    ClimatologyScores.merge([_scores(parts[0]), ClimatologyScores(parts[1]["sums"], parts[1]["counts"], M, K + 1)])


def test_scaled_agrees_with_the_reference_on_affinely_mapped_inputs():
  M, K = 6, 5
  members, clim, truth, w = _data(M, K, seed=4)
  a = np.array([2.0, -0.5, 8.0])                            # powers of two: the mapped float32 values are exact
  b = np.random.default_rng(5).integers(-8, 9, truth.shape).astype(np.float32)      # an offset per point: it drops out
  mapped = R.reference(members * a.astype(np.float32) + b, clim * a.astype(np.float32) + b, truth * a.astype(np.float32) + b, w)
  got = _scores(R.reference(members, clim, truth, w)).scaled(a)
  # the affine-map term of DESIGN.md section 8c: the mapped values are rounded to float32 once more (the offset is added)
  tol = 1e-5 * mapped["abs"] + 1e-6 * np.abs(a)[None, :, None] * mapped["abs"][..., :1]
  assert np.all(np.abs(got.sums - mapped["sums"]) <= tol)
  np.testing.assert_array_equal(got.counts, mapped["counts"])
  np.testing.assert_allclose(got.acc, _scores(mapped).acc, rtol=1e-4)
  np.testing.assert_allclose(got.crpss, _scores(mapped).crpss, rtol=1e-4, atol=1e-6)
  for bad in ([1.0, 0.0, 1.0], [1.0, np.nan, 1.0], [1.0, 2.0]):
    with pytest.raises(ValueError):
      got.scaled(bad)


def test_per_variable_on_a_dataset_template():
  B, n_lat, n_lon = 2, 4, 6
  dims = ("batch", "time", "lat", "lon")
  template = datasets.Dataset({"t2m": datasets.Variable(dims, np.zeros((B, 1, n_lat, n_lon), np.float32)),
                               "z": datasets.Variable(("batch", "time", "level", "lat", "lon"),
                                                      np.zeros((B, 1, 2, n_lat, n_lon), np.float32))},
                              {"lat": np.linspace(-90, 90, n_lat), "lon": np.arange(n_lon) * 60.0, "level": np.array([500, 850])})
  layout = datasets.channel_layout(template)
  C = sum(n for _, _, n in layout)
  members, clim, truth, w = _data(4, 3, G=n_lat * n_lon, B=B, C=C, seed=6)
  sc = _scores(R.reference(members, clim, truth, w))
  out = sc.per_variable(template)
  for name, off, n in layout:
    np.testing.assert_array_equal(out["acc"][name], sc.acc[:, off:off + n])
    np.testing.assert_array_equal(out["crpss"][name], sc.crpss[:, off:off + n])
    assert out["valid_points"][name].shape == (B, n)
  assert set(out) >= {"acc", "acc_centred", "acc_members", "crps", "crps_climatology", "crpss", "msss", "rmse_climatology"}
  with pytest.raises(ValueError, match="channels"):
    ClimatologyScores(np.zeros((B, C + 1, 12)), np.zeros((B, C + 1), np.uint64), 4, 3).per_variable(template)


# ---- the two forms of the mean absolute difference ------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 8, 33, 50, 64])
@pytest.mark.parametrize("offset", [0.0, 300.0, 1e5])
def test_the_gap_form_is_the_pair_form_within_the_bound(M, offset):
  rng = np.random.default_rng(M)
  x = (offset + rng.standard_normal((M, 40, 2, 3)) * np.logspace(-2, 2, 3)).astype(np.float32)
  x[1, :10] = x[0, :10]                                     # ties
  x[:, 10:13] = x[0, 10:13]                                 # all equal: zero, on both sides
  pair, gap = R.pair_form(x), R.gap_form(x)
  bound = (M * M + 8) * 2.0 ** -53 * np.abs(pair)
  assert np.all(np.abs(pair - gap) <= bound)
  assert np.all(gap >= 0.0) and not gap[10:13].any() and not pair[10:13].any()
  members, clim, truth, w = _data(M, 3, G=40, seed=M, offset=offset)
  a, b = R.reference(members, clim, truth, w), R.reference(members, clim, truth, w, d=R.gap_form)
  assert np.all(np.abs(a["sums"] - b["sums"]) <= R.tolerance(a, 40))
  np.testing.assert_array_equal(a["sums"][..., :9], b["sums"][..., :9])   # only F5 and C5 depend on the form


# ---- the binding --------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_and_the_package_the_names():
  import gencast_flax_nnx_amd as pkg
  lib = _lib.load_library()
  assert hasattr(lib, "gc_ens_clim_score") and "gc_ens_clim_score" in _lib.SIGNATURES
  assert pkg.ClimatologyScores is ClimatologyScores and "ClimatologyScores" in pkg.__all__
  for owner, name in ((pkg.GenCast, "ensemble_climatology"), (pkg.NaNCleaner, "ensemble_climatology"),
                      (pkg.InputsAndResiduals, "ensemble_climatology"), (pkg.EnsembleSampler, "climatology"),
                      (pkg.Denoiser, "climatology_handle"), (_lib.NativeDenoiser, "ens_clim_score")):
    assert callable(getattr(owner, name)), name


def test_the_binding_checks_its_arguments_before_the_call():
  nd = object.__new__(_lib.NativeDenoiser)
  other = object.__new__(_lib.NativeDenoiser)
  nd._ens_members = 0
  with pytest.raises(TypeError):
    nd.ens_clim_score("not a handle")
  with pytest.raises(ValueError, match="another handle"):
    nd.ens_clim_score(nd)
  with pytest.raises(_lib.GencastHipError, match="ens_reserve"):
    nd.ens_clim_score(other)


# ---- ScoredStore(climatology=...) with a handle that records ------------------------------------------------------------------
def test_scored_store_pushes_the_samples_and_scores():
  log = []
  h, c = RecordingHandle("main", log), RecordingHandle("clim", log)
  st = verification.ScoredStore(h, 4, np.ones(6, np.float32), climatology=c)
  st.setup()
  assert log == [("main", "reserve", 4), ("main", "weight")]             # the climatology's store: sized by the first K
  fields = [np.full((6, 2, 3), float(j), np.float32) for j in range(3)]
  out = st.score_climatology(fields, "truth")
  assert isinstance(out, ClimatologyScores) and (out.n_members, out.n_climatology, out.invalid) == (4, 3, 7)
  assert log[2:] == [("clim", "reserve", 3), ("clim", "push_host", 0, 0.0), ("clim", "push_host", 1, 1.0),
                     ("clim", "push_host", 2, 2.0), ("main", "clim_score", "clim", False)]
  del log[:]
  st.score_climatology(fields, None)                                     # the same K: pushed again, not reserved again
  assert [x[1] for x in log] == ["push_host"] * 3 + ["clim_score"] and log[-1] == ("main", "clim_score", "clim", True)
  del log[:]
  assert st.score_climatology(None, None).n_climatology == 3             # the samples already there
  assert log == [("main", "clim_score", "clim", True)]
  del log[:]
  st.score_climatology(fields[:2], None)                                 # another K: a new store
  assert log[0] == ("clim", "reserve", 2) and len(log) == 4
  # without a climatology nothing of it is touched
  del log[:]
  plain = verification.ScoredStore(h, 4, np.ones(6, np.float32))
  plain.setup()
  assert plain.score_climatology(fields, None) is None and all(x[1] not in ("push_host", "clim_score") for x in log)


def test_a_derived_view_derives_its_climatology_from_the_source_climatology():
  log = []
  src, view, csrc, cview = (RecordingHandle(n, log) for n in ("src", "view", "csrc", "cview"))
  st = verification.ScoredStore(view, 4, np.ones(6, np.float32), plan={"op": [0]}, source=src, climatology=cview,
                                climatology_source=csrc)
  st.setup()
  st.score("source truth")
  del log[:]
  out = st.score_climatology(None, None, n_samples=5, source_truth="source truth")
  assert out.n_climatology == 5
  assert log == [("cview", "reserve", 5), ("cview", "derive_set"), ("cview", "derive", "csrc", "source truth"),
                 ("view", "clim_score", "cview", True)]
  del log[:]
  st.score_climatology(None, None, n_samples=5, source_truth="next truth")     # the plan and the store are kept
  assert log == [("cview", "derive", "csrc", "next truth"), ("view", "clim_score", "cview", True)]
  with pytest.raises(ValueError, match="climatology source"):
    verification.ScoredStore(view, 4, np.ones(6, np.float32), climatology_source=csrc)


# ---- rollout results ----------------------------------------------------------------------------------------------------
def _ens(M=4, B=2, C=3, seed=0):
  rng = np.random.default_rng(seed)
  return EnsembleScores(rng.uniform(1, 2, (B, C, 6)), rng.integers(0, 9, (B, C, M + 1)).astype(np.uint64), M)


def _clim_scores(seed):
  members, clim, truth, w = _data(4, 3, G=20, seed=seed)
  return _scores(R.reference(members, clim, truth, w))


def test_rollout_results_merge_with_and_without_climatology():
  c = [[_clim_scores(10 * d + k) for k in range(2)] for d in range(2)]
  with_c = [rollout.EnsembleRolloutResult([_ens(seed=k) for k in range(2)], n_members=4, climatology=c[d],
                                          climatology_normalized=c[d]) for d in range(2)]
  merged = with_c[0].merge(with_c[1])
  for k in range(2):
    np.testing.assert_array_equal(merged.climatology[k].sums, c[0][k].sums + c[1][k].sums)
    np.testing.assert_array_equal(merged.climatology_normalized[k].counts, c[0][k].counts + c[1][k].counts)
  without = rollout.EnsembleRolloutResult([_ens(seed=k) for k in range(2)], n_members=4)
  assert without.climatology is None and without.merge(without).climatology is None
  with pytest.raises(ValueError, match="climatology"):
    with_c[0].merge(without)
  with pytest.raises(ValueError, match="climatology"):
    without.merge(with_c[0])
  with pytest.raises(ValueError, match="lead times"):
    rollout.EnsembleRolloutResult([_ens()], n_members=4, climatology=c[0])
  d = [rollout.DerivedRolloutResult([_ens(seed=k) for k in range(2)], [_ens(seed=k) for k in range(2)], climatology=c[i],
                                    climatology_normalized=c[i]) for i in range(2)]
  dm = d[0].merge(d[1])
  np.testing.assert_array_equal(dm.climatology[1].sums, c[0][1].sums + c[1][1].sums)
  plain = rollout.DerivedRolloutResult([_ens(seed=k) for k in range(2)], [_ens(seed=k) for k in range(2)])
  assert plain.merge(plain).climatology is None
  with pytest.raises(ValueError, match="climatology"):
    d[0].merge(plain)


def test_the_sampler_refuses_more_than_one_rank_and_a_bad_sample_count():
  from gencast_flax_nnx_amd import ensemble

  class _S:
    _denoiser = None
  with pytest.raises(ValueError, match="one rank"):
    ensemble.EnsembleSampler(_S(), rank=0, world_size=2).climatology(None, None, None, 4, [None, None])
  with pytest.raises(ValueError, match="2..64"):
    ensemble.EnsembleSampler(_S()).climatology(None, None, None, 4, [None])
