"""Threshold-weighted CRPS, host side: the float64 reference of tests/tail_reference.py against closed
forms, `verification.TailScores`, the binding's own checks, `ScoredStore(tails=)`, the rollout's series and results and the
one-step wrappers.  No device."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, datasets, verification
from gencast_flax_nnx_amd.verification import EventSpec, TailScores
from tests import tail_reference as R


# ---- the reference against closed forms -----------------------------------------------------------------------------------------
def test_two_members_by_hand_on_both_sides_of_the_threshold():
  """x = (1, 4), y = 2.  Upper tail at t: v = max(., t); lower tail: v = min(., t).  ae = mean |v(x_i) - v(y)|, d = |v(x_0) -
  v(x_1)| (one pair), o = [y > t] / [y < t]."""
  members = np.array([1.0, 4.0], np.float32).reshape(2, 1, 1, 1)
  truth = np.array([2.0], np.float32).reshape(1, 1, 1)
  # t = 0 (below both), t = 3 (between: above the truth), t = 1.5 (between: below the truth), t = 5 (above both)
  hand = {(0.0, +1): (1.5, 3.0, 1.0),      # nothing clamps: |1-2|, |4-2| -> 1.5; |1-4| = 3
          (0.0, -1): (0.0, 0.0, 0.0),      # everything is 0
          (3.0, +1): (0.5, 1.0, 0.0),      # (3, 4) against 3: (0 + 1) / 2; |3-4| = 1; 2 > 3 is false
          (3.0, -1): (1.0, 2.0, 1.0),      # (1, 3) against 2: (1 + 1) / 2; |1-3| = 2; 2 < 3
          (1.5, +1): (1.25, 2.5, 1.0),     # (1.5, 4) against 2: (0.5 + 2) / 2; 2.5; 2 > 1.5
          (1.5, -1): (0.25, 0.5, 0.0),     # (1, 1.5) against 1.5: (0.5 + 0) / 2; 0.5; 2 < 1.5 is false
          (5.0, +1): (0.0, 0.0, 0.0),
          (5.0, -1): (1.5, 3.0, 1.0)}
  for (t, direction), (ae, d, o) in hand.items():
    got = R.point_terms(members, truth, np.full((1, 1, 1), t, np.float32), direction)
    assert (got[0].item(), got[1].item(), got[2].item(), bool(got[3].item())) == (ae, d, o, True), (t, direction)
  # the event is strict: a truth on the threshold is in neither tail's event, and counts
  for direction in (+1, -1):
    got = R.point_terms(members, truth, np.full((1, 1, 1), 2.0, np.float32), direction)
    assert got[2].item() == 0.0 and bool(got[3].item())
  ref = R.reference(members, truth, np.array([0.5], np.float32), np.array([3.0, 3.0], np.float32).reshape(2, 1, 1, 1), (+1, -1))
  np.testing.assert_array_equal(ref["sums"].reshape(2, 4), [[0.5, 0.25, 0.5, 0.0], [0.5, 0.5, 1.0, 0.5]])
  np.testing.assert_array_equal(ref["counts"].ravel(), [1, 1])
  np.testing.assert_array_equal(ref["invalid"], [0, 0])


@pytest.mark.parametrize("M", [2, 3, 8, 33, 50, 64])
def test_gap_form_is_pair_form_and_the_two_tails_add_up(M):
  """On float32 normals with exact ties, in float64: the gap form equals the pair form, and upper(t) + lower(t) equals the
  plain |x_i - y| and |x_i - x_j| term by term -- all three with error 0.0 (every difference of two such float32 values and
  every partial sum is exact in double)."""
  rng = np.random.default_rng(M)
  n = 257
  x = rng.standard_normal((M, n)).astype(np.float32)
  y = rng.standard_normal(n).astype(np.float32)
  thr = rng.standard_normal(n).astype(np.float32)
  x[M - 1, :40] = x[0, :40]                               # ties between members
  y[30:60] = x[0, 30:60]                                  # the truth on a member
  thr[50:80] = x[M // 2, 50:80]                           # the threshold on a member
  thr[80:100] = y[80:100]                                 # the threshold on the truth
  up, lo = R.clamp(x, thr, +1).astype(np.float64), R.clamp(x, thr, -1).astype(np.float64)
  yu, yl = R.clamp(y, thr, +1).astype(np.float64), R.clamp(y, thr, -1).astype(np.float64)
  x64, y64 = x.astype(np.float64), y.astype(np.float64)
  for u in (up, lo, x64):
    assert np.max(np.abs(R.gap_form(u) - R.pair_form(u))) == 0.0
  assert np.max(np.abs((np.abs(up - yu) + np.abs(lo - yl)) - np.abs(x64 - y64))) == 0.0          # ae, slot by slot
  for i in range(M):
    for j in range(i + 1, M):                                                                    # d, pair by pair
      assert np.max(np.abs((np.abs(up[i] - up[j]) + np.abs(lo[i] - lo[j])) - np.abs(x64[i] - x64[j]))) == 0.0
  assert np.max(np.abs((R.pair_form(up) + R.pair_form(lo)) - R.pair_form(x64))) == 0.0
  assert np.max(np.abs((np.abs(up - yu).sum(0) + np.abs(lo - yl).sum(0)) - np.abs(x64 - y64).sum(0))) == 0.0


def test_reference_skips_what_is_not_finite_per_threshold():
  rng = np.random.default_rng(5)
  M, G, B, C = 3, 6, 1, 2
  members = rng.standard_normal((M, G, B, C)).astype(np.float32)
  truth = rng.standard_normal((G, B, C)).astype(np.float32)
  thr = np.zeros((2, G, B, C), np.float32)
  truth[0, 0, 0] = np.nan
  members[1, 1, 0, 0] = np.inf
  thr[1, :, 0, 1] = np.nan
  thr[0, 2, 0, 1] = np.inf
  ref = R.reference(members, truth, np.ones(G, np.float32), thr, (+1, -1))
  np.testing.assert_array_equal(ref["counts"], np.array([[[4, 5]], [[4, 0]]], np.uint64))
  np.testing.assert_array_equal(ref["invalid"], [3, 8])
  assert np.isfinite(ref["sums"]).all() and not ref["sums"][1, 0, 1].any()
  np.testing.assert_array_equal(ref["sums"][..., 0], ref["counts"].astype(np.float64))


# ---- TailScores ---------------------------------------------------------------------------------------------------------------------
def _scores(rng, T=2, B=2, C=3, M=4, directions=(+1, -1)):
  sums = rng.uniform(1, 2, (T, B, C, 4))
  return TailScores(sums, rng.integers(1, 9, (T, B, C)).astype(np.uint64), M, directions, rng.integers(0, 5, T).astype(np.uint64))


def test_tail_scores_formulas():
  rng = np.random.default_rng(0)
  sc = _scores(rng, M=5)
  s = sc.sums
  np.testing.assert_array_equal(sc.twcrps, (s[..., 1] - 0.5 * s[..., 2]) / s[..., 0])
  np.testing.assert_array_equal(sc.twcrps_ensemble, (s[..., 1] - 0.5 * (4.0 / 5.0) * s[..., 2]) / s[..., 0])
  np.testing.assert_array_equal(sc.abs_error, s[..., 1] / s[..., 0])
  np.testing.assert_array_equal(sc.pair_distance, s[..., 2] / s[..., 0])
  np.testing.assert_array_equal(sc.base_rate, s[..., 3] / s[..., 0])
  np.testing.assert_array_equal(sc.valid_weight, s[..., 0])
  assert sc.valid_points is sc.counts and sc.directions == (1, -1) and sc.n_members == 5
  for name in ("twcrps", "twcrps_ensemble", "abs_error", "pair_distance", "base_rate"):
    assert getattr(sc, name).shape == (2, 2, 3) and getattr(sc, name).dtype == np.float64
  # nothing counted (a NaN threshold): NaN, not an error
  s0 = s.copy()
  s0[1, 0, 2] = 0.0
  empty = TailScores(s0, sc.counts, 5, sc.directions)
  assert np.isnan(empty.twcrps[1, 0, 2]) and np.isnan(empty.base_rate[1, 0, 2]) and np.isfinite(empty.twcrps[0]).all()
  np.testing.assert_array_equal(empty.invalid, [0, 0])
  for bad in (dict(sums=s[..., :3]), dict(counts=sc.counts[:1]), dict(n_members=1), dict(directions=(1,)), dict(directions=(1, 0))):
    args = dict(sums=s, counts=sc.counts, n_members=5, directions=(1, -1))
    args.update(bad)
    with pytest.raises(ValueError):
      TailScores(**args)


def test_tail_scores_merge_scaled_and_per_variable():
  rng = np.random.default_rng(1)
  a, b = _scores(rng), _scores(rng)
  m = TailScores.merge([a, b])
  np.testing.assert_array_equal(m.sums, a.sums + b.sums)
  np.testing.assert_array_equal(m.counts, a.counts + b.counts)
  np.testing.assert_array_equal(m.invalid, a.invalid + b.invalid)
  assert m.directions == a.directions and m.n_members == a.n_members
  for other in (_scores(rng, M=5), _scores(rng, directions=(+1, +1)), _scores(rng, C=4)):
    with pytest.raises(ValueError, match="differ"):
      TailScores.merge([a, other])
  with pytest.raises(ValueError, match="nothing"):
    TailScores.merge([])
  scale = np.array([4.0, 1.0, 0.25])
  sc = a.scaled(scale)
  np.testing.assert_array_equal(sc.sums[..., 0], a.sums[..., 0])
  np.testing.assert_array_equal(sc.sums[..., 1], a.sums[..., 1] * scale)
  np.testing.assert_array_equal(sc.sums[..., 2], a.sums[..., 2] * scale)
  np.testing.assert_array_equal(sc.sums[..., 3], a.sums[..., 3])
  np.testing.assert_array_equal(sc.twcrps, a.twcrps * scale)
  np.testing.assert_array_equal(sc.base_rate, a.base_rate)
  assert sc.counts is a.counts or np.array_equal(sc.counts, a.counts)
  np.testing.assert_array_equal(sc.invalid, a.invalid)
  for bad in ([1.0, -1.0, 1.0], [1.0, 0.0, 1.0], [1.0, np.nan, 1.0], [1.0, np.inf, 1.0]):   # a negative scale swaps the tails
    with pytest.raises(ValueError, match="> 0"):
      a.scaled(bad)
  with pytest.raises(ValueError, match="shape"):
    a.scaled([1.0, 2.0])
  flat = ("batch", "time", "lat", "lon")
  z = np.zeros((2, 1, 2, 2), np.float32)
  template = datasets.Dataset({"p": datasets.Variable(("batch", "time", "level", "lat", "lon"), np.zeros((2, 1, 2, 2, 2), np.float32)),
                               "q": datasets.Variable(flat, z)}, {"lat": np.array([-45.0, 45.0]), "lon": np.array([0.0, 180.0]),
                                                                  "level": np.array([500, 850])})
  pv = a.per_variable(template)
  layout = {name: (off, n) for name, off, n in datasets.channel_layout(template)}
  assert set(pv) == {"twcrps", "twcrps_ensemble", "abs_error", "pair_distance", "base_rate", "valid_weight", "valid_points"}
  for name, (off, n) in layout.items():
    np.testing.assert_array_equal(pv["twcrps"][name], a.twcrps[:, :, off:off + n])
    np.testing.assert_array_equal(pv["valid_points"][name], a.counts[:, :, off:off + n])
  with pytest.raises(ValueError, match="channels"):
    _scores(rng, C=4).per_variable(template)


# ---- the ABI and the binding's own checks: before the C call, so without a device -----------------------------------------------
def test_the_entries_are_declared_exported_and_bound():
  import gencast_flax_nnx_amd as pkg
  lib = _lib.load_library()
  for name in ("gc_ens_tail_set", "gc_ens_tail_score"):
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert hasattr(_lib.NativeDenoiser, name[3:])
  assert pkg.TailScores is verification.TailScores and "TailScores" in pkg.__all__
  assert lib.gc_abi_version() == 1 and lib.gc_num_kernel_classes() == 13
  for where in (pkg.EnsembleSampler, pkg.GenCast, pkg.InputsAndResiduals, pkg.NaNCleaner):
    assert hasattr(where, "tails" if where is pkg.EnsembleSampler else "ensemble_tails")


class _NoCall:
  def __getattr__(self, name):
    raise AssertionError(f"{name} must not be reached")


def test_binding_rejects_bad_arguments_before_the_c_call():
  nd = object.__new__(_lib.NativeDenoiser)
  nd._lib, nd._h = _NoCall(), None
  nd.cfg = _lib.GcConfig(128, 128, 2, 256, 1, 10, 6, 2, 32, 32, 16.0)
  nd.num_grid_nodes, nd._ens_members, nd._tail_thresholds = 312, 0, 0
  thr = np.zeros((2, 312, 2, 6), np.float32)
  for t, d in ((thr[0], (1,)), (thr[:, :311], (1, -1)), (np.zeros((9, 312, 2, 6), np.float32), (1,) * 9),
               (thr[:0], ()), (thr, (1,)), (thr, (1, 0)), (thr, (1, -1, 1))):
    with pytest.raises(ValueError):
      nd.ens_tail_set(t, d)
  with pytest.raises(_lib.GencastHipError, match="ens_tail_set"):
    nd.ens_tail_score(None)
  nd._tail_thresholds = 2
  with pytest.raises(_lib.GencastHipError, match="ens_reserve"):
    nd.ens_tail_score(None)
  nd._ens_members = 8
  with pytest.raises(ValueError, match="truth must be"):
    nd.ens_tail_score(np.zeros((312, 2, 5), np.float32))


# ---- ScoredStore(tails=) with a handle that records -----------------------------------------------------------------------------
class _Handle:
  def __init__(self, M, B=2, C=3, T=2):
    self.calls, self.M, self.B, self.C, self.T = [], M, B, C, T

  def ens_reserve(self, n):
    self.calls.append(("reserve", n))

  def ens_set_node_weight(self, w):
    self.calls.append(("weight",))

  def ens_tail_set(self, thresholds, directions):
    self.calls.append(("tail_set", thresholds, tuple(directions)))

  def ens_tail_score(self, truth):
    self.calls.append(("tail_score", truth is None))
    n = sum(1 for c in self.calls if c[0] == "tail_score")
    return (np.full((self.T, self.B, self.C, 4), float(n)), np.full((self.T, self.B, self.C), 5, np.uint64),
            np.full(self.T, 7, np.uint64))

  def ens_score(self, truth, want_fields=False):
    self.calls.append(("score", truth is None))
    return np.ones((self.B, self.C, 6)), np.ones((self.B, self.C, self.M + 1), np.uint64)


def _spec():
  return EventSpec({"q": np.array([1.0, -1.0])}, (+1, -1))


def test_scored_store_sets_the_tails_and_scores():
  h = _Handle(4)
  st = verification.ScoredStore(h, 4, np.ones(4, np.float32), tails=_spec(), tail_thresholds="packed")
  st.setup()
  assert h.calls == [("reserve", 4), ("weight",), ("tail_set", "packed", (1, -1))]
  got = st.score_tails("truth")
  assert h.calls[-1] == ("tail_score", False)
  assert isinstance(got, TailScores) and got.n_members == 4 and got.directions == (1, -1)
  np.testing.assert_array_equal(got.invalid, [7, 7])
  np.testing.assert_array_equal(got.twcrps, 0.5)                  # (1 - 1/2) / 1
  st.score_tails(None)
  assert h.calls[-1] == ("tail_score", True)
  # without tails no call is made on the handle
  h2 = _Handle(4)
  plain = verification.ScoredStore(h2, 4, np.ones(4, np.float32))
  plain.setup()
  plain.configure()
  assert plain.score_tails(None) is None and plain.tails is None
  assert h2.calls == [("reserve", 4), ("weight",)]
  # set per score: the thresholds are set again by every scoring call, not by setup
  h3 = _Handle(4)
  per = verification.ScoredStore(h3, 4, np.ones(4, np.float32), tails=_spec(), tail_thresholds="packed", set_per_score=True)
  per.setup()
  assert h3.calls == [("reserve", 4), ("weight",)]
  per.score_tails(None)
  assert [c[0] for c in h3.calls[2:]] == ["tail_set", "tail_score"]


def test_store_series_appends_the_tail_scores_after_the_others():
  from gencast_flax_nnx_amd import rollout
  h = _Handle(4)
  store = verification.ScoredStore(h, 4, np.ones(4, np.float32), tails=_spec(), tail_thresholds="packed")
  store.setup()
  scale = np.array([4.0, 1.0, 0.25])
  series = rollout._StoreSeries(store, scale, None)
  series.score_lead("truth")
  series.score_lead("truth")
  assert [c[0] for c in h.calls[3:]] == ["score", "tail_score"] * 2
  assert h.calls[4] == ("tail_score", True)                       # on the truth already on the device
  assert len(series.tails) == len(series.raw_tails) == 2
  np.testing.assert_array_equal(series.raw_tails[1].sums, 2.0)    # in the order of the calls
  np.testing.assert_array_equal(series.tails[0].sums[..., 1], series.raw_tails[0].sums[..., 1] * scale)
  np.testing.assert_array_equal(series.tails[0].sums[..., 0], series.raw_tails[0].sums[..., 0])
  d = series.derived_result()
  assert len(d.tails) == 2 and len(d.tails_normalized) == 2 and d.tails[0] is series.tails[0]
  plain = rollout._StoreSeries(verification.ScoredStore(_Handle(4), 4, np.ones(4, np.float32)), np.ones(3), None)
  assert plain.tails is None and plain.raw_tails is None
  plain.score_lead("truth")
  assert [c[0] for c in plain.store.handle.calls] == ["score"]
  assert "tails" not in vars(plain.derived_result())


def test_rollout_results_merge_with_and_without_tails():
  from gencast_flax_nnx_amd import rollout
  rng = np.random.default_rng(0)
  M, B, C = 4, 2, 3
  ens = lambda: verification.EnsembleScores(rng.uniform(1, 2, (B, C, 6)), rng.integers(0, 9, (B, C, M + 1)).astype(np.uint64), M)
  tl = [[_scores(rng) for _ in range(2)] for _ in range(2)]
  with_t = [rollout.EnsembleRolloutResult([ens() for _ in range(2)], n_members=M, tails=tl[d], tails_normalized=tl[d]) for d in range(2)]
  merged = with_t[0].merge(with_t[1])
  for k in range(2):
    np.testing.assert_array_equal(merged.tails[k].sums, tl[0][k].sums + tl[1][k].sums)
    np.testing.assert_array_equal(merged.tails_normalized[k].counts, tl[0][k].counts + tl[1][k].counts)
  without = rollout.EnsembleRolloutResult([ens() for _ in range(2)], n_members=M)
  assert without.tails is None and without.tails_normalized is None
  assert "tails" not in vars(without) and "tails_normalized" not in vars(without)   # a result not asked for them is as it was
  assert sorted(vars(without)) == sorted(["scores", "scores_normalized", "spectra", "spectra_normalized", "events", "order",
                                          "order_normalized", "climatology", "climatology_normalized", "derived", "windows",
                                          "mean", "variance", "members", "quantiles", "n_members"])
  assert without.merge(without).tails is None and "tails" not in vars(without.merge(without))
  with pytest.raises(ValueError, match="tail scores"):
    with_t[0].merge(without)
  with pytest.raises(ValueError, match="tail scores"):
    without.merge(with_t[0])
  with pytest.raises(ValueError, match="lead times"):
    rollout.EnsembleRolloutResult([ens()], n_members=M, tails=tl[0], tails_normalized=tl[0])
  d = [rollout.DerivedRolloutResult([ens() for _ in range(2)], [ens() for _ in range(2)], tails=tl[i], tails_normalized=tl[i])
       for i in range(2)]
  np.testing.assert_array_equal(d[0].merge(d[1]).tails[1].sums, tl[0][1].sums + tl[1][1].sums)
  w = [rollout.WindowRolloutResult([1, 3], 2, [ens() for _ in range(2)], [ens() for _ in range(2)], tails=tl[i],
                                   tails_normalized=tl[i]) for i in range(2)]
  np.testing.assert_array_equal(w[0].merge(w[1]).tails[0].sums, tl[0][0].sums + tl[1][0].sums)
  plain = rollout.WindowRolloutResult([1, 3], 2, [ens() for _ in range(2)], [ens() for _ in range(2)])
  assert plain.merge(plain).tails is None and "tails" not in vars(plain)
  with pytest.raises(ValueError, match="tail scores"):
    w[0].merge(plain)


def test_sampler_refuses_more_than_one_rank():
  from gencast_flax_nnx_amd import ensemble

  class _S:
    _denoiser = None
  with pytest.raises(ValueError, match="one rank"):
    ensemble.EnsembleSampler(_S(), rank=0, world_size=2).tails(None, None, None, 4, _spec())


def test_rollout_refuses_a_tails_key_that_names_no_store():
  from gencast_flax_nnx_amd import rollout, synthetic
  lat, lon = np.linspace(-90, 90, 5), np.arange(8) * 45.0
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  spec = EventSpec({"2m_temperature": np.array([280.0])}, (+1,))
  runner = rollout.EnsembleRollout(model=None)                    # (the check comes before anything touches the model)
  with pytest.raises(ValueError, match="nope"):
    runner.run(inp, tgt, frc, 1, 3, tails={None: spec, "nope": spec})
  with pytest.raises(ValueError, match="wind"):
    runner.run(inp, tgt, frc, 1, 3, tails={"wind": spec}, windows=None, derived=None)


# ---- the one-step wrappers ----------------------------------------------------------------------------------------------------------
def test_wrappers_map_the_thresholds_and_scale_the_sums_back():
  """`InputsAndResiduals.ensemble_tails` hands the wrapped predictor normalised inputs, residual-normalised targets and the
  thresholds sent through the map of the targets (exactly as `ensemble_events` does), and scales S1 and S2 back with the
  residual scale of every target channel; `NaNCleaner` cleans inputs and forcings and lets the targets' NaNs through."""
  from gencast_flax_nnx_amd import NaNCleaner, config, rollout, synthetic
  lat, lon = np.linspace(-90, 90, 5), np.arange(8) * 45.0
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  C, M, T = 82, 4, 2
  rng = np.random.default_rng(1)
  raw = TailScores(rng.uniform(1, 2, (T, 1, C, 4)), rng.integers(1, 9, (T, 1, C)).astype(np.uint64), M, (+1, -1), [3, 4])
  seen = {}

  class _Predictor:
    def ensemble_tails(self, inputs, targets, forcings=None, **kwargs):
      seen.update(inputs=inputs, targets=targets, forcings=forcings, kwargs=kwargs)
      return raw

    def ensemble_events(self, inputs, targets, forcings=None, **kwargs):
      seen.update(event_kwargs=kwargs)
      return None

  def stats(v):
    names = set(config.TASK.input_variables) | set(config.TASK.target_variables) | set(frc.keys())
    return datasets.Dataset({n: (datasets.Variable(("level",), np.full(13, v, np.float32)) if n in config.ALL_ATMOSPHERIC_VARS
                                 else datasets.Variable((), np.float32(v))) for n in names})
  norm = rollout.InputsAndResiduals(_Predictor(), stats(2.0), stats(0.5), stats(0.25))
  k = "2m_temperature"
  spec = EventSpec({k: np.array([280.0, 270.0])}, (+1, -1))
  got = norm.ensemble_tails(inp, tgt, frc, num_members=M, spec=spec)
  assert set(seen["kwargs"]) == {"num_members", "spec"} and seen["kwargs"]["num_members"] == M
  np.testing.assert_array_equal(seen["inputs"][k].data, (inp[k].data - np.float32(0.5)) / np.float32(2.0))
  np.testing.assert_array_equal(seen["targets"][k].data, (tgt[k].data - inp[k].data[:, -1:]) / np.float32(0.25))
  nspec = seen["kwargs"]["spec"]
  assert nspec.directions == (1, -1)
  for t, value in enumerate((280.0, 270.0)):                      # the map of the targets: residual, then the residual scale
    want = (np.full_like(tgt[k].data, value) - inp[k].data[:, -1:]) / np.float32(0.25)
    np.testing.assert_array_equal(nspec.thresholds[k][t], want)
  norm.ensemble_events(inp, tgt, frc, num_members=M, spec=spec)   # the same thresholds as the events get
  for name in nspec.thresholds:
    np.testing.assert_array_equal(nspec.thresholds[name], seen["event_kwargs"]["spec"].thresholds[name])
  assert set(tgt.keys()) <= set(inp.keys())                       # every target is a residual variable: scale 0.25
  np.testing.assert_array_equal(got.sums[..., 1], raw.sums[..., 1] * 0.25)
  np.testing.assert_array_equal(got.sums[..., 2], raw.sums[..., 2] * 0.25)
  np.testing.assert_array_equal(got.sums[..., 0], raw.sums[..., 0])
  np.testing.assert_array_equal(got.sums[..., 3], raw.sums[..., 3])
  np.testing.assert_array_equal(got.counts, raw.counts)
  np.testing.assert_array_equal(got.invalid, [3, 4])
  # NaNCleaner around it: a NaN in the inputs is filled, one in the targets reaches the predictor
  dirty_in = datasets.Dataset({n: datasets.Variable(v.dims, np.array(v.data, copy=True)) for n, v in inp.items()}, inp.coords)
  dirty_tg = datasets.Dataset({n: datasets.Variable(v.dims, np.array(v.data, copy=True)) for n, v in tgt.items()}, tgt.coords)
  dirty_in[k].data[..., 0, 0] = np.nan
  dirty_tg[k].data[..., 1, 1] = np.nan
  stack = NaNCleaner(norm, k, datasets.Dataset({k: datasets.Variable((), np.float32(0))}))
  again = stack.ensemble_tails(dirty_in, dirty_tg, frc, num_members=M, spec=spec)
  assert np.array_equal(again.sums, got.sums)
  assert np.isfinite(seen["inputs"][k].data).all() and np.isnan(seen["targets"][k].data[..., 1, 1]).all()
