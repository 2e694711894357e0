"""The fractions skill score without a device: the two restatements of the definition (tests/fss_reference.py) against each
other, the displacement law and the growth of skill with scale on them, `verification.FractionsScores`, `EventSpec(scales_km=)`,
`quantize_row_weights`, `EventScores.merge` with fractions, the events row of `SCORERS` with a recording handle, and the ABI."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import EventScores, EventSpec, _lib, losses, synthetic, verification
from gencast_flax_nnx_amd.verification import DerivedSpec, FractionsScores, quantize_row_weights
from tests import fss_reference as R
from tests.test_abi import _declared

N_LAT, N_LON, M = 13, 24, 4
LAT = np.linspace(-90, 90, N_LAT)
ROW_WQ = quantize_row_weights(losses.normalized_latitude_weights(LAT))
WQ = np.repeat(ROW_WQ, N_LON).astype(np.uint32)
SCALES = ((0, 0), (1, 2), (3, 5), (12, 11))                  # (r_lat, r_lon everywhere)


def _full(r):
  return np.full(N_LAT, r, np.int32)


# ---- the reference, twice ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_lat,r_lon", [(0, _full(0)), (1, _full(2)), (3, DerivedSpec.window(LAT, np.arange(N_LON) * 15.0, 2500.0)[1]),
                                         (12, _full(11))])
def test_the_literal_and_the_separable_reference_agree_exactly(r_lat, r_lon):
  code = R.random_codes(N_LAT, N_LON, M, seed=3)
  code[6, :] = 255
  code[6, 5] = 2 | 128                                      # a counted centre, its row otherwise not counted
  lit = R.literal(code, M, r_lat, r_lon, ROW_WQ, WQ)
  valid, A, B, N, P, O = R.point_fields(code.reshape(-1), M, N_LAT, N_LON, r_lat, r_lon, ROW_WQ)
  grid = lambda a: a.reshape(N_LAT, N_LON)
  assert (grid(valid) == (code != 255)).all() and valid.sum() > 200
  for name, got in (("A", A), ("B", B), ("N", N)):
    assert (grid(got)[code != 255] == lit[name][code != 255].astype(np.int64)).all(), name
  np.testing.assert_array_equal(grid(P), lit["P"])          # NaN where the point does not count, on both sides
  np.testing.assert_array_equal(grid(O), lit["O"])
  np.testing.assert_array_equal(R.column_sums(valid, P, O, WQ), lit["sums"])
  both = R.separable(code.reshape(1, -1, 1, 1), M, N_LAT, N_LON, [r_lat], [r_lon], ROW_WQ, WQ)
  np.testing.assert_array_equal(both["sums"][0, 0, 0, 0], lit["sums"])
  np.testing.assert_array_equal(both["prob"][0, 0, :, 0, 0], lit["P"].reshape(-1).astype(np.float32))


def test_a_lone_counted_centre_sees_itself_only():
  code = np.full((N_LAT, N_LON), 255, np.uint8)
  code[6, 5] = 3 | 128
  lit = R.literal(code, M, 12, _full(11), ROW_WQ, WQ)
  assert lit["N"][6, 5] == int(ROW_WQ[6]) and lit["P"][6, 5] == 0.75 and lit["O"][6, 5] == 1.0
  w = float(WQ[6 * N_LON + 5])
  assert lit["sums"] == [w * 0.0625, w * (0.5625 + 1.0), w * 0.75, w]


# ---- what the score must do ---------------------------------------------------------------------------------------------------
def test_displacement_law():
  """The truth in the event at one point per row, every member 3 columns east, r_lat = 0: a window of 2 r + 1 longitudes holds
  both from r = 3 on and FSS = max(0, 2 r + 1 - 3) / (2 r + 1).  (At r = 11 the windows wrap onto each other: not part of it.)"""
  code = R.displacement_codes(N_LAT, N_LON, M, 3)
  for r, want in ((0, 0.0), (1, 0.0), (3, 4.0 / 7.0), (5, 8.0 / 11.0)):
    s = R.literal(code, M, 0, _full(r), ROW_WQ, WQ)["sums"]
    assert abs((1.0 - s[0] / s[1]) - want) <= 1e-15, (r, 1.0 - s[0] / s[1], want)
    assert want == max(0, 2 * r + 1 - 3) / (2 * r + 1)


def test_fss_rises_with_scale_on_random_codes():
  code = R.random_codes(N_LAT, N_LON, M, seed=0)
  fss = []
  for r_lat, r in SCALES:
    s = R.literal(code, M, r_lat, _full(r), ROW_WQ, WQ)["sums"]
    fss.append(1.0 - s[0] / s[1])
  print("fss at", SCALES, fss)
  assert all(a < b for a, b in zip(fss, fss[1:])) and 0.0 < fss[0] and fss[-1] < 1.0


# ---- FractionsScores ----------------------------------------------------------------------------------------------------------
def _sums(seed, T=2, S=3, B=2, C=3):
  rng = np.random.default_rng(seed)
  sums = np.empty((T, S, B, C, 4))
  sums[..., 1] = rng.uniform(1.0, 2.0, (T, S, B, C))
  sums[..., 0] = sums[..., 1] * rng.uniform(0.0, 1.0, (T, S, B, C))
  sums[..., 2:] = rng.uniform(0.1, 1.0, (T, S, B, C, 2))
  return sums, rng.integers(2, 9, (T, B, C)).astype(np.uint64)


def _fs(seed, **kw):
  sums, weight = _sums(seed, **kw)
  return FractionsScores(sums, weight, 4, (1, -1), (0.0, 200.0, 500.0), 8.0)


def test_fractions_scores_are_the_formulas():
  fs = _fs(0)
  want = R.scores(fs.sums, fs.weight)
  for name, ref in want.items():
    np.testing.assert_array_equal(getattr(fs, name), ref, err_msg=name)
  np.testing.assert_array_equal(fs.valid_weight, fs.weight.astype(np.float64) / 8.0)
  assert fs.fss.shape == (2, 3, 2, 3)


def test_zero_denominators_give_nan():
  sums, weight = _sums(1)
  sums[0, :, 0, 0] = 0.0                                    # nobody in the event, nothing counted
  weight[0, 0, 0] = 0
  sums[1, 1, 1, 1, 3] = 0.0                                 # never observed in this column at this scale
  fs = FractionsScores(sums, weight, 4, (1, -1), (0.0, 200.0, 500.0), 8.0)
  for name in ("fss", "fbs", "forecast_fraction", "observed_fraction", "fss_uniform", "frequency_bias"):
    assert np.isnan(getattr(fs, name)[0, :, 0, 0]).all(), name
  assert np.isnan(fs.frequency_bias[1, 1, 1, 1]) and np.isfinite(fs.fss[1, 1, 1, 1])
  assert np.isnan(fs.skilful_scale_km[0, 0, 0])


def test_skilful_scale_is_the_smallest_that_clears_the_bar():
  sums = np.zeros((1, 3, 1, 4, 4))
  weight = np.full((1, 1, 4), 10, np.uint64)
  sums[..., 1] = 1.0
  sums[..., 3] = 2.0                                        # observed fraction 0.2: the bar is 0.6
  for c, fss in enumerate(([0.7, 0.8, 0.9], [0.1, 0.6, 0.9], [0.1, 0.2, 0.61], [0.1, 0.2, 0.3])):
    sums[0, :, 0, c, 0] = 1.0 - np.asarray(fss)
  fs = FractionsScores(sums, weight, 4, (1,), (0.0, 200.0, 500.0), 1.0)
  np.testing.assert_array_equal(fs.fss_uniform, 0.6)
  np.testing.assert_array_equal(fs.skilful_scale_km[0, 0], [0.0, 200.0, 500.0, np.nan])


def test_merge_is_the_scores_of_the_dates_taken_together():
  a, b = _fs(2), _fs(3)
  both = FractionsScores.merge([a, b])
  np.testing.assert_array_equal(both.sums, a.sums + b.sums)
  np.testing.assert_array_equal(both.weight, a.weight + b.weight)
  np.testing.assert_array_equal(both.fss, 1.0 - (a.sums[..., 0] + b.sums[..., 0]) / (a.sums[..., 1] + b.sums[..., 1]))
  assert not np.allclose(both.fss, 0.5 * (a.fss + b.fss))   # never a mean of scores
  assert both.scales_km == a.scales_km and both.n_members == 4 and both.directions == (1, -1) and both.scale == 8.0
  # on the reference: two "dates" of codes side by side are one column of twice the centres
  c1, c2 = R.random_codes(N_LAT, N_LON, M, 5), R.random_codes(N_LAT, N_LON, M, 6)
  s1, s2 = (np.array(R.literal(c, M, 1, _full(2), ROW_WQ, WQ)["sums"]) for c in (c1, c2))
  w = lambda c: np.uint64(int(WQ.reshape(N_LAT, N_LON)[c != 255].astype(np.uint64).sum()))
  one = lambda s, c: FractionsScores(s.reshape(1, 1, 1, 1, 4), np.array([[[w(c)]]]), M, (1,), (300.0,), 1.0)
  merged = FractionsScores.merge([one(s1, c1), one(s2, c2)])
  assert merged.fss[0, 0, 0, 0] == 1.0 - (s1[0] + s2[0]) / (s1[1] + s2[1])
  assert merged.fbs[0, 0, 0, 0] == (s1[0] + s2[0]) / float(int(w(c1)) + int(w(c2)))


def test_merge_and_constructor_raise_on_mismatch():
  sums, weight = _sums(4)
  a = _fs(4)
  for other in (FractionsScores(sums, weight, 5, (1, -1), (0.0, 200.0, 500.0), 8.0),
                FractionsScores(sums, weight, 4, (1, 1), (0.0, 200.0, 500.0), 8.0),
                FractionsScores(sums, weight, 4, (1, -1), (0.0, 200.0, 600.0), 8.0),
                FractionsScores(sums, weight, 4, (1, -1), (0.0, 200.0, 500.0), 4.0),
                FractionsScores(sums[:, :, :1], weight[:, :1], 4, (1, -1), (0.0, 200.0, 500.0), 8.0)):
    with pytest.raises(ValueError, match="merge: the parts differ in members, directions, scales, scale or shape"):
      FractionsScores.merge([a, other])
  with pytest.raises(ValueError, match="nothing to merge"):
    FractionsScores.merge([])
  for bad in (dict(sums=sums[..., :3]), dict(weight=weight[:1]), dict(n_members=1), dict(directions=(1,)),
              dict(scales_km=(0.0, 1.0)), dict(scale=0.0)):
    kw = dict(sums=sums, weight=weight, n_members=4, directions=(1, -1), scales_km=(0.0, 200.0, 500.0), scale=8.0)
    kw.update(bad)
    with pytest.raises(ValueError):
      FractionsScores(**kw)


def test_per_variable_splits_the_channel_axis():
  tgt = synthetic.make_example(lat=np.linspace(-90, 90, 5), lon=np.arange(8) * 45.0, batch=2, seed=1)[1]
  fs = FractionsScores(*_sums(7, C=82), 4, (1, -1), (0.0, 200.0, 500.0), 8.0)
  pv = fs.per_variable(tgt)
  assert set(pv) == set(FractionsScores._listed)
  assert pv["fss"]["temperature"].shape == (2, 3, 2, 13) and pv["fss"]["2m_temperature"].shape == (2, 3, 2, 1)


# ---- EventSpec(scales_km=), quantize_row_weights, EventScores.merge ------------------------------------------------------------------
def test_event_spec_takes_scales_and_hands_them_on():
  tgt = synthetic.make_example(lat=np.linspace(-90, 90, 5), lon=np.arange(8) * 45.0, batch=2, seed=1)[1]
  thr = {"2m_temperature": np.array([1.0, 2.0])}
  plain = EventSpec(thr, [1, -1])
  assert plain.scales_km is None and plain.fractions_plan is None
  plain.packed(tgt)
  assert plain.fractions_plan is None
  with pytest.raises(ValueError, match="no scales_km"):
    plain.windows(tgt)
  spec = EventSpec(thr, [1, -1], scales_km=[0, 5000.0, 10000])
  assert spec.scales_km == (0.0, 5000.0, 10000.0)
  assert spec.mapped(tgt, lambda name, v: v).scales_km == spec.scales_km
  r_lat, r_lon, row_wq = spec.windows(tgt)
  assert r_lat.dtype == np.int32 and r_lon.dtype == np.int32 and row_wq.dtype == np.uint32
  assert r_lat.shape == (3,) and r_lon.shape == (3, 5) and row_wq.shape == (5,)
  for s, radius in enumerate(spec.scales_km):
    want = DerivedSpec.window(np.linspace(-90, 90, 5), np.arange(8) * 45.0, radius)
    assert r_lat[s] == want[0] and (r_lon[s] == want[1]).all()
  assert r_lat[0] == 0 and (r_lon[0, 1:-1] == 0).all() and r_lat[1] == 1
  np.testing.assert_array_equal(row_wq, quantize_row_weights(losses.normalized_latitude_weights(np.linspace(-90, 90, 5))))
  np.testing.assert_array_equal(spec.packed(tgt), plain.packed(tgt))           # the thresholds are what they were
  for got, want in zip(spec.fractions_plan, (r_lat, r_lon, row_wq)):
    np.testing.assert_array_equal(got, want)
  for bad in ([], [200.0, 100.0], [100.0, 100.0], [-1.0], [np.nan], [np.inf], list(range(9))):
    with pytest.raises(ValueError, match="scales_km"):
      EventSpec(thr, [1, -1], scales_km=bad)


def test_a_feature_spec_hands_its_scales_to_the_event_spec_of_its_strike_store():
  det = {"low": dict(variable="mean_sea_level_pressure", kind="min", radius_km=600, strike_km=300)}
  assert verification.FeatureSpec(det).event_spec().scales_km is None
  ev = verification.FeatureSpec(det, scales_km=[0, 300.0]).event_spec()
  assert ev.scales_km == (0.0, 300.0) and ev.directions == (1,) and list(ev.thresholds) == ["low"]
  with pytest.raises(ValueError, match="scales_km"):
    verification.FeatureSpec(det, scales_km=[300.0, 0.0])


def test_quantize_row_weights_keeps_the_pole_rows_of_the_quarter_degree_grid():
  lat = np.linspace(-90, 90, 721)
  w = losses.normalized_latitude_weights(lat)
  q = quantize_row_weights(w)
  assert q.dtype == np.uint32 and q.min() >= 1 and q.max() <= 2 ** 24 - 1 and 2 * int(q.max()) > 2 ** 24 - 1
  e = -1100
  while w.max() * 2.0 ** (e + 1) <= 2 ** 24 - 1:              # the largest e by search (times a power of two: exact)
    e += 1
  np.testing.assert_array_equal(q, np.maximum(1, np.rint(w * 2.0 ** e)))
  assert q[0] == q[-1] and q[0] >= 1 and q[0] < q[1]
  tiny = quantize_row_weights([1e-12, 1.0, 0.0])
  np.testing.assert_array_equal(tiny, [1, 2 ** 23, 1])        # a weight that rounds to 0 keeps 1
  np.testing.assert_array_equal(quantize_row_weights([1.0, 0.5], bits=4), [8, 4])
  for bad in ([], [np.nan, 1.0], [-1.0, 1.0], [0.0, 0.0], [np.inf]):
    with pytest.raises(ValueError):
      quantize_row_weights(bad)


def _events(seed, fractions=None):
  rng = np.random.default_rng(seed)
  t = rng.integers(0, 50, (2, 2, 3, 2, 5)).astype(np.uint64)
  return EventScores(t, t // 2, 4, (1, -1), 8.0, fractions=fractions)


def test_event_scores_merge_with_and_without_fractions():
  plain = EventScores.merge([_events(0), _events(1)])
  assert plain.fractions is None
  np.testing.assert_array_equal(plain.weighted, _events(0).weighted + _events(1).weighted)
  a, b = _events(0, _fs(2)), _events(1, _fs(3))
  both = EventScores.merge([a, b])
  np.testing.assert_array_equal(both.weighted, plain.weighted)
  np.testing.assert_array_equal(both.fractions.sums, a.fractions.sums + b.fractions.sums)
  np.testing.assert_array_equal(both.brier, plain.brier)
  for parts in ([a, _events(1)], [_events(0), b]):
    with pytest.raises(ValueError, match="only some of the event scores carry fractions"):
      EventScores.merge(parts)
  assert EventScores(a.weighted, a.counts, 4, (1, -1), 8.0, None).fractions is None      # the positional arguments are what they were


# ---- the events row of the table, with a handle that records ------------------------------------------------------------------
class _Handle:
  def __init__(self, T=2, S=3, B=2, C=3, M=4):
    self.calls, self.T, self.S, self.B, self.C, self.M = [], T, S, B, C, M

  def ens_reserve(self, n):
    self.calls.append(("reserve", n))

  def ens_set_node_weight(self, w):
    self.calls.append(("weight",))

  def ens_event_set(self, thr, directions, wq):
    self.calls.append(("event_set", thr))

  def ens_fss_set(self, r_lat, r_lon, row_wq):
    self.calls.append(("fss_set", len(r_lat), np.shape(r_lon), len(row_wq)))

  def ens_event_score(self, truth):
    self.calls.append(("event_score", truth is None))
    t = np.full((self.T, self.B, self.C, 2, self.M + 1), 3, np.uint64)
    return t, t, np.zeros(self.T, np.uint64)

  def ens_fss_score(self):
    self.calls.append(("fss_score",))
    return np.ones((self.T, self.S, self.B, self.C, 4))

  def ens_score(self, truth, want_fields=False):
    self.calls.append(("score", truth is None))
    return np.ones((self.B, self.C, 6)), np.ones((self.B, self.C, self.M + 1), np.uint64)


def test_the_events_row_hands_the_plan_over_and_attaches_the_fractions():
  tgt = synthetic.make_example(lat=np.linspace(-90, 90, 5), lon=np.arange(8) * 45.0, batch=2, seed=1)[1]
  spec = EventSpec({"2m_temperature": np.array([1.0, 2.0])}, [1, -1], scales_km=[0, 5000.0, 10000.0])
  wq = (np.ones(40, np.uint32), 8.0)
  h = _Handle()
  st = verification.ScoredStore(h, 4, np.ones(40, np.float32), events=spec, thresholds=spec.packed(tgt), weight_q=wq)
  st.setup()
  assert [c[0] for c in h.calls] == ["reserve", "weight", "event_set", "fss_set"] and h.calls[-1] == ("fss_set", 3, (3, 5), 5)
  _, ev = st.score("truth")
  assert [c[0] for c in h.calls[4:]] == ["score", "event_score", "fss_score"]
  fr = ev.fractions
  assert isinstance(fr, FractionsScores) and fr.scales_km == spec.scales_km and fr.scale == 8.0 and fr.n_members == 4
  np.testing.assert_array_equal(fr.weight, np.full((2, 2, 3), 30, np.uint64))   # the total of the event table
  np.testing.assert_array_equal(fr.valid_weight, ev.valid_weight)
  # without scales: the calls of before, and no fractions
  h2 = _Handle()
  plain = EventSpec({"2m_temperature": np.array([1.0, 2.0])}, [1, -1])
  st2 = verification.ScoredStore(h2, 4, np.ones(40, np.float32), events=plain, thresholds=plain.packed(tgt), weight_q=wq)
  st2.setup()
  _, ev2 = st2.score("truth")
  assert [c[0] for c in h2.calls] == ["reserve", "weight", "event_set", "score", "event_score"] and ev2.fractions is None
  # a spec with scales whose windows nobody made is an error, not a silent skip
  bare = EventSpec({"2m_temperature": np.array([1.0, 2.0])}, [1, -1], scales_km=[100.0])
  st3 = verification.ScoredStore(_Handle(), 4, np.ones(40, np.float32), events=bare, thresholds="packed", weight_q=wq)
  with pytest.raises(ValueError, match="needs its windows"):
    st3.setup()


# ---- the ABI and the binding's own checks ------------------------------------------------------------------------------------------
NAMES = ("gc_ens_fss_set", "gc_ens_fss_score", "gc_ens_fss_fields")


def test_the_entries_are_declared_exported_and_bound():
  import gencast_flax_nnx_amd as pkg
  lib = _lib.load_library()
  declared = _declared("gencast_hip.h")
  for name in NAMES:
    assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES
    assert hasattr(_lib.NativeDenoiser, name[3:])
  assert pkg.FractionsScores is FractionsScores and "FractionsScores" in pkg.__all__
  assert lib.gc_abi_version() == 1 and lib.gc_num_kernel_classes() == 13
  assert b"gfx950" in lib.gc_build_info()                    # (tests/test_abi.py: built from the sources it sits beside)
  import os
  csrc = os.path.join(os.path.dirname(_lib.LIB_PATH))
  assert "gc_fss.hip" in open(os.path.join(csrc, "SOURCES")).read().split()


class _NoCall:
  def __getattr__(self, name):
    raise AssertionError(f"{name} must not be reached")


def test_binding_rejects_bad_arguments_before_the_c_call():
  nd = object.__new__(_lib.NativeDenoiser)
  nd._lib, nd._h = _NoCall(), None
  nd.cfg = _lib.GcConfig(128, 128, 2, 256, 1, 10, 6, 2, 32, 32, 16.0)
  nd.num_grid_nodes, nd._ens_members, nd._event_thresholds, nd._fss_scales = 312, 0, 0, 0
  ok_lat, ok_lon, ok_w = np.zeros(2, np.int32), np.zeros((2, 13), np.int32), np.ones(13, np.uint32)
  for r_lat, r_lon, w, n_lon in (
      (np.zeros(0, np.int32), np.zeros((0, 13), np.int32), ok_w, None),       # no scale
      (np.zeros(9, np.int32), np.zeros((9, 13), np.int32), ok_w, None),       # more than 8
      (ok_lat, np.zeros((3, 13), np.int32), ok_w, None),                      # r_lon of another S
      (ok_lat, np.zeros((2, 7), np.int32), ok_w, None),                       # 7 does not divide 312
      (ok_lat, ok_lon, ok_w, 25),                                             # 13 x 25 != G
      (np.array([0, -1], np.int32), ok_lon, ok_w, None),
      (ok_lat, np.full((2, 13), 12, np.int32), ok_w, None),                   # beyond (24 - 1) // 2
      (ok_lat, np.full((2, 13), -1, np.int32), ok_w, None),
      (ok_lat, ok_lon, np.zeros(13, np.uint32), None),
      (ok_lat, ok_lon, np.full(13, 2 ** 24, np.uint32), None),
      (ok_lat, ok_lon, np.ones(13), None),                                    # not integers
      (ok_lat, ok_lon, np.ones(12, np.uint32), None)):
    with pytest.raises(ValueError):
      nd.ens_fss_set(r_lat, r_lon, w, n_lon)
  with pytest.raises(_lib.GencastHipError, match="ens_fss_set"):
    nd.ens_fss_score()
  with pytest.raises(_lib.GencastHipError, match="ens_fss_set"):
    nd.ens_fss_fields(0, 0)
  nd._fss_scales = 2
  with pytest.raises(_lib.GencastHipError, match="ens_event_set"):
    nd.ens_fss_score()
  nd._event_thresholds = 3
  for t, s in ((3, 0), (-1, 0), (0, 2), (0, -1)):
    with pytest.raises(ValueError):
      nd.ens_fss_fields(t, s)
