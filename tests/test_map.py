"""The host side of the score maps: the definition of tests/map_reference.py, `ScoreMaps` and
`EventMaps` on reference planes, `MapSpec`, and the way a `ScoredStore` carries the unit.  No device, no library: the handles
record (`helpers.RecordingHandle`)."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import datasets, verification
from gencast_flax_nnx_amd.verification import EventMaps, EventSpec, MapSpec, ScoreMaps
from tests import event_reference as ER
from tests import map_reference as R
from tests import verification_reference as VR
from tests.helpers import RecordingHandle

G, B, C = 40, 2, 3


def _date(M, seed, offset=0.0):
  rng = np.random.default_rng(seed)
  scale = np.array([0.01, 1.0, 300.0], np.float32)
  members = (rng.standard_normal((M, G, B, C)).astype(np.float32) + np.float32(offset)) * scale
  truth = (rng.standard_normal((G, B, C)).astype(np.float32) + np.float32(offset)) * scale
  members[0, 3, 0, 1] = np.nan
  truth[7, 1, 2] = np.inf
  truth[11] = members[1, 11]                                  # the truth on a member
  members[2 % M, 13] = members[0, 13]                         # two members tie
  return members, truth


def _maps(dates, M, channels=None):
  sums, counts, _ = R.reference(dates, channels)
  return ScoreMaps(sums, counts, M, channels, len(dates))


def _ulps(a, b):
  return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


# ---- the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 8, 33, 50, 64])
def test_gap_form_equals_the_pair_loop_under_a_common_offset(M):
  """Members of 1e4 + N(0, 1): sum_{i<j} |x_i - x_j| pair by pair (tests/verification_reference.py) against the gap form,
  within M^2 2^-53 d -- every term of either is non-negative and exact differences of float32 values are exact in float64,
  so only the at most M^2 / 2 additions round.  The cancelling form sum_k (2k - M + 1) x_(k) has terms of size M 1e4 and
  would be wrong by orders of magnitude more."""
  rng = np.random.default_rng(M)
  x = (np.float32(1e4) + rng.standard_normal((M, 500)).astype(np.float32)).astype(np.float64)
  pair = VR.pair_sum_brute(x)
  gap = R.gap_sum(np.sort(x, axis=0))
  assert np.all(gap > 0.0)
  err = np.abs(gap - pair)
  print(f"M={M}: worst |gap - pair| / (M^2 2^-53 d) = {float(np.max(err / (M * M * 2.0 ** -53 * pair))):.3f}")
  assert np.all(err <= M * M * 2.0 ** -53 * pair)


def test_point_terms_are_those_of_the_ensemble_scores():
  """m, s2, ae and r are the operations of tests/verification_reference.py in the same order: the same bytes.  d differs in
  form (gaps against pairs), within the bound above."""
  M = 8
  members, truth = _date(M, 1)
  t, v = R.point_terms(members, truth), VR.point_terms(members, truth)
  ok = t["counted"]
  assert np.array_equal(ok, v["valid"]) and int((~ok).sum()) == 2
  y = truth.astype(np.float64)
  assert np.array_equal(t["e"][ok], (v["m"] - y)[ok]) and np.array_equal(t["s2"][ok], v["s2"][ok])
  assert np.array_equal(t["r"][ok], v["r"][ok])
  assert np.all(np.abs(t["ae"] - v["ae"])[ok] <= M * 2.0 ** -53 * v["ae"][ok])      # (sorted order against slot order)
  assert np.all(np.abs(t["d"] - v["d"])[ok] <= M * M * 2.0 ** -53 * v["d"][ok])


# ---- ScoreMaps on reference planes -------------------------------------------------------------------------------------------
def test_scores_from_the_planes():
  M = 5
  dates = [_date(M, s) for s in (1, 2, 3)]
  maps = _maps(dates, M)
  P, N = maps.sums, maps.counts.astype(np.float64)
  n0 = np.where(N[0] > 0, N[0], np.nan)
  assert maps.dates == 3 and int(N[0].min()) == 0 and int(N[0].max()) == 3          # (the planted NaN is on every date)
  assert np.array_equal(maps.crps, (P[3] - P[4] / 2) / n0, equal_nan=True)
  assert np.array_equal(maps.bias, P[0] / n0, equal_nan=True)
  assert np.array_equal(maps.rmse, np.sqrt(P[1] / n0), equal_nan=True)
  assert np.array_equal(maps.spread_skill_ratio, np.sqrt(6.0 / 5.0) * np.sqrt(P[2] / n0) / np.sqrt(P[1] / n0), equal_nan=True)
  assert np.array_equal(maps.crps_ensemble, (P[3] - 0.5 * 4.0 / 5.0 * P[4]) / n0, equal_nan=True)
  assert np.array_equal(maps.outlier_low, N[1] / n0, equal_nan=True) and np.array_equal(maps.outlier_high, N[2] / n0, equal_nan=True)
  # the standard error against the per-date values themselves
  c = np.stack([np.where(R.point_terms(*d)["counted"], R.point_terms(*d)["c"], np.nan) for d in dates])
  full = N[0] == 3
  want = np.sqrt(np.var(c[:, full], axis=0, ddof=1) / 3.0)
  np.testing.assert_allclose(maps.crps_stderr[full], want, rtol=1e-9)
  assert np.isnan(maps.crps[3, 0, 1]) and np.isnan(maps.crps_stderr[3, 0, 1])


def test_merge_is_the_reference_over_both_dates_byte_for_byte():
  M = 8
  a, b, c = _date(M, 4), _date(M, 5), _date(M, 6)
  both = ScoreMaps.merge([_maps([a], M), _maps([b], M)])
  ref = _maps([a, b], M)
  assert both.sums.tobytes() == ref.sums.tobytes() and both.counts.tobytes() == ref.counts.tobytes() and both.dates == 2
  three = ScoreMaps.merge([_maps([a], M), _maps([b], M), _maps([c], M)])      # a LEFT fold: ((a + b) + c)
  assert three.sums.tobytes() == _maps([a, b, c], M).sums.tobytes()
  sub = ScoreMaps.merge([_maps([a], M, [0, 2]), _maps([b], M, [0, 2])])
  assert sub.channels == (0, 2) and sub.sums.tobytes() == ref.sums[..., [0, 2]].tobytes()


def test_merge_refuses_what_does_not_add():
  a = _maps([_date(4, 1)], 4)
  with pytest.raises(ValueError, match="members, channels or shape"):
    ScoreMaps.merge([a, _maps([_date(5, 1)], 5)])
  with pytest.raises(ValueError, match="members, channels or shape"):
    ScoreMaps.merge([_maps([_date(4, 1)], 4, [0, 1]), _maps([_date(4, 1)], 4, [0, 2])])
  with pytest.raises(ValueError, match="members, channels or shape"):
    ScoreMaps.merge([a, ScoreMaps(a.sums[:, :5], a.counts[:, :5], 4)])
  with pytest.raises(ValueError, match="nothing to merge"):
    ScoreMaps.merge([])
  with pytest.raises(ValueError, match="must be"):
    ScoreMaps(a.sums, a.counts[:2], 4)


def test_scaled_against_recomputation_from_scaled_members():
  """Scales that are exact in float32 (powers of two, one negative), so the scaled members are the scaled values and the
  recomputation rounds where the original did: within 4 ulp (in fact equal).  A negative scale mirrors the ranks."""
  M = 6
  members, truth = _date(M, 9)
  a = np.array([4.0, -0.5, 0.125])
  shift = np.array([0.0, 0.0, 0.0], np.float32)
  scaled = _maps([(members * a.astype(np.float32) + shift, truth * a.astype(np.float32) + shift)], M)
  got = _maps([(members, truth)], M).scaled(a)
  assert np.array_equal(got.counts, scaled.counts)
  assert got.counts[1][..., 1].sum() > 0 and got.counts[2][..., 1].sum() > 0
  worst = float(np.nanmax(np.where(scaled.sums != 0.0, _ulps(got.sums, scaled.sums), 0.0)))
  print(f"scaled: worst distance {worst:.2f} ulp")
  assert worst <= 4.0
  with pytest.raises(ValueError, match="channel_scale"):
    got.scaled([1.0, 2.0])
  with pytest.raises(ValueError, match="non-zero"):
    got.scaled([1.0, 0.0, 2.0])


def test_region_of_one_date_against_the_column_sums():
  """sum_g w plane against `verification_reference.reference`: S0 .. S4 are the same per-point doubles (ae in another order of
  its M terms, d in another form) added in another order: (G + M^2 + 8) 2^-53 A_k, the bound of section 8c."""
  M = 8
  members, truth = _date(M, 12)
  w = np.random.default_rng(0).uniform(0.1, 2.0, G).astype(np.float32)
  ref = VR.reference(members, truth, w)
  reg = _maps([(members, truth)], M).region(w)
  err = np.abs(reg.sums - ref["sums"])
  tol = VR.sum_tolerance(ref, G, M)
  print(f"region: worst error / bound {float(np.max(err / tol)):.3f}")
  assert np.all(err <= tol)
  assert np.array_equal(reg.valid_points, ref["hist"].sum(-1))
  assert np.array_equal(reg.rank_histogram[..., 0], ref["hist"][..., 0]) and np.array_equal(reg.rank_histogram[..., -1], ref["hist"][..., -1])
  assert not reg.rank_histogram[..., 1:-1].any()
  np.testing.assert_allclose(reg.crps, VR.scores(ref, M)["crps"], rtol=1e-12)
  # a mask: the nodes outside it are not counted
  mask = (np.arange(G) % 2 == 0).astype(np.float64)
  half = _maps([(members, truth)], M).region(mask)
  assert np.array_equal(half.valid_points, R.point_terms(members, truth)["counted"][::2].sum(0))


def test_to_dataset_marks_the_points_that_never_counted():
  n_lat, n_lon = 5, 8
  template = datasets.Dataset({"t": datasets.Variable(("batch", "time", "level", "lat", "lon"), np.zeros((1, 1, 2, n_lat, n_lon))),
                               "z": datasets.Variable(("batch", "time", "lat", "lon"), np.zeros((1, 1, n_lat, n_lon)))},
                              {"lat": np.linspace(-90, 90, n_lat), "lon": np.arange(n_lon) * 45.0, "level": np.array([500.0, 850.0])})
  M = 4
  rng = np.random.default_rng(2)
  members = rng.standard_normal((M, G, B, C)).astype(np.float32)
  truth = rng.standard_normal((G, B, C)).astype(np.float32)
  truth[9, 1, 1] = np.nan                                    # channel 1 = t at 850
  ch = MapSpec(variables=["t"], levels=[850.0]).channels(template).tolist() + [2]
  maps = _maps([(members, truth)], M, [1, 2])
  assert ch == [1, 2]
  ds = maps.to_dataset(template, "crps")
  t, z = np.asarray(ds["t"].data), np.asarray(ds["z"].data)
  assert t.shape == (B, 1, 2, n_lat, n_lon) and z.shape == (B, 1, n_lat, n_lon)
  assert np.isnan(t[:, 0, 0]).all()                                               # level 500: not covered
  assert np.array_equal(t[:, 0, 1].reshape(B, G), maps.crps[..., 0].T, equal_nan=True)
  assert np.array_equal(z[:, 0].reshape(B, G), maps.crps[..., 1].T)
  assert np.isnan(np.asarray(maps.to_dataset(template, "bias")["t"].data)[1, 0, 1].reshape(G)[9]) and maps.counts[0, 9, 1, 0] == 0
  with pytest.raises(ValueError, match="not a score"):
    maps.to_dataset(template, "merge")


# ---- MapSpec -----------------------------------------------------------------------------------------------------------------
def _level_template():
  shape4, shape3 = (1, 1, 3, 4, 6), (1, 1, 4, 6)
  return datasets.Dataset(
      {"temperature": datasets.Variable(("batch", "time", "level", "lat", "lon"), np.zeros(shape4)),
       "2m_temperature": datasets.Variable(("batch", "time", "lat", "lon"), np.zeros(shape3)),
       "u_component_of_wind": datasets.Variable(("batch", "time", "level", "lat", "lon"), np.zeros(shape4))},
      {"lat": np.linspace(-90, 90, 4), "lon": np.arange(6) * 60.0, "level": np.array([250.0, 500.0, 850.0])})


def test_map_spec_channels_on_a_template_with_levels():
  """Stacking order: variables sorted by name -- 2m_temperature (0), temperature (1, 2, 3), u_component_of_wind (4, 5, 6)."""
  t = _level_template()
  assert [x[:] for x in datasets.channel_layout(t)] == [("2m_temperature", 0, 1), ("temperature", 1, 3), ("u_component_of_wind", 4, 3)]
  assert MapSpec().channels(t).tolist() == list(range(7)) and MapSpec().channels(t).dtype == np.int32
  assert MapSpec(variables=["u_component_of_wind", "2m_temperature"]).channels(t).tolist() == [0, 4, 5, 6]
  assert MapSpec(levels=[850.0, 250.0]).channels(t).tolist() == [0, 1, 3, 4, 6]           # a surface variable has no level: kept
  assert MapSpec(variables="temperature", levels=[500]).channels(t).tolist() == [2]


def test_map_spec_refusals():
  t = _level_template()
  with pytest.raises(ValueError, match="not a target variable"):
    MapSpec(variables=["vorticity"]).channels(t)
  with pytest.raises(ValueError, match="not one of the template's levels"):
    MapSpec(levels=[700.0]).channels(t)
  with pytest.raises(ValueError, match="distinct"):
    MapSpec(variables=["temperature", "temperature"])
  with pytest.raises(ValueError, match="non-empty"):
    MapSpec(variables=[])
  with pytest.raises(ValueError, match="distinct"):
    MapSpec(levels=[500.0, 500.0])
  flat = datasets.Dataset({"z": datasets.Variable(("batch", "lat", "lon"), np.zeros((1, 4, 6)))},
                          {"lat": np.linspace(-90, 90, 4), "lon": np.arange(6) * 60.0})
  with pytest.raises(ValueError, match="no 'level' coordinate"):
    MapSpec(levels=[500.0]).channels(flat)
  assert MapSpec(["a"], [1.0], True) == MapSpec(("a",), (1,), events=True) and MapSpec() != MapSpec(events=True)


# ---- EventMaps ---------------------------------------------------------------------------------------------------------------
def test_event_maps_from_reference_codes():
  """Three dates of code bytes (tests/event_reference.py) into the planes; the brier of the planes summed with the quantised
  weights against `EventScores.brier` of the merged tables: both are ratios of sums that are exact in float64 here, the
  table's numerator a sum of M + 1 rounded terms -- within 8 ulp."""
  M, T = 7, 2
  events = np.zeros((T, 5, G, B, C), np.uint32)
  tables = []
  for seed in (1, 2, 3):
    members, truth, w, thr, d = ER.data(M, G, B, C, seed=seed, T=T)
    truth[seed, 0, 1] = np.nan
    if seed == 1:                                             # one set of weights for every date
      wq, scale = verification.quantize_node_weights(w)
    ref = ER.tables(members, truth, thr, d, wq)
    R.accumulate_events(events, ref["code"])
    tables.append(verification.EventScores(ref["weighted"], ref["counts"], M, d, scale, ref["invalid"]))
  maps = EventMaps(events, M, d, None, 3)
  assert int(maps.valid_dates.min()) == 2 and int(maps.valid_dates.max()) == 3
  merged = verification.EventScores.merge(tables)
  reg = maps.region(wq)
  assert np.array_equal(reg["valid_weight"] / scale, merged.valid_weight)
  worst = float(np.max(_ulps(reg["brier"], merged.brier)))
  print(f"event maps: brier within {worst:.2f} ulp of the tables'")
  assert worst <= 8.0
  np.testing.assert_allclose(reg["base_rate"], merged.base_rate, rtol=1e-14)
  e = events.astype(np.float64)
  assert np.array_equal(maps.brier, (e[:, 2] - 2 * M * e[:, 3] + M * M * e[:, 4]) / (M * M * e[:, 0]))
  np.testing.assert_allclose(maps.brier, (e[:, 2] / M ** 2 - 2 * e[:, 3] / M + e[:, 4]) / e[:, 0], rtol=0, atol=1e-14)
  assert np.array_equal(maps.forecast_probability, e[:, 1] / (M * e[:, 0]))
  two = EventMaps.merge([maps, maps])
  assert np.array_equal(two.events, 2 * events) and two.dates == 6
  with pytest.raises(ValueError, match="differ"):
    EventMaps.merge([maps, EventMaps(events, M + 1, d)])


# ---- the store ---------------------------------------------------------------------------------------------------------------
class _Handle(RecordingHandle):
  def ens_map_set(self, channels, n_slots, n_event_thresholds):
    self._log("map_set", None if channels is None else tuple(int(c) for c in channels), n_slots, n_event_thresholds)
    self._map = (self.C if channels is None else len(channels), n_event_thresholds)

  def ens_map_accumulate(self, slot, truth):
    self._log("map_accumulate", slot, truth is None)

  def ens_map_accumulate_events(self, slot):
    self._log("map_accumulate_events", slot)

  def ens_map_download(self, slot, events=None):
    self._log("map_download", slot, events)
    Cs, T = self._map
    return (self._filled("map_download", (6, self.G, self.B, Cs)), self._filled("map_download", (3, self.G, self.B, Cs), np.uint32),
            self._filled("map_download", (T, 5, self.G, self.B, Cs), np.uint32) if events else None, np.array([2, 1], np.int64))

  def ens_map_reset(self, slot):
    self._log("map_reset", slot)


def _store(log, **kw):
  return verification.ScoredStore(_Handle("h", log, M=4, B=B, C=C, G=G), 4, np.ones(G, np.float32), **kw)


def test_a_store_sets_accumulates_downloads_and_resets_its_maps():
  log = []
  st = _store(log, maps=MapSpec(), map_channels=[0, 2], map_slots=3)
  st.setup()
  assert [c[1:] for c in log] == [("reserve", 4), ("weight",), ("map_set", (0, 2), 3, 0)]
  st.accumulate_maps(1, "truth")
  st.accumulate_maps(2)
  maps = st.download_maps(1)
  st.reset_maps()
  st.reset_maps(2)
  assert [c[1:] for c in log[3:]] == [("map_accumulate", 1, False), ("map_accumulate", 2, True), ("map_download", 1, False),
                                      ("map_reset", -1), ("map_reset", 2)]
  assert isinstance(maps, ScoreMaps) and maps.channels == (0, 2) and maps.n_members == 4 and maps.dates == 2
  assert maps.sums.shape == (6, G, B, 2)


def test_a_store_with_event_planes_adds_the_codes_behind_the_fields():
  spec = EventSpec({"x": np.zeros((2,))}, (+1, -1))
  thr = np.zeros((2, G, B, C), np.float32)
  log = []
  st = _store(log, maps=MapSpec(events=True), events=spec, thresholds=thr, weight_q=(np.ones(G, np.uint32), 1.0))
  st.setup()
  assert [c[1] for c in log] == ["reserve", "weight", "event_set", "map_set"] and log[-1][2:] == (None, 1, 2)
  st.accumulate_maps(0)
  maps, ev = st.download_maps(0)
  assert [c[1:] for c in log[4:]] == [("map_accumulate", 0, True), ("map_accumulate_events", 0), ("map_download", 0, True)]
  assert isinstance(ev, EventMaps) and ev.directions == (1, -1) and ev.events.shape == (2, 5, G, B, C) and ev.dates == 1
  assert maps.channels == (0, 1, 2)


def test_the_store_refusals():
  with pytest.raises(ValueError, match="two views must not add into one accumulator"):
    _store([], maps=MapSpec(), set_per_score=True)
  with pytest.raises(ValueError, match="need the store's EventSpec"):
    _store([], maps=MapSpec(events=True))
  with pytest.raises(TypeError, match="MapSpec"):
    _store([], maps="crps")
  with pytest.raises(ValueError, match="1..128"):
    _store([], maps=MapSpec(), map_slots=129)
  with pytest.raises(ValueError, match="needs map_channels"):
    _store([], maps=MapSpec(variables=["t"]))
  plain = _store([])
  for call in (lambda: plain.accumulate_maps(0), lambda: plain.download_maps(0), plain.reset_maps):
    with pytest.raises(ValueError, match="no MapSpec"):
      call()


def test_the_unit_stands_beside_the_scorer_table():
  assert verification.MAP_SCORER not in verification.SCORERS and verification.scorer("maps") is verification.MAP_SCORER
  assert verification.MAP_SCORER.word == "score maps" and verification.MAP_SCORER.score is None
