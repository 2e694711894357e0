"""Ensemble feature detection, host side: `verification.FeatureSpec` (template, plan, channel_stats,
every ValueError, thresholds and depths under a normalisation) on config.TASK, the restated definition in
tests/feature_reference.py on planted fields, `verification.link_tracks` on hand-made lists and the merge rule of an
`EnsembleRolloutResult` with features.  The device side is tests/test_gpu_feature.py and tests/test_gpu_feature_rollout.py."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import DerivedSpec, FeatureSpec, datasets, link_tracks, synthetic, verification
from tests import derive_reference as DR
from tests import feature_reference as R

LAT13, LON24 = np.linspace(-90, 90, 13), np.arange(24) * 15.0
MSLP = "mean_sea_level_pressure"


def _targets(batch=2):
  return synthetic.make_example(lat=LAT13, lon=LON24, batch=batch, seed=0)[1]


def _low(**kw):
  base = dict(variable=MSLP, kind="min", radius_km=2500.0, threshold=100500.0, ring_km=4000.0, depth=200.0, strike_km=1700.0)
  base.update(kw)
  return base


# ---- the spec -------------------------------------------------------------------------------------------------------------------
def test_template_plan_and_channel_stats():
  t = _targets()
  spec = FeatureSpec({"low": _low(), "jet": dict(variable="u_component_of_wind", level=3, kind="max", radius_km=(1, 2), strike_km=(0, 0))},
                     max_centres=7)
  assert spec.names == ["jet", "low"]                       # the channel order of the strike store: sorted
  tmpl = spec.template(t)
  assert [n for n, _, _ in datasets.channel_layout(tmpl)] == ["jet", "low"]
  for name in spec.names:
    assert tmpl[name].dims == ("batch", "time", "lat", "lon") and np.shape(tmpl[name].data) == (2, 1, 13, 24)
  plan = spec.plan(t)
  assert plan["c_src"] == 82 and plan["max_centres"] == 7 and (plan["n_lat"], plan["n_lon"]) == (13, 24)
  np.testing.assert_array_equal(plan["channel"], [43 + 3, 16])
  np.testing.assert_array_equal(plan["direction"], [1, -1])
  np.testing.assert_array_equal(plan["use_threshold"], [0, 1])
  assert plan["threshold"].dtype == np.float32 and plan["threshold"][1] == np.float32(100500.0)
  for key, km, d in (("r", 2500.0, 1), ("ring", 4000.0, 1), ("strike", 1700.0, 1)):
    r_lat, r_lon = DerivedSpec.window(LAT13, LON24, km)     # every radius is the window of gc_ens_derive
    assert plan[key + "_lat"][d] == r_lat
    np.testing.assert_array_equal(plan[key + "_lon"][d], r_lon)
  assert plan["r_lat"][0] == 1 and np.all(plan["r_lon"][0] == 2) and plan["ring_lat"][0] == 0 and plan["strike_lat"][0] == 0
  np.testing.assert_array_equal(plan["depth"], [0.0, 200.0])
  assert plan.names == ("jet", "low") and np.all(plan.scale == 1.0) and np.all(plan.loc == 0.0)
  scale, loc = spec.channel_stats(t)
  np.testing.assert_array_equal(scale, [1.0, 1.0])
  np.testing.assert_array_equal(loc, [0.0, 0.0])
  ev = spec.event_spec()
  assert ev.directions == (1,) and np.all(ev.packed(tmpl) == np.float32(0.5))


def test_thresholds_and_depths_take_the_normalisation():
  t = _targets()
  scale, loc = np.linspace(1.0, 9.0, 82), np.linspace(-4.0, 4.0, 82)
  scale[16], loc[16] = 1300.0, 101000.0
  plan = FeatureSpec({"low": _low(), "high": _low(kind="max", threshold=102000.0, depth=650.0)}).plan(t, scale, loc)
  np.testing.assert_array_equal(plan["channel"], [16, 16])
  assert plan["threshold"][0] == np.float32((102000.0 - 101000.0) / 1300.0)       # "high" sorts first
  assert plan["threshold"][1] == np.float32((100500.0 - 101000.0) / 1300.0)
  np.testing.assert_array_equal(plan["depth"], [650.0 / 1300.0, 200.0 / 1300.0])
  np.testing.assert_array_equal(plan.scale, [1300.0, 1300.0])
  np.testing.assert_array_equal(plan.loc, [101000.0, 101000.0])
  with pytest.raises(ValueError, match="shape"):
    FeatureSpec({"low": _low()}).plan(t, scale[:-1], loc)
  with pytest.raises(ValueError, match="positive"):
    FeatureSpec({"low": _low()}).plan(t, -scale, loc)


def test_every_value_error_of_the_spec():
  t = _targets()
  bad_at_init = [
      dict(low=_low(depth=None)),                            # ring without depth
      dict(low=_low(ring_km=None)),                          # depth without ring_km
      dict(low=_low(ring_km=2500.0)), dict(low=_low(ring_km=1000.0)),   # a ring not larger than the extremum radius
      dict(low=_low(kind="saddle")), dict(low=_low(radius_km=None)), dict(low=_low(strike_km=None)), dict(low=_low(radius_km=-1.0)),
      dict(low=_low(strike_km=np.inf)), dict(low=_low(threshold=np.nan)), dict(low=_low(depth=np.inf)), dict(low=_low(colour="red")),
      dict(low={k: v for k, v in _low().items() if k != "variable"}), dict(low=_low(radius_km=(1,))), dict(low=_low(radius_km=(-1, 2))),
      {}, {f"d{i}": _low() for i in range(9)}]               # none, and more than 8 detectors
  for detectors in bad_at_init:
    with pytest.raises(ValueError):
      FeatureSpec(detectors)
  for mc in (0, 1025, 2.5, True):
    with pytest.raises(ValueError, match="max_centres"):
      FeatureSpec({"low": _low()}, max_centres=mc)
  bad_on_template = [
      dict(variable="sea_ice", radius_km=500.0, strike_km=500.0),                             # unknown variable
      dict(variable="geopotential", radius_km=500.0, strike_km=500.0),                        # levels, none named
      dict(variable="geopotential", level=13, radius_km=500.0, strike_km=500.0),              # level out of range
      dict(variable="geopotential", level=-1, radius_km=500.0, strike_km=500.0),
      dict(variable=MSLP, level=1, radius_km=500.0, strike_km=500.0),
      _low(radius_km=(2, 1), ring_km=(2, 3)),                                                  # a ring no larger, as windows
      _low(radius_km=(1, np.full(12, 1))), _low(radius_km=(1, 12)), _low(strike_km=(1, -1))]   # r_lon: length, range
  for det in bad_on_template:
    spec = FeatureSpec({"x": det})
    with pytest.raises(ValueError):
      spec.plan(t)
  with pytest.raises(ValueError, match="not a target variable"):
    FeatureSpec({"x": bad_on_template[0]}).template(t)
  assert FeatureSpec({"z": dict(variable="geopotential", level=12, radius_km=500.0, strike_km=0.0)}).plan(t)["channel"][0] == 3 + 12


def test_a_store_takes_a_derive_plan_or_a_feature_plan():
  plan = FeatureSpec({"low": _low()}).plan(_targets())
  with pytest.raises(ValueError, match="not both"):
    verification.ScoredStore(object(), 2, plan={}, feature_plan=plan, source=object())
  with pytest.raises(ValueError, match="go together"):
    verification.ScoredStore(object(), 2, feature_plan=plan)
  with pytest.raises(ValueError, match="no feature plan"):
    verification.ScoredStore(object(), 2).centres()


# ---- the reference on planted fields ----------------------------------------------------------------------------------------------
N_LAT, N_LON = 13, 24


def _gaussian(i0, j0, depth, width=1.5):
  i, j = np.meshgrid(np.arange(N_LAT), np.arange(N_LON), indexing="ij")
  dj = np.minimum(np.abs(j - j0), N_LON - np.abs(j - j0))
  return (-depth * np.exp(-((i - i0) ** 2 + dj ** 2) / (2.0 * width ** 2))).astype(np.float32).reshape(-1)


def _plan(**det):
  base = dict(channel=0, direction=-1, r_lat=2, r_lon=np.full(N_LAT, 3), strike_lat=1, strike_lon=np.full(N_LAT, 2))
  base.update(det)
  return R.plan_of(1, N_LAT, N_LON, [base], max_centres=8)


def _detect(field, plan):
  count, node, value, strike = R.apply(field.reshape(-1, 1, 1), plan)
  return int(count[0, 0]), node[0, 0], value[0, 0], strike[:, 0, 0]


def test_a_gaussian_low_is_found_at_its_node_and_moves_with_the_longitude():
  plan = _plan(threshold=-1.0)
  field = _gaussian(6, 20, 8.0)
  for shift in range(0, 12):                                # 20 .. 23, then across longitude 0 to 7
    moved = np.roll(field.reshape(N_LAT, N_LON), shift, axis=1).reshape(-1)
    count, node, value, strike = _detect(moved, plan)
    assert count == 1 and node[0] == 6 * N_LON + (20 + shift) % N_LON and node[1] == -1
    assert value[0] == np.float32(-8.0) and value[1] == 0.0
    hit = np.flatnonzero(strike == 1.0)
    want = sorted(i * N_LON + (20 + shift + t) % N_LON for i in (5, 6, 7) for t in range(-2, 3))
    assert hit.tolist() == want and np.all((strike == 0.0) | (strike == 1.0))
  # the same low as a maximum of the negated field; and no centre above the threshold
  up = _plan(direction=1, threshold=1.0)
  count, node, value, _ = _detect(-field, up)
  assert count == 1 and node[0] == 6 * N_LON + 20 and value[0] == np.float32(8.0)
  assert _detect(field, _plan(threshold=-8.5))[0] == 0 and _detect(field, _plan(threshold=-8.0))[0] == 1


def test_two_lows_closer_than_the_radius_give_one_centre():
  near = _gaussian(6, 5, 8.0, 0.8) + _gaussian(6, 8, 6.0, 0.8)       # 3 columns apart: inside r_lon = 3
  far = _gaussian(6, 5, 8.0, 0.8) + _gaussian(6, 9, 6.0, 0.8)        # 4 apart: two windows, two centres
  plan = _plan(threshold=-1.0)
  count, node, _, _ = _detect(near, plan)
  assert count == 1 and node[0] == 6 * N_LON + 5
  count, node, _, _ = _detect(far, plan)
  assert count == 2 and node[:2].tolist() == [6 * N_LON + 5, 6 * N_LON + 9]
  # equal depths: the tie goes to the lower node index; a constant field has one centre per window, none with the rule off
  tie = np.minimum(_gaussian(6, 5, 8.0, 0.8), _gaussian(6, 8, 8.0, 0.8))
  count, node, _, _ = _detect(tie, plan)
  assert count == 1 and node[0] == 6 * N_LON + 5
  flat = _plan(r_lat=N_LAT, r_lon=np.full(N_LAT, (N_LON - 1) // 2 + 0))
  assert _detect(np.zeros(N_LAT * N_LON, np.float32), flat)[0] >= 1 and _detect(np.zeros(N_LAT * N_LON, np.float32), flat)[1][0] == 0


def test_a_shallow_low_fails_the_ring_test_and_a_deep_one_passes():
  ring = dict(ring_lat=3, ring_lon=np.full(N_LAT, 4), depth=2.0)
  shallow, deep = _gaussian(6, 10, 1.5, 1.0), _gaussian(6, 10, 5.0, 1.0)
  assert _detect(shallow, _plan())[0] >= 1                  # an extremum it is
  count, node, _, _ = _detect(deep, _plan(**ring))
  assert count == 1 and node[0] == 6 * N_LON + 10
  assert _detect(shallow, _plan(**ring))[0] == 0
  # the ring is the boundary only: a deeper value INSIDE it does not matter, one ON it does
  inside = deep.copy()
  inside[6 * N_LON + 12] = -4.0                             # inside the ring, above the centre
  assert _detect(inside, _plan(**ring))[0] == 1
  on_it = deep.copy()
  on_it[6 * N_LON + 14] = -3.5                              # on the ring (t = +4 in the centre's row): depth 1.5 < 2
  assert _detect(on_it, _plan(**ring))[0] == 0
  on_top = deep.copy()
  on_top[3 * N_LON + 8] = -3.5                              # on the ring's top row (i - 3, t = -2)
  assert _detect(on_top, _plan(**ring))[0] == 0
  nan_ring = deep.copy()
  for i in range(3, 10):                                    # a ring without a finite value fails
    for t in range(-4, 5):
      if abs(i - 6) == 3 or abs(t) == 4:
        nan_ring[i * N_LON + 10 + t] = np.nan
  assert _detect(nan_ring, _plan(**ring))[0] == 0


def test_the_strike_field_is_the_max_pool_of_the_indicator():
  rng = np.random.default_rng(3)
  field = (np.round(rng.standard_normal((N_LAT * N_LON, 2, 1)) * 4.0) / 4.0).astype(np.float32)
  field[[7, 100, 200], 0, 0] = np.nan
  field[150, 1, 0] = np.inf
  s_lon = DerivedSpec.window(LAT13, LON24, 2500.0)[1]
  plan = R.plan_of(1, N_LAT, N_LON, [dict(channel=0, direction=-1, r_lat=1, r_lon=np.full(N_LAT, 2), strike_lat=2, strike_lon=s_lon)])
  count, node, _, strike = R.apply(field, plan)
  flags = R.centres(field[..., 0], plan, 0)
  assert flags.sum(axis=0).tolist() == count[:, 0].tolist() and count.min() > 3
  pooled = DR.pool_direct(np.where(np.isfinite(field[..., 0]), flags.astype(np.float32), np.float32(np.nan)), DR.MAX, N_LAT, N_LON,
                          2, s_lon, np.ones(N_LAT))
  np.testing.assert_array_equal(strike[..., 0], pooled)
  assert np.isnan(strike[7, 0, 0]) and np.isnan(strike[150, 1, 0]) and np.isnan(strike).sum() == 4


# ---- tracks -----------------------------------------------------------------------------------------------------------------------
def _lead(*centres):
  return dict(lat=[c[0] for c in centres], lon=[c[1] for c in centres], value=[c[2] for c in centres], node=[c[3] for c in centres])


def test_link_tracks_on_a_crossing_pair():
  # two systems that swap their order in node index while moving: the link goes by distance, not by position in the list
  leads = [_lead((10.0, 100.0, 1.0, 5), (10.0, 110.0, 2.0, 6)), _lead((10.0, 108.0, 2.1, 3), (10.0, 102.0, 1.1, 9))]
  tracks = link_tracks(leads, 500.0)
  assert tracks == [[(0, 10.0, 100.0, 1.0), (1, 10.0, 102.0, 1.1)], [(0, 10.0, 110.0, 2.0), (1, 10.0, 108.0, 2.1)]]
  assert link_tracks(leads, 100.0) == [[(0, 10.0, 100.0, 1.0)], [(0, 10.0, 110.0, 2.0)], [(1, 10.0, 108.0, 2.1)], [(1, 10.0, 102.0, 1.1)]]
  # across longitude 0, and the great circle near a pole
  assert len(link_tracks([_lead((0.0, 359.0, 1.0, 0)), _lead((0.0, 1.0, 1.0, 0))], 250.0)) == 1
  assert len(link_tracks([_lead((89.0, 0.0, 1.0, 0)), _lead((89.0, 180.0, 1.0, 0))], 250.0)) == 1


def test_link_tracks_with_a_centre_that_vanishes():
  leads = [_lead((0.0, 10.0, 1.0, 1), (30.0, 50.0, 2.0, 2)), _lead((0.0, 12.0, 1.5, 4)), _lead(), _lead((0.0, 14.0, 1.7, 8))]
  tracks = link_tracks(leads, 400.0)
  assert tracks == [[(0, 0.0, 10.0, 1.0), (1, 0.0, 12.0, 1.5)], [(0, 30.0, 50.0, 2.0)], [(3, 0.0, 14.0, 1.7)]]
  assert link_tracks([], 100.0) == [] and link_tracks([_lead()], 100.0) == []
  with pytest.raises(ValueError):
    link_tracks(leads, -1.0)


def test_link_tracks_breaks_a_tie_in_distance_by_node_index():
  # one later centre, equally far from two earlier ones: the earlier centre with the lower node index takes it
  leads = [_lead((0.0, 12.0, 2.0, 7), (0.0, 8.0, 1.0, 3)), _lead((0.0, 10.0, 3.0, 5))]
  assert link_tracks(leads, 400.0) == [[(0, 0.0, 8.0, 1.0), (1, 0.0, 10.0, 3.0)], [(0, 0.0, 12.0, 2.0)]]
  # one earlier centre, two later ones equally far: the later centre with the lower node index
  leads = [_lead((0.0, 10.0, 3.0, 5)), _lead((0.0, 12.0, 2.0, 9), (0.0, 8.0, 1.0, 4))]
  assert link_tracks(leads, 400.0) == [[(0, 0.0, 10.0, 3.0), (1, 0.0, 8.0, 1.0)], [(1, 0.0, 12.0, 2.0)]]
  # and without node indices the position in the list stands in
  leads = [dict(lat=[0.0, 0.0], lon=[12.0, 8.0], value=[2.0, 1.0]), dict(lat=[0.0], lon=[10.0], value=[3.0])]
  assert link_tracks(leads, 400.0)[0] == [(0, 0.0, 12.0, 2.0), (1, 0.0, 10.0, 3.0)]


def test_a_rollout_result_merges_its_features_and_hides_them_when_there_are_none():
  from gencast_flax_nnx_amd import EnsembleRolloutResult, EnsembleScores, EventScores, FeatureRolloutResult
  rng = np.random.default_rng(0)
  score = lambda c: EnsembleScores(rng.uniform(1, 2, (1, c, 6)), rng.integers(1, 9, (1, c, 4)).astype(np.uint64), 3)
  event = lambda: EventScores(rng.integers(1, 9, (1, 1, 1, 2, 4)).astype(np.uint64), rng.integers(1, 9, (1, 1, 1, 2, 4)).astype(np.uint64),
                              3, [1], 64.0, np.zeros(1, np.uint64))

  def result(with_features=True):
    s = [score(1), score(1)]
    part = FeatureRolloutResult(s, s, [event(), event()], centres=[{}, {}], strike_probability=[None, None])
    return EnsembleRolloutResult([score(4), score(4)], n_members=3, scores_normalized=[score(4), score(4)],
                                 features={"low": part} if with_features else None)

  a, b, plain = result(), result(), result(False)
  assert plain.features is None and "features" not in vars(plain) and "features" in vars(a)
  m = a.merge(b).features["low"]
  for k in range(2):
    np.testing.assert_array_equal(m.scores[k].sums, a.features["low"].scores[k].sums + b.features["low"].scores[k].sums)
    np.testing.assert_array_equal(m.events[k].weighted, a.features["low"].events[k].weighted + b.features["low"].events[k].weighted)
  assert m.centres is None and m.strike_probability is None          # they belong to one date
  assert plain.merge(result(False)).features is None
  with pytest.raises(ValueError, match="only one of the two results carries features"):
    a.merge(plain)


def test_unpack_centres_in_physical_units():
  t = _targets(batch=1)
  scale, loc = np.ones(82), np.zeros(82)
  scale[16], loc[16] = 1300.0, 101000.0
  plan = FeatureSpec({"low": _low()}, max_centres=3).plan(t, scale, loc)
  count = np.array([[[2]], [[5]]], np.int32)               # [M + 1 = 2, B = 1, D = 1]; the truth has more than are listed
  node = np.array([[[[30, 100, -1]]], [[[0, 23, 311]]]], np.int32)
  value = np.array([[[[-1.0, 0.5, 0.0]]], [[[0.0, 1.0, 2.0]]]], np.float32)
  out = verification.unpack_centres(count, node, value, plan)
  members, truth = verification.split_centres(out)
  m0, tr = members["low"][0][0], truth["low"][0]
  assert m0["count"] == 2 and m0["node"].tolist() == [30, 100]
  np.testing.assert_array_equal(m0["lat"], LAT13[[1, 4]])
  np.testing.assert_array_equal(m0["lon"], LON24[[6, 4]])
  np.testing.assert_array_equal(m0["value"], [101000.0 - 1300.0, 101000.0 + 650.0])
  assert tr["count"] == 5 and tr["node"].tolist() == [0, 23, 311] and tr["lat"].tolist() == [-90.0, -90.0, 90.0]
