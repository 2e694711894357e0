"""Derived and pooled ensemble fields, host side: the two restatements of the definition in
tests/derive_reference.py against each other, `verification.DerivedSpec` (template, plan, channel_stats, window, every
ValueError) on config.TASK, and the merge rules of `EnsembleRolloutResult` with derived results.  The device side is
tests/test_gpu_derive.py and tests/test_gpu_derived_rollout.py."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import DerivedSpec, EventScores, config, datasets, losses, rollout, synthetic, verification
from tests import derive_reference as R

LAT13, LON24 = np.linspace(-90, 90, 13), np.arange(24) * 15.0
WIND = [("norm2", "10m_wind_speed", "10m_u_component_of_wind", "10m_v_component_of_wind"),
        ("norm2", "wind_speed", "u_component_of_wind", "v_component_of_wind"), ("copy", "2m_temperature")]


def _targets(lat=LAT13, lon=LON24, batch=2):
  return synthetic.make_example(lat=lat, lon=lon, batch=batch, seed=0)[1]


def _r_lon_cases(n_lat, n_lon, lat, lon):
  cap = (n_lon - 1) // 2
  return [np.zeros(n_lat, np.int32), np.full(n_lat, 2, np.int32), DerivedSpec.window(lat, lon, 2500.0)[1], np.full(n_lat, cap, np.int32)]


# ---- the two restatements of the definition ------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lat,n_lon", [(13, 24), (11, 15)])
def test_the_direct_and_the_separable_restatement_agree(n_lat, n_lon):
  lat, lon = np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)
  rng = np.random.default_rng(n_lon)
  G, B, C = n_lat * n_lon, 2, 5
  d = (rng.uniform(0.5, 20.0, (G, B, C)) * np.logspace(-2, 3, C)).astype(np.float32)     # positive: a sum has no cancellation
  d[rng.integers(0, G, 25), rng.integers(0, B, 25), 0] = np.nan
  d[[3, 50, 99], 1, 1] = [np.inf, -np.inf, np.inf]
  d[3 * n_lon:4 * n_lon, 0, 2] = np.nan                     # a whole latitude row
  d[:, 1, 3] = np.nan                                       # a whole column
  d[:, 0, 4] = np.nan
  d[5 * n_lon + 7, 0, 4] = 2.5                              # a finite centre, every neighbour NaN
  rw = losses.normalized_latitude_weights(lat)
  caps = _r_lon_cases(n_lat, n_lon, lat, lon)
  assert caps[2].max() == (n_lon - 1) // 2 and caps[2].min() < caps[2].max()
  for r_lat in (0, 1, 3, 12):
    for r_lon in caps:
      for pool in (R.MAX, R.MIN):
        a = R.pool_direct(d, pool, n_lat, n_lon, r_lat, r_lon, rw)
        b = R.pool_separable(d, pool, n_lat, n_lon, r_lat, r_lon, rw)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(np.isnan(a), ~np.isfinite(d))
        assert a[5 * n_lon + 7, 0, 4] == np.float32(2.5)
      a = R.pool_direct(d, R.MEAN, n_lat, n_lon, r_lat, r_lon, rw)
      b = R.pool_separable(d, R.MEAN, n_lat, n_lon, r_lat, r_lon, rw)
      np.testing.assert_array_equal(np.isnan(a), ~np.isfinite(d))
      ok = np.isfinite(a)
      assert np.all(np.abs(a[ok] - b[ok]) <= 1e-15 * np.abs(a[ok])), float(np.max(np.abs(a[ok] - b[ok]) / np.abs(a[ok])))
      assert a[5 * n_lon + 7, 0, 4] == 2.5
  # r = 0 in both directions is the identity on the finite points; MAX >= MEAN >= MIN on every window
  for pool in (R.MAX, R.MIN, R.MEAN):
    out = R.pool_direct(d, pool, n_lat, n_lon, 0, caps[0], rw)
    np.testing.assert_array_equal(out[np.isfinite(d)], d[np.isfinite(d)])
  hi, lo, mid = (R.pool_direct(d, p, n_lat, n_lon, 1, caps[1], rw) for p in (R.MAX, R.MIN, R.MEAN))
  ok = np.isfinite(d)
  assert np.all(hi[ok] >= mid[ok] * (1 - 1e-12)) and np.all(mid[ok] >= lo[ok] * (1 - 1e-12))


def test_derive_copies_bits_and_takes_the_norm_in_double():
  rng = np.random.default_rng(3)
  x = rng.standard_normal((40, 2, 4)).astype(np.float32)
  x[0, 0, 1] = np.nan
  x[1, 1, 2] = np.inf
  aff = np.array([[1, 0, 1, 0], [3.7, -12.5, 0.9, 4.0], [1, 0, 1, 0]], np.float64)
  d = R.derive(x, [0, 1, 0], [3, 1, 1], [0, 2, 0], aff)
  np.testing.assert_array_equal(d[..., 0].view(np.uint32), x[..., 3].view(np.uint32))
  np.testing.assert_array_equal(d[..., 2].view(np.uint32), x[..., 1].view(np.uint32))
  want = np.hypot(x[..., 1].astype(np.float64) * 3.7 - 12.5, x[..., 2].astype(np.float64) * 0.9 + 4.0)
  ok = np.isfinite(want)
  np.testing.assert_allclose(d[..., 1][ok], want[ok], rtol=2.0 ** -23)
  assert np.isnan(d[0, 0, 1]) and np.isinf(d[1, 1, 1])


# ---- DerivedSpec -----------------------------------------------------------------------------------------------------------
def test_template_plan_and_channel_stats_on_the_task():
  tgt = _targets()
  assert sorted(tgt.keys()) == sorted(config.TASK.target_variables)
  where = {n: (o, c) for n, o, c in datasets.channel_layout(tgt)}
  c_src = sum(c for _, c in where.values())
  spec = DerivedSpec(WIND)
  tmpl = spec.template(tgt)
  assert datasets.channel_layout(tmpl) == [("10m_wind_speed", 0, 1), ("2m_temperature", 1, 1), ("wind_speed", 2, 13)]
  assert tmpl["wind_speed"].dims == tgt["u_component_of_wind"].dims
  assert np.shape(tmpl["wind_speed"].data) == np.shape(tgt["u_component_of_wind"].data)
  assert tmpl["10m_wind_speed"].dims == tgt["10m_u_component_of_wind"].dims
  np.testing.assert_array_equal(tmpl.coords["lat"], tgt.coords["lat"])
  rng = np.random.default_rng(1)
  scale, loc = rng.uniform(0.5, 2.0, c_src), rng.uniform(-1.0, 1.0, c_src)
  plan = spec.plan(tgt, scale, loc)
  assert plan["c_src"] == c_src == 82 and plan["pool"] == 0 and plan["r_lon"] is None and plan["row_weight"] is None
  assert (plan["n_lat"], plan["n_lon"], plan["r_lat"]) == (13, 24, 0)
  u10, v10, t2 = where["10m_u_component_of_wind"][0], where["10m_v_component_of_wind"][0], where["2m_temperature"][0]
  u, v = where["u_component_of_wind"][0], where["v_component_of_wind"][0]
  np.testing.assert_array_equal(plan["op"], [1, 0] + [1] * 13)
  np.testing.assert_array_equal(plan["src_a"], [u10, t2] + list(range(u, u + 13)))
  np.testing.assert_array_equal(plan["src_b"][[0] + list(range(2, 15))], [v10] + list(range(v, v + 13)))
  np.testing.assert_array_equal(plan["affine"][0], [scale[u10], loc[u10], scale[v10], loc[v10]])
  np.testing.assert_array_equal(plan["affine"][1], [1, 0, 1, 0])
  for k in range(13):
    np.testing.assert_array_equal(plan["affine"][2 + k], [scale[u + k], loc[u + k], scale[v + k], loc[v + k]])
  sd, ld = spec.channel_stats(tgt, scale, loc)
  np.testing.assert_array_equal(sd, [1.0, scale[t2]] + [1.0] * 13)
  np.testing.assert_array_equal(ld, [0.0, loc[t2]] + [0.0] * 13)
  plain = spec.plan(tgt)                                     # no statistics: scale 1, location 0
  np.testing.assert_array_equal(plain["affine"], np.tile([1.0, 0.0, 1.0, 0.0], (15, 1)))
  # the reference applied to this plan: the norm of the un-normalised components
  x = rng.standard_normal((13 * 24, 2, c_src)).astype(np.float32)
  d = R.apply(x, plan)
  want = np.hypot(x[..., u10].astype(np.float64) * scale[u10] + loc[u10], x[..., v10].astype(np.float64) * scale[v10] + loc[v10])
  np.testing.assert_allclose(d[..., 0], want, rtol=2.0 ** -23)
  np.testing.assert_array_equal(d[..., 1], x[..., t2])
  # pooled plans: explicit radii, and a great-circle radius through window()
  r_lon = [11, 5, 3, 2, 2, 1, 1, 1, 2, 2, 3, 5, 11]
  pooled = DerivedSpec(WIND, pool="max", r_lat=1, r_lon=r_lon).plan(tgt, scale, loc)
  assert pooled["pool"] == 1 and pooled["r_lat"] == 1 and pooled["r_lon"].dtype == np.int32
  np.testing.assert_array_equal(pooled["r_lon"], r_lon)
  np.testing.assert_array_equal(pooled["row_weight"], losses.normalized_latitude_weights(tgt))
  by_radius = DerivedSpec([("copy", "2m_temperature")], pool="mean", radius_km=2500.0).plan(tgt)
  want_lat, want_lon = DerivedSpec.window(LAT13, LON24, 2500.0)
  assert by_radius["pool"] == 3 and by_radius["r_lat"] == want_lat
  np.testing.assert_array_equal(by_radius["r_lon"], want_lon)
  assert DerivedSpec([("copy", "2m_temperature")], pool="min", radius_km=0.0).plan(tgt)["pool"] == 2
  # every target variable copied: the identity map in packed order
  ident = DerivedSpec([("copy", v) for v in config.TASK.target_variables]).plan(tgt)
  np.testing.assert_array_equal(ident["src_a"], np.arange(82))
  assert not ident["op"].any()


def test_window_at_one_degree_and_500_km():
  lat, lon = np.linspace(-90, 90, 181), np.arange(360.0)
  r_lat, r_lon = DerivedSpec.window(lat, lon, 500.0)
  assert r_lat == 4 and r_lon.shape == (181,)
  assert r_lon[0] == r_lon[180] == 179 and r_lon[90] == 4
  assert np.all(np.diff(r_lon[:91]) <= 0) and np.all(r_lon == r_lon[::-1])          # narrowest at the equator, symmetric
  assert r_lon[30] == int(np.floor(500.0 / (111.195 * np.cos(np.deg2rad(60.0)))))    # 60 degrees south: 8
  assert DerivedSpec.window(lat, lon, 0.0)[0] == 0 and DerivedSpec.window(lat, lon, 0.0)[1][90] == 0
  assert DerivedSpec.window(lat, lon, 1e6)[1].max() == 179


def test_every_value_error():
  tgt = _targets()
  T2 = [("copy", "2m_temperature")]
  for bad in ([], [("copy",)], [("norm2", "w", "10m_u_component_of_wind")], [("hypot", "w", "a", "b")],
              [("copy", "2m_temperature"), ("norm2", "2m_temperature", "10m_u_component_of_wind", "10m_v_component_of_wind")]):
    with pytest.raises(ValueError):
      DerivedSpec(bad)
  with pytest.raises(ValueError, match="pool must be"):
    DerivedSpec(T2, pool="median", radius_km=100.0)
  with pytest.raises(ValueError, match="needs a pool"):
    DerivedSpec(T2, radius_km=100.0)
  with pytest.raises(ValueError, match="needs a pool"):
    DerivedSpec(T2, r_lat=1, r_lon=[0] * 13)
  with pytest.raises(ValueError, match="either radius_km or"):
    DerivedSpec(T2, pool="max")
  with pytest.raises(ValueError, match="either radius_km or"):
    DerivedSpec(T2, pool="max", radius_km=100.0, r_lat=1, r_lon=[0] * 13)
  with pytest.raises(ValueError, match="together"):
    DerivedSpec(T2, pool="max", r_lat=1)
  with pytest.raises(ValueError, match="radius_km"):
    DerivedSpec(T2, pool="max", radius_km=-1.0)
  with pytest.raises(ValueError, match="r_lat"):
    DerivedSpec(T2, pool="max", r_lat=-1, r_lon=[0] * 13)
  # against a template: unknown variables, unequal channel counts, windows that do not fit the grid, statistics
  with pytest.raises(ValueError, match="not a target variable"):
    DerivedSpec([("copy", "10m_wind_speed")]).plan(tgt)
  with pytest.raises(ValueError, match="not a target variable"):
    DerivedSpec([("norm2", "w", "10m_u_component_of_wind", "nope")]).template(tgt)
  unequal = DerivedSpec([("norm2", "w", "10m_u_component_of_wind", "v_component_of_wind")])
  for call in (unequal.template, unequal.plan, unequal.channel_stats):
    with pytest.raises(ValueError, match="channel by channel"):
      call(tgt)
  with pytest.raises(ValueError, match="one entry per latitude row"):
    DerivedSpec(T2, pool="max", r_lat=1, r_lon=[0] * 12).plan(tgt)
  with pytest.raises(ValueError, match="r_lon must lie in 0 .. 11"):
    DerivedSpec(T2, pool="max", r_lat=1, r_lon=[12] * 13).plan(tgt)
  with pytest.raises(ValueError, match="r_lon must lie in"):
    DerivedSpec(T2, pool="max", r_lat=1, r_lon=[-1] + [0] * 12).plan(tgt)
  with pytest.raises(ValueError, match="scale and loc"):
    DerivedSpec(T2).plan(tgt, np.ones(81), np.zeros(82))
  with pytest.raises(ValueError, match="scale and loc"):
    DerivedSpec(T2).channel_stats(tgt, np.ones(82), np.zeros(3))
  with pytest.raises(ValueError, match="at least two"):
    DerivedSpec.window([0.0], LON24, 100.0)


# ---- EnsembleRolloutResult with derived results ---------------------------------------------------------------------------
B, C, CD = 2, 6, 3


def _scores(rng, c, M):
  return verification.EnsembleScores(rng.uniform(1.0, 2.0, (B, c, 6)), rng.integers(0, 9, (B, c, M + 1)).astype(np.uint64), M)


def _result(seed, names=("wind", "smooth"), with_events=("wind",), horizon=2, M=3, derived=True):
  rng = np.random.default_rng(seed)
  scores = [_scores(rng, C, M) for _ in range(horizon)]
  parts = None
  if derived:
    parts = {}
    for name in names:
      ds = [_scores(rng, CD, M) for _ in range(horizon)]
      ev = None
      if name in with_events:
        ev = [EventScores(rng.integers(0, 99, (2, B, CD, 2, M + 1)).astype(np.uint64),
                          rng.integers(0, 9, (2, B, CD, 2, M + 1)).astype(np.uint64), M, [1, -1], 1024.0) for _ in range(horizon)]
      parts[name] = rollout.DerivedRolloutResult([s.scaled(np.full(CD, 2.0)) for s in ds], ds, ev, members=[[1]] * horizon)
  return rollout.EnsembleRolloutResult(scores, n_members=M, scores_normalized=scores, derived=parts)


def test_merge_adds_the_derived_results_name_by_name_and_lead_by_lead():
  a, b = _result(1), _result(2)
  m = a.merge(b)
  assert sorted(m.derived) == ["smooth", "wind"]
  for name in m.derived:
    for k in range(2):
      np.testing.assert_array_equal(m.derived[name].scores[k].sums, a.derived[name].scores[k].sums + b.derived[name].scores[k].sums)
      np.testing.assert_array_equal(m.derived[name].scores_normalized[k].rank_histogram,
                                    a.derived[name].scores_normalized[k].rank_histogram + b.derived[name].scores_normalized[k].rank_histogram)
    assert m.derived[name].members is None                   # members belong to one date
  np.testing.assert_array_equal(m.derived["wind"].events[1].weighted, a.derived["wind"].events[1].weighted + b.derived["wind"].events[1].weighted)
  assert m.derived["smooth"].events is None
  np.testing.assert_array_equal(m.scores[0].sums, a.scores[0].sums + b.scores[0].sums)
  twice = a.merge(a)
  np.testing.assert_array_equal(twice.derived["wind"].events[0].counts, 2 * a.derived["wind"].events[0].counts)


def test_merge_raises_when_the_derived_parts_do_not_match():
  a = _result(1)
  with pytest.raises(ValueError, match="only one of the two results carries derived"):
    a.merge(_result(2, derived=False))
  with pytest.raises(ValueError, match="only one of the two results carries derived"):
    _result(2, derived=False).merge(a)
  with pytest.raises(ValueError, match="derived names differ"):
    a.merge(_result(2, names=("wind", "other")))
  with pytest.raises(ValueError, match="derived names differ"):
    a.merge(_result(2, names=("wind",)))
  with pytest.raises(ValueError, match="carries events"):
    a.merge(_result(2, with_events=()))
  plain = _result(3, derived=False)
  assert plain.derived is None and plain.merge(_result(4, derived=False)).derived is None
