"""Derived fields across levels and along the grid, host side: `verification.DerivedSpec` with the sum,
norm, vorticity and divergence forms (validation, template, plan tables, channel_stats, the helpers) on config.TASK, and the
properties of the definition restated in tests/derive_expr_reference.py.  The device side is tests/test_gpu_derive_expr.py
and tests/test_gpu_derive_expr_rollout.py."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import DerivedSpec, datasets, synthetic
from tests import derive_expr_reference as X
from tests import derive_reference as R

LAT13, LON24 = np.linspace(-90, 90, 13), np.arange(24) * 15.0
LEVELS = (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)
U, V, Q, Z = "u_component_of_wind", "v_component_of_wind", "specific_humidity", "geopotential"
LEGACY_KEYS = ["affine", "c_src", "n_lat", "n_lon", "op", "pool", "r_lat", "r_lon", "row_weight", "src_a", "src_b"]
EXPR_KEYS = sorted(LEGACY_KEYS + ["scale", "loc", "term_start", "term_coef", "term_a", "term_b", "coslat", "inv_rcos", "inv_dphi",
                                  "inv_2dlam", "pole_row"])


def _targets(lat=LAT13, lon=LON24, batch=2):
  return synthetic.make_example(lat=lat, lon=lon, batch=batch, seed=0)[1]


def _where(tgt):
  return {n: o for n, o, _ in datasets.channel_layout(tgt)}


# ---- spec validation ----------------------------------------------------------------------------------------------------------
def test_every_value_error_of_the_new_forms():
  tgt = _targets()
  for bad, match in (([("sum", "s")], "an output must be"),
                     ([("sum", "s", [])], "1 .. 64 terms"),
                     ([("sum", "s", [(1.0, (Z, 0))] * 65)], "1 .. 64 terms"),
                     ([("sum", "s", 3.0)], "a term list is a sequence"),
                     ([("sum", "s", [(1.0,)])], "a term is"),
                     ([("sum", "s", [(np.nan, (Z, 0))])], "not a finite number"),
                     ([("sum", "s", [(np.inf, (Z, 0))])], "not a finite number"),
                     ([("sum", "s", [("one", (Z, 0))])], "not a finite number"),
                     ([("sum", "s", [(1.0, Z)])], "a factor is"),
                     ([("sum", "s", [(1.0, (Z, 0.5))])], "a factor is"),
                     ([("sum", "s", [(1.0, (Z, True))])], "a factor is"),
                     ([("norm", "s", [(1.0, (Z, 0))])], "an output must be"),
                     ([("norm", "s", [(1.0, (Z, 0))], [])], "1 .. 64 terms"),
                     ([("vorticity", "z", U)], "an output must be"),
                     ([("vorticity", "z", U, V, 0.5)], "the level must be an index"),
                     ([("divergence", "z", U, V, 1, 2)], "an output must be"),
                     ([("curl", "z", U, V)], "an output must be"),
                     ([("sum", "s", [(1.0, (Z, 0))]), ("vorticity", "s", U, V)], "distinct")):
    with pytest.raises(ValueError, match=match):
      DerivedSpec(bad)
  for bad, match in (([("sum", "s", [(1.0, ("nope", 0))])], "'nope' is not a target variable"),
                     ([("sum", "s", [(1.0, (Z, 0), ("nope", 0))])], "'nope' is not a target variable"),
                     ([("sum", "s", [(1.0, (Z, 13))])], "level 13 of 'geopotential' outside 0 .. 12"),
                     ([("sum", "s", [(1.0, (Z, -1))])], "outside 0 .. 12"),
                     ([("sum", "s", [(1.0, (Z, None))])], "has 13 levels: name one"),
                     ([("sum", "s", [(1.0, ("2m_temperature", 1))])], "outside 0 .. 0"),
                     ([("vorticity", "z", U, "nope")], "'nope' is not a target variable"),
                     ([("vorticity", "z", U, V, 13)], "outside 0 .. 12"),
                     ([("divergence", "z", U, "10m_v_component_of_wind")], "divergence is taken channel by channel")):
    spec = DerivedSpec(bad)
    for call in (spec.template, spec.plan, spec.channel_stats):
      with pytest.raises(ValueError, match=match):
        call(tgt)
  many = DerivedSpec([("sum", f"s{k:02d}", [(1.0, (Z, 0))] * 64) for k in range(17)])            # 1088 terms in the plan
  with pytest.raises(ValueError, match="at most 1024"):
    many.plan(tgt)
  # the grid of vorticity / divergence
  vort = DerivedSpec([("vorticity", "z", U, V, 10)])
  with pytest.raises(ValueError, match="at least 3 longitudes"):
    vort.plan(_targets(lon=np.array([0.0, 180.0])))
  with pytest.raises(ValueError, match="equally spaced latitudes"):
    vort.plan(_targets(lat=np.array([-90.0, -50.0, -20.0, 0.0, 30.0, 60.0, 90.0])))
  with pytest.raises(ValueError, match="equally spaced longitudes round the whole circle"):
    vort.plan(_targets(lon=np.arange(12) * 15.0))
  with pytest.raises(ValueError, match="equally spaced longitudes"):
    vort.plan(_targets(lon=np.array([0.0, 90.0, 200.0, 270.0])))
  DerivedSpec([DerivedSpec.select("z500", Z, 7)]).plan(_targets(lon=np.array([0.0, 180.0])))   # the term sums need no grid
  with pytest.raises(ValueError, match="ascending or descending"):
    DerivedSpec.pressure_weights([1000, 850, 900])
  with pytest.raises(ValueError, match="at least two"):
    DerivedSpec.pressure_weights([1000])


# ---- plan tables --------------------------------------------------------------------------------------------------------------
def test_a_legacy_spec_gives_the_plan_it_always_gave():
  tgt = _targets()
  rng = np.random.default_rng(1)
  scale, loc = rng.uniform(0.5, 2.0, 82), rng.uniform(-1.0, 1.0, 82)
  spec = DerivedSpec([("norm2", "wind_speed", U, V), ("copy", "2m_temperature")], pool="max", radius_km=2500.0)
  assert spec.legacy
  plan = spec.plan(tgt, scale, loc)
  assert sorted(plan) == LEGACY_KEYS
  w = _where(tgt)
  np.testing.assert_array_equal(plan["op"], [0] + [1] * 13)
  assert plan["op"].dtype == plan["src_a"].dtype == plan["src_b"].dtype == np.int32
  np.testing.assert_array_equal(plan["src_a"], [w["2m_temperature"]] + list(range(w[U], w[U] + 13)))
  np.testing.assert_array_equal(plan["src_b"], [w["2m_temperature"]] + list(range(w[V], w[V] + 13)))
  np.testing.assert_array_equal(plan["affine"][0], [1, 0, 1, 0])
  for k in range(13):
    np.testing.assert_array_equal(plan["affine"][1 + k], [scale[w[U] + k], loc[w[U] + k], scale[w[V] + k], loc[w[V] + k]])
  assert (plan["c_src"], plan["pool"], plan["n_lat"], plan["n_lon"]) == (82, 1, 13, 24)
  want_lat, want_lon = DerivedSpec.window(LAT13, LON24, 2500.0)
  assert plan["r_lat"] == want_lat
  np.testing.assert_array_equal(plan["r_lon"], want_lon)
  # the reference of the legacy ops reads the plan as it is, and the new reference agrees with it on those ops
  x = rng.standard_normal((13 * 24, 2, 82)).astype(np.float32)
  unpooled = DerivedSpec([("norm2", "wind_speed", U, V), ("copy", "2m_temperature")]).plan(tgt, scale, loc)
  np.testing.assert_array_equal(X.derive(x, unpooled)[0], R.derive(x, unpooled["op"], unpooled["src_a"], unpooled["src_b"], unpooled["affine"]))


def test_plan_template_and_channel_stats_of_the_new_forms():
  tgt = _targets()
  w = _where(tgt)
  rng = np.random.default_rng(2)
  scale, loc = rng.uniform(0.5, 2.0, 82), rng.uniform(-1.0, 1.0, 82)
  spec = DerivedSpec([DerivedSpec.ivt("ivt", Q, U, V, LEVELS), DerivedSpec.thickness("thick", Z, 5, 7), ("vorticity", "vort850", U, V, 10),
                      ("divergence", "div", U, V), ("copy", "2m_temperature"), ("norm2", "wind10", "10m_u_component_of_wind", "10m_v_component_of_wind"),
                      DerivedSpec.select("z500", Z, 7), DerivedSpec.shear("shear", U, V, 3, 10), DerivedSpec.column_integral("tcwv", Q, LEVELS)])
  assert not spec.legacy
  tmpl = spec.template(tgt)
  assert datasets.channel_layout(tmpl) == [("2m_temperature", 0, 1), ("div", 1, 13), ("ivt", 14, 1), ("shear", 15, 1), ("tcwv", 16, 1),
                                           ("thick", 17, 1), ("vort850", 18, 1), ("wind10", 19, 1), ("z500", 20, 1)]
  flat = ("batch", "time", "lat", "lon")
  assert tmpl["div"].dims == tgt[U].dims and np.shape(tmpl["div"].data) == np.shape(tgt[U].data)
  for name in ("ivt", "shear", "tcwv", "thick", "vort850", "z500"):
    assert tmpl[name].dims == flat and np.shape(tmpl[name].data) == (2, 1, 13, 24)
  np.testing.assert_array_equal(tmpl.coords["lat"], tgt.coords["lat"])
  plan = spec.plan(tgt, scale, loc)
  assert sorted(plan) == EXPR_KEYS
  np.testing.assert_array_equal(plan["op"], [0] + [5] * 13 + [3, 3, 2, 2, 4, 1, 2])
  np.testing.assert_array_equal(plan["src_a"][:14], [w["2m_temperature"]] + list(range(w[U], w[U] + 13)))
  np.testing.assert_array_equal(plan["src_b"][1:14], list(range(w[V], w[V] + 13)))
  assert (plan["src_a"][18], plan["src_b"][18]) == (w[U] + 10, w[V] + 10)                       # vort850
  assert (plan["src_a"][19], plan["src_b"][19]) == (w["10m_u_component_of_wind"], w["10m_v_component_of_wind"])
  np.testing.assert_array_equal(plan["affine"][19], [scale[0], loc[0], scale[1], loc[1]])
  np.testing.assert_array_equal(plan["scale"], scale)
  np.testing.assert_array_equal(plan["loc"], loc)
  # the term table: ivt 13 + 13, shear 2 + 2, tcwv 13, thick 2, z500 1, in channel order
  ts = plan["term_start"]
  assert ts.shape == (21, 3) and ts.dtype == np.int32 and not ts[[0, 1, 13, 18, 19]].any()
  np.testing.assert_array_equal(ts[14:18], [[0, 13, 26], [26, 28, 30], [30, 43, 43], [43, 45, 45]])
  np.testing.assert_array_equal(ts[20], [45, 46, 46])
  assert plan["term_coef"].shape == plan["term_a"].shape == plan["term_b"].shape == (46,)
  wts = DerivedSpec.pressure_weights(LEVELS)
  np.testing.assert_array_equal(plan["term_coef"][:26], np.concatenate([wts, wts]))
  np.testing.assert_array_equal(plan["term_a"][:26], list(range(w[Q], w[Q] + 13)) * 2)
  np.testing.assert_array_equal(plan["term_b"][:26], list(range(w[U], w[U] + 13)) + list(range(w[V], w[V] + 13)))
  np.testing.assert_array_equal(plan["term_coef"][26:30], [1, -1, 1, -1])
  np.testing.assert_array_equal(plan["term_a"][26:30], [w[U] + 3, w[U] + 10, w[V] + 3, w[V] + 10])
  np.testing.assert_array_equal(plan["term_b"][26:], -1)
  np.testing.assert_array_equal(plan["term_coef"][43:45], [1 / 9.80665, -1 / 9.80665])
  np.testing.assert_array_equal(plan["term_a"][43:], [w[Z] + 5, w[Z] + 7, w[Z] + 7])
  # the row tables are those of the definition
  for k, v in X.row_tables(LAT13, LON24).items():
    np.testing.assert_array_equal(plan[k], v, err_msg=k)
  np.testing.assert_array_equal(plan["pole_row"], [1] + [0] * 11 + [1])
  assert plan["coslat"][0] == plan["coslat"][12] == 0.0 and plan["pole_row"].dtype == np.int32
  assert plan["inv_2dlam"] == 1.0 / (2.0 * np.deg2rad(15.0))
  np.testing.assert_allclose(plan["inv_dphi"][[0, 1, 12]], [1 / np.deg2rad(15.0), 1 / np.deg2rad(30.0), 1 / np.deg2rad(15.0)], rtol=1e-14)
  np.testing.assert_allclose(plan["inv_rcos"][6], 1.0 / 6371000.0, rtol=1e-15)
  # descending latitudes: negative spacings, the same magnitudes
  down = spec.plan(_targets(lat=LAT13[::-1].copy()), scale, loc)
  np.testing.assert_allclose(down["inv_dphi"], -plan["inv_dphi"][::-1], rtol=1e-14)
  # without vorticity / divergence no row table is made
  sums = DerivedSpec([DerivedSpec.select("z500", Z, 7), ("copy", "2m_temperature")]).plan(tgt)
  assert sorted(sums) == EXPR_KEYS and all(sums[k] is None for k in ("coslat", "inv_rcos", "inv_dphi", "inv_2dlam", "pole_row"))
  np.testing.assert_array_equal(sums["scale"], np.ones(82))
  # in physical units already: (1, 0), but for the copy
  sd, ld = spec.channel_stats(tgt, scale, loc)
  np.testing.assert_array_equal(sd, [scale[w["2m_temperature"]]] + [1.0] * 20)
  np.testing.assert_array_equal(ld, [loc[w["2m_temperature"]]] + [0.0] * 20)
  # a pooled plan of the new forms carries the window as a legacy one does
  pooled = DerivedSpec([DerivedSpec.select("z500", Z, 7)], pool="mean", radius_km=2500.0).plan(tgt)
  assert pooled["pool"] == 3 and pooled["row_weight"].shape == (13,) and pooled["r_lon"].dtype == np.int32


def test_the_helpers_build_the_tuples():
  np.testing.assert_allclose(DerivedSpec.pressure_weights([1000, 850, 500]), np.array([7500.0, 25000.0, 17500.0]) / 9.80665, rtol=1e-15)
  np.testing.assert_allclose(DerivedSpec.pressure_weights([500, 850, 1000]), np.array([17500.0, 25000.0, 7500.0]) / 9.80665, rtol=1e-15)
  np.testing.assert_allclose(DerivedSpec.pressure_weights([1000, 850, 500], g=10.0), [750.0, 2500.0, 1750.0], rtol=1e-15)
  assert DerivedSpec.select("z500", Z, 7) == ("sum", "z500", [(1.0, (Z, 7))])
  assert DerivedSpec.thickness("t", Z, 5, 7, g=10.0) == ("sum", "t", [(0.1, (Z, 5)), (-0.1, (Z, 7))])
  assert DerivedSpec.shear("s", U, V, 3, 10) == ("norm", "s", [(1.0, (U, 3)), (-1.0, (U, 10))], [(1.0, (V, 3)), (-1.0, (V, 10))])
  name, out, terms = DerivedSpec.column_integral("tcwv", Q, [1000, 850, 500])
  assert (name, out) == ("sum", "tcwv") and [t[1] for t in terms] == [(Q, 0), (Q, 1), (Q, 2)]
  np.testing.assert_allclose([t[0] for t in terms], np.array([7500.0, 25000.0, 17500.0]) / 9.80665, rtol=1e-15)
  _, _, t1, t2 = DerivedSpec.ivt("ivt", Q, U, V, [1000, 850, 500])
  assert [t[1:] for t in t1] == [((Q, k), (U, k)) for k in range(3)] and [t[1:] for t in t2] == [((Q, k), (V, k)) for k in range(3)]
  assert [t[0] for t in t1] == [t[0] for t in t2] == [t[0] for t in terms]
  assert DerivedSpec([DerivedSpec.ivt("ivt", Q, U, V, LEVELS)]).names == ["ivt"]


# ---- properties of the reference ------------------------------------------------------------------------------------------------
def _rotation(n_lat, n_lon, u0=40.0):
  """Solid-body rotation u = U0 cos(lat), v = 0 on a grid with poles, as a float32 field [G, 1, 2], and the plan of its
  vorticity and divergence."""
  lat, lon = np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)
  u = u0 * np.cos(np.deg2rad(lat))[:, None] * np.ones(n_lon)
  x = np.stack([u, np.zeros_like(u)], axis=-1).reshape(n_lat * n_lon, 1, 2).astype(np.float32)
  plan = X.raw_plan(2, [("vorticity", 0, 1), ("divergence", 0, 1)], n_lat, n_lon, lat=lat, lon=lon)
  return lat, x, plan


def test_solid_body_rotation_has_vorticity_two_u0_sin_lat_over_r_and_no_divergence():
  u0, worst = 40.0, []
  for n_lat in (25, 49, 97):
    lat, x, plan = _rotation(n_lat, 16, u0)
    d, _ = X.derive(x, plan)
    g = d.reshape(n_lat, 16, 2).astype(np.float64)
    want = 2.0 * u0 * np.sin(np.deg2rad(lat)) / X.EARTH_RADIUS_M
    np.testing.assert_array_equal(g[..., 1], 0.0)              # v = 0 and u has no zonal gradient: exactly none
    inner = slice(2, n_lat - 2)                                # centred rows whose neighbours are centred too
    worst.append(np.abs(g[inner, :, 0] - want[inner, None]).max())
    assert worst[-1] < 0.05 * np.abs(want).max() * (25.0 / n_lat) ** 2 * 4
    # a pole row is the zonal mean of its neighbour: one value, finite
    for i, ia in ((0, 1), (n_lat - 1, n_lat - 2)):
      assert np.all(g[i, :, 0] == g[i, 0, 0]) and np.isfinite(g[i, 0, 0])
      np.testing.assert_allclose(g[i, 0, 0], g[ia, :, 0].mean(), rtol=2.0 ** -22)
  # halving the spacing cuts the interior error by more than 3 (second order: 4), until float32 inputs show
  assert worst[0] / worst[1] > 3.0 and worst[1] / worst[2] > 3.0, worst


def test_a_pole_row_is_the_zonal_mean_of_the_adjacent_rows_double_results():
  n_lat, n_lon = 9, 12
  lat, lon = np.linspace(90, -90, n_lat), np.arange(n_lon) * 30.0           # descending
  rng = np.random.default_rng(4)
  x = rng.standard_normal((n_lat * n_lon, 2, 3)).astype(np.float32)
  plan = X.raw_plan(3, [("vorticity", 0, 2), ("divergence", 2, 1)], n_lat, n_lon, scale=[2.0, 0.5, 3.0], loc=[1.0, -1.0, 0.25], lat=lat, lon=lon)
  d, bound = X.derive(x, plan)
  for j, vort in ((0, True), (1, False)):
    r, _ = X.curl(x, plan, vort, plan["src_a"][j], plan["src_b"][j])
    r = r.reshape(n_lat, n_lon, 2)
    for i, ia in ((0, 1), (n_lat - 1, n_lat - 2)):
      s = np.zeros(2)
      for l in range(n_lon):
        s = s + r[ia, l]
      np.testing.assert_array_equal(d.reshape(n_lat, n_lon, 2, 2)[i, :, :, j], np.broadcast_to((s / n_lon).astype(np.float32), (n_lon, 2)))
  assert np.isfinite(d).all() and np.all(bound > 0)
  x[1 * n_lon + 5, 0, 2] = np.nan                               # a NaN next to the pole, in the field differenced along the row
  d2, _ = X.derive(x, plan)                                     # of both ops: the whole pole row of that batch entry
  g = d2.reshape(n_lat, n_lon, 2, 2)
  assert np.isnan(g[0, :, 0, :]).all() and np.isfinite(g[0, :, 1, :]).all() and np.isfinite(g[n_lat - 1]).all()
  assert np.isnan(g[1, :, 0, :]).sum() == 4                     # in the row itself: the two neighbours, in both ops


def test_the_term_sums_of_the_reference():
  rng = np.random.default_rng(5)
  x = rng.standard_normal((30, 2, 4)).astype(np.float32)
  scale, loc = np.array([2.0, 0.5, 3.0, 1.5]), np.array([1.0, -1.0, 0.25, 0.0])
  plan = X.raw_plan(4, [("sum", [(1.0, 2, -1)]), ("sum", [(2.0, 0, 1), (-3.0, 2, -1)]), ("norm", [(1.0, 0, -1)], [(1.0, 1, -1)]), ("copy", 3)],
                    5, 6, scale=scale, loc=loc)
  d, bound = X.derive(x, plan)
  p = x.astype(np.float64) * scale + loc
  np.testing.assert_array_equal(d[..., 0], p[..., 2].astype(np.float32))               # one unit term is p(c)
  np.testing.assert_array_equal(d[..., 1], (2.0 * p[..., 0] * p[..., 1] + -3.0 * p[..., 2]).astype(np.float32))
  np.testing.assert_allclose(d[..., 2], np.hypot(p[..., 0], p[..., 1]), rtol=2.0 ** -23)
  np.testing.assert_array_equal(d[..., 3].view(np.uint32), x[..., 3].view(np.uint32))
  assert np.all(bound[..., 3] == 0) and np.all(bound[..., :3] >= np.spacing(np.abs(d[..., :3])))
  assert np.all(bound[..., :3] <= 1.001 * np.spacing(np.abs(d[..., :3])) + 1e-14)       # the double chain adds next to nothing
  x[3, 0, 0], x[4, 1, 2] = np.nan, np.inf                       # IEEE: NaN and inf propagate
  d, _ = X.derive(x, plan)
  assert np.isnan(d[3, 0, 1]) and np.isnan(d[3, 0, 2]) and d[4, 1, 0] == np.inf and d[4, 1, 1] == -np.inf and np.isfinite(d[3, 0, 0])


# ---- through a rollout on recording handles -----------------------------------------------------------------------------------
def test_a_rollout_hands_the_plan_of_the_new_forms_to_its_views_as_it_is():
  """`EnsembleRollout.run(derived=...)`, the climatology view and a window over the view on `helpers.RecordingHandle`s (the
  2 x 3 grid of tests/test_rollout_call_sequence.py): every `ens_derive_set` gets the plan dict of `DerivedSpec.plan`, new keys
  included, and nothing else about the calls differs from an entry of legacy forms."""
  from gencast_flax_nnx_amd import WindowSpec
  from tests import test_rollout_call_sequence as S
  new = DerivedSpec([("vorticity", "zeta", "u", "v"), DerivedSpec.thickness("thick", "z", 0, 1)])
  old = DerivedSpec([("norm2", "zeta", "u", "v"), ("copy", "u")])
  climatology = lambda k: [S._fields(40 + 10 * k + j, 1) for j in range(2)]
  logs = {}
  for name, spec in (("new", new), ("old", old)):
    logs[name] = []
    S._rollout(logs[name], derived={"d": spec}, climatology=climatology, windows={"w": WindowSpec("max", 2, stride=1, source="d")})
  assert [c[:2] for c in logs["new"]] == [c[:2] for c in logs["old"]]              # the same calls on the same handles
  sets = [c for c in logs["new"] if c[1] == "derive_set"]
  assert {c[0] for c in sets} == {"view2", "climview2"} and len(sets) == 2
  want = new.plan(S._fields(20, 1), [2.0, 0.5, 4.0, 1.0], [1.0, -1.0, 2.0, 0.0])      # the scales and locations of S._stats()
  for c in sets:
    got = dict(c[2:])
    assert sorted(got) == EXPR_KEYS
    for k, v in want.items():
      np.testing.assert_array_equal(got[k], v, err_msg=k)
  assert list(want["op"]) == [2, 4] and want["term_start"].tolist() == [[0, 2, 2], [0, 0, 0]] and want["pole_row"].tolist() == [0, 0]
  for c in (c for c in logs["old"] if c[1] == "derive_set"):
    assert sorted(dict(c[2:])) == LEGACY_KEYS
