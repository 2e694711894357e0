"""Spectral band views, host side: the float64 definition of tests/band_reference.py against the
identities a filter on the sphere has to satisfy, `verification.BandSpec` (validation, naming, channel order, taper,
wavelengths, statistics, plan) on config.TASK, the synthesis tables of `spectra.SphericalAnalysis`, and the band plan of
`verification.ScoredStore`.  The device side is tests/test_gpu_band.py and tests/test_gpu_band_rollout.py.

The identities are asserted to a bound that is composed, not measured.  A field of the model f = Y c (Y: the synthesis of
`band_reference.synthesise`, c its coefficients) does not come back as Y (w c) exactly, for three reasons, each bounded here:
  * the arithmetic of the view itself: the `tol` that `band_reference.view` returns;
  * f is Y c only up to the rounding e of its own synthesis, |e| <= 2 dg (`synthesise`'s own bound); an input error of
    at most max |e| moves a coefficient by at most max |e| S_lm (`spectrum_reference.pointwise_gain`);
  * the tables are inverse to each other only up to their own rounding (Q_m = pinv(A_m) comes out of an SVD): analysing the
    columns of Y gives I + Delta, Delta known to `coef_tolerance`, so the coefficients of f are c + Delta c.
The last two are errors of the coefficients, |dc| <= (|Delta| + dDelta) |c| + max |e| S; weighted with |w| they go through the
synthesis with the absolute tables, which `synthesise` does with its `db` argument."""
import inspect

import numpy as np
import pytest

from gencast_flax_nnx_amd import BandSpec, SphericalAnalysis, _lib, datasets, synthetic, verification
from tests import band_reference as B
from tests import spectrum_reference as R

N_LAT, N_LON, L = 21, 40, 20
LAT, LON = np.linspace(-90, 90, N_LAT), np.arange(N_LON) * (360.0 / N_LON)
LAT13, LON24 = np.linspace(-90, 90, 13), np.arange(24) * 15.0


class _Grid:
  """The float64 lpmv tables of the 21 x 40 grid and what the bound needs of them, made once."""
  _made = None

  @classmethod
  def get(cls):
    if cls._made is None:
      g = cls._made = cls()
      g.atabs, g.stabs = R.tables(LAT, LON, L), B.synthesis_tables(LAT, LON, L)
      n = 2 * L * L
      eye = np.eye(n).reshape(2, L, L, n)
      valid = (np.arange(L)[:, None] <= np.arange(L)[None, :])[None, :, :, None]       # l >= m
      eye = np.where(valid, eye, 0.0)
      eye[1, 0] = 0.0                                                                   # no sine part at m = 0
      Y, dY = B.synthesise(eye, np.zeros_like(eye), np.abs(eye), *g.stabs)
      a, A = R.analyse(Y, *g.atabs)
      # Delta[coefficient out, coefficient in]; the rounding of Y itself enters through the gain
      g.gain = R.pointwise_gain(*g.atabs)                                              # [2, L, L]
      g.delta = (np.abs(a - eye) + R.coef_tolerance(A, N_LAT, N_LON) + g.gain[..., None] * 2.0 * dY.max(axis=(0, 1))[None, None, None, :])
      g.delta = np.where(valid, g.delta, 0.0).reshape(n, n)
    return cls._made


def _field(c):
  """c [2, L, L, N] -> (f = Y c, max |e| per column: the rounding of that synthesis)."""
  g = _Grid.get()
  f, dg = B.synthesise(c, np.zeros_like(c), np.abs(c), *g.stabs)
  return f, 2.0 * dg.max(axis=(0, 1))


def _model_bound(c, w, e_max):
  """|view_w(Y c + e) - Y (w c)| beyond the view's own tolerance: the coefficient errors through the absolute synthesis."""
  g = _Grid.get()
  N = c.shape[3]
  dc = (g.delta @ np.abs(c).reshape(-1, N)).reshape(2, L, L, N) + g.gain[..., None] * e_max[None, None, None, :]
  zero = np.zeros_like(c)
  carried = B.synthesise(zero, np.abs(np.asarray(w, np.float64))[None, None, :, None] * dc, zero, *g.stabs)[1]
  return 2.0 * carried


def _coefficients(N, seed):
  c = np.random.default_rng(seed).standard_normal((2, L, L, N)) * np.logspace(-2, 3, N)
  c = np.where((np.arange(L)[:, None] <= np.arange(L)[None, :])[None, :, :, None], c, 0.0)
  c[1, 0] = 0.0
  return c


def _sharp(lo, hi):
  return ((np.arange(L) >= lo) & (np.arange(L) <= hi)).astype(np.float64)


# ---- the definition ---------------------------------------------------------------------------------------------------------
def test_a_band_limited_field_comes_back_under_the_all_ones_response():
  g = _Grid.get()
  c = _coefficients(6, 1)
  f, e = _field(c)
  d, tol = B.view(f, np.ones(L), False, g.atabs, g.stabs)
  bound = tol + _model_bound(c, np.ones(L), e) + e[None, None, :]
  print(f"round trip: worst |view - f| / bound {np.max(np.abs(d - f) / bound):.3g}, bound / max |f| {np.max(bound / np.abs(f).max(axis=(0, 1))):.3g}")
  assert np.all(np.abs(d - f) <= bound)
  assert np.all(bound <= 1e-9 * np.abs(f).max(axis=(0, 1)))          # (the bound means something: far below any band's content)


def test_bands_that_partition_the_wavenumbers_sum_to_the_all_ones_view():
  g = _Grid.get()
  rng = np.random.default_rng(2)
  f = (rng.standard_normal((N_LAT, N_LON, 5)) * np.logspace(-3, 4, 5)).astype(np.float32)   # NOT band-limited: grid-point noise
  whole, tol = B.view(f, np.ones(L), False, g.atabs, g.stabs)
  parts = [B.view(f, w, False, g.atabs, g.stabs) for w in (_sharp(0, 3), _sharp(4, 11), _sharp(12, L - 1))]
  total, bound = np.zeros_like(whole), tol.copy()
  for d, t in parts:
    total = total + d
    bound += t + R.U * np.abs(total)
  assert np.all(np.abs(total - whole) <= bound)
  # the tapered bands of a BandSpec partition too: two bands that meet at an edge sum to one there
  w, _ = BandSpec({"a": (0, 3), "b": (4, 11), "c": (12, None)}, taper=1.5).responses(L)
  np.testing.assert_allclose(w.sum(axis=0), 1.0, rtol=0, atol=4 * R.U)
  assert 0 < w[0, 4] < w[0, 3] < 1
  # and the grid-point noise has a large part outside the span of the basis, which only `complement` keeps
  resid = np.sqrt(np.mean((f - whole) ** 2, axis=(0, 1)) / np.mean(f.astype(np.float64) ** 2, axis=(0, 1)))
  assert np.all((resid > 0.5) & (resid < 0.9)), resid


def test_low_plus_its_complement_is_the_field():
  g = _Grid.get()
  rng = np.random.default_rng(3)
  f = (rng.standard_normal((N_LAT, N_LON, 4)) * np.logspace(-1, 5, 4) + np.logspace(0, 6, 4)).astype(np.float32)
  w = BandSpec({"lo": (0, 5)}, taper=1).responses(L)[0][0]
  low, t0 = B.view(f, w, False, g.atabs, g.stabs)
  high, t1 = B.view(f, w, True, g.atabs, g.stabs)
  total = low + high
  assert np.all(np.abs(total - f) <= t0 + t1 + R.U * np.abs(total))


def test_a_single_harmonic_lands_only_in_the_band_that_holds_it():
  g = _Grid.get()
  cases = [(0, 0, 0), (0, 3, 7), (1, 3, 7), (0, 19, 19), (1, 5, 12), (0, 0, 13)]       # (part, m, l)
  c = np.zeros((2, L, L, len(cases)))
  for n, (part, m, l) in enumerate(cases):
    c[part, m, l, n] = 2.5 * (n + 1)
  f, e = _field(c)
  bands = [_sharp(0, 6), _sharp(7, 12), _sharp(13, L - 1)]
  for w in bands:
    d, tol = B.view(f, w, False, g.atabs, g.stabs)
    want = f * np.array([w[l] for _, _, l in cases])[None, None, :]
    bound = tol + _model_bound(c, w, e) + e[None, None, :]
    assert np.all(np.abs(d - want) <= bound)
    assert np.all(bound <= 1e-9 * np.abs(f).max(axis=(0, 1)))


def test_a_constant_comes_back_times_the_weight_of_wavenumber_zero():
  g = _Grid.get()
  consts = np.array([3.25, -1.0e5, 2.0e-3])
  f = np.broadcast_to(consts, (N_LAT, N_LON, 3)).copy()
  c = np.zeros((2, L, L, 3))
  c[0, 0, 0] = consts * np.sqrt(4.0 * np.pi)                   # Y_00 = 1 / sqrt(4 pi)
  e = 4.0 * R.U * np.abs(consts)                               # c_00 Y_00 is the constant up to two roundings
  for w0, comp in ((1.0, False), (0.25, False), (0.25, True), (0.0, True)):
    w = _sharp(0, 4) * w0
    w[1:5] = 1.0
    d, tol = B.view(f, w, comp, g.atabs, g.stabs)
    want = consts * ((1.0 - w0) if comp else w0)
    bound = tol + _model_bound(c, w, e) + e[None, None, :] + R.U * np.abs(consts)
    assert np.all(np.abs(d - want[None, None, :]) <= bound), (w0, comp)


def test_band_fields_marks_the_columns_that_read_a_value_that_is_not_finite():
  sa = SphericalAnalysis(LAT13, LON24, 12)
  atabs, stabs = sa.device_tables(), sa.synthesis_tables()
  rng = np.random.default_rng(4)
  x = rng.standard_normal((13 * 24, 2, 3)).astype(np.float32)
  resp, comp = BandSpec({"lo": (0, 3), "hi": dict(l=(0, 3), complement=True)}).responses(12)
  src, band = np.array([0, 0, 2, 2]), np.array([0, 1, 0, 1])
  clean = B.band_fields(x, 13, 24, resp, comp, src, band, atabs, stabs)
  x[17, 1, 2] = np.inf
  d, tol, bad = B.band_fields(x, 13, 24, resp, comp, src, band, atabs, stabs)
  assert bad.tolist() == [[False, False, False], [False, False, True]]
  assert np.isnan(d[:, 1, 2:]).all() and not np.isnan(d[:, 0]).any() and not np.isnan(d[:, 1, :2]).any()
  keep = ~np.isnan(d)
  np.testing.assert_array_equal(d[keep], clean[0][keep])
  np.testing.assert_array_equal(tol[keep], clean[1][keep])


# ---- BandSpec ---------------------------------------------------------------------------------------------------------------
def _targets(lat=LAT13, lon=LON24, batch=2):
  return synthetic.make_example(lat=lat, lon=lon, batch=batch, seed=0)[1]


@pytest.mark.parametrize("kw,match", [
    (dict(bands={}), "1 .. 8"), (dict(bands={str(k): (0, 1) for k in range(9)}), "1 .. 8"), (dict(bands=[("a", (0, 1))]), "mapping"),
    (dict(bands={"a": (3, 2)}), "l_lo <= l_hi"), (dict(bands={"a": (-1, 2)}), "l_lo <= l_hi"), (dict(bands={"a": (0.5, 2)}), "integers"),
    (dict(bands={"a": (None, 2)}), "l_lo <= l_hi"), (dict(bands={"a": (0, 12)}, lmax=12), "beyond lmax"),
    (dict(bands={"a": dict(l=(0, 1), response=[1.0])}), "either"), (dict(bands={"a": dict(l=(0, 1), what=1)}), "either"),
    (dict(bands={"a": np.array([1.0, np.nan])}), "finite"), (dict(bands={"a": np.ones(5)}, lmax=12), "lmax is 12"),
    (dict(bands={"": (0, 1)}), "non-empty"), (dict(bands={"a": (0, 1)}, taper=-1), "taper"), (dict(bands={"a": (0, 1)}, lmax=0), "lmax"),
    (dict(bands={"a": (0, 1)}, variables=[]), "variables"), (dict(bands={"a": (0, 1)}, variables=["x", "x"]), "variables")])
def test_band_spec_rejects(kw, match):
  with pytest.raises(ValueError, match=match):
    BandSpec(**kw)


def test_band_spec_names_channels_and_statistics():
  t = _targets()
  spec = BandSpec({"lo": (0, 3), "mid": (4, 8), "hi": dict(l=(0, 3), complement=True)}, variables=["geopotential", "2m_temperature"], taper=1)
  assert spec.names == ["geopotential_lo", "geopotential_mid", "geopotential_hi", "2m_temperature_lo", "2m_temperature_mid", "2m_temperature_hi"]
  assert spec.band_names == ["lo", "mid", "hi"] and BandSpec({"lo": (0, 3)}).names == ["lo"]
  tt = spec.template(t)
  where0 = {n: (o, k) for n, o, k in datasets.channel_layout(t)}
  layout = datasets.channel_layout(tt)
  assert [n for n, _, _ in layout] == sorted(spec.names)                # packed in sorted-name order, like every Dataset
  for name, _, n in layout:
    var = name.rsplit("_", 1)[0]
    assert tt[name].dims == t[var].dims and n == where0[var][1]         # the level dim travels with the variable
  plan = spec.plan(t)
  assert list(plan) == list(inspect.signature(_lib.NativeDenoiser.ens_band_set).parameters)[1:]
  c_d = sum(n for _, _, n in layout)
  assert plan["c_src"] == 82 and plan["response"].shape == (3, 12) and plan["src_channel"].shape == plan["band"].shape == (c_d,)
  assert plan["complement"].tolist() == [0, 0, 1] and plan["response"].dtype == np.float64
  for name, off, n in layout:
    var, band = name.rsplit("_", 1)
    assert plan["src_channel"][off:off + n].tolist() == list(range(where0[var][0], where0[var][0] + n))
    assert set(plan["band"][off:off + n].tolist()) == {["lo", "mid", "hi"].index(band)}
  w = plan["response"]
  np.testing.assert_array_equal(w[0], w[2])
  assert w[0, :3].tolist() == [1, 1, 1] and 0.5 < w[0, 3] < 1 and 0 < w[0, 4] < 0.5 and not w[0, 5:].any()
  np.testing.assert_allclose(w[0] + w[1], np.r_[np.ones(8), w[1, 8:]], rtol=0, atol=2 * R.U)   # the shared edge sums to one
  assert w[1, 9] > 0 and not w[1, 10:].any()
  np.testing.assert_array_equal(BandSpec({"a": (4, 8)}).responses(12)[0][0], (np.arange(12) >= 4) & (np.arange(12) <= 8))
  # statistics: the source's scale; the location times w[0], or 1 - w[0] with complement
  scale, loc = np.arange(1.0, 83.0), np.arange(82.0) * 10.0 + 5.0
  ds, dl = spec.channel_stats(t, scale, loc)
  np.testing.assert_array_equal(ds, scale[plan["src_channel"]])
  w0 = np.where(plan["band"] == 2, 1.0 - w[plan["band"], 0], w[plan["band"], 0])
  np.testing.assert_array_equal(dl, loc[plan["src_channel"]] * w0)
  assert set(w0.tolist()) == {0.0, 1.0} and dl[plan["band"] == 1].tolist() == [0.0] * 14 and (dl[plan["band"] == 0] > 0).all()
  part = BandSpec({"p": np.r_[0.25, np.ones(11)], "q": dict(response=np.r_[0.25, np.ones(11)], complement=True)}, variables=["2m_temperature"])
  np.testing.assert_array_equal(part.channel_stats(t, scale, loc)[1], loc[2] * np.array([0.25, 0.75]))
  # all variables by default, lmax from the grid or as given
  assert len(BandSpec({"lo": (0, 3)}).plan(t)["band"]) == 82
  assert BandSpec({"lo": (0, 3)}, lmax=8).plan(t)["response"].shape == (1, 8)
  for bad, match in ((BandSpec({"lo": (0, 3)}, variables=["nope"]), "not a target variable"), (BandSpec({"lo": (0, 3)}, lmax=13), "lmax must be"),
                     (BandSpec({"lo": (0, 12)}), "beyond lmax"), (BandSpec({"lo": np.ones(7)}), "7 weights")):
    with pytest.raises(ValueError, match=match):
      bad.plan(t)
  with pytest.raises(ValueError, match="shape"):
    spec.channel_stats(t, scale[:5], loc)


def test_band_spec_from_wavelengths():
  spec = BandSpec.from_wavelengths_km({"planetary": (None, 10000.0), "synoptic": (10000.0, 2000.0),
                                       "small": dict(km=(None, 2000.0), complement=True)}, lmax=40)
  circ = 2.0 * np.pi * 6371.0
  assert round(circ / 10000.0) == 4 and round(circ / 2000.0) == 20
  assert spec.bands == {"planetary": ("l", 0, 4, False), "synoptic": ("l", 4, 20, False), "small": ("l", 0, 20, True)}
  assert BandSpec.from_wavelengths_km({"a": (5000.0, None)}).bands == {"a": ("l", 8, None, False)}
  with pytest.raises(ValueError, match="wavelength"):
    BandSpec.from_wavelengths_km({"a": (0.0, 100.0)})


def test_the_products_synthesis_tables_agree_with_lpmv():
  sa = SphericalAnalysis(LAT, LON, L)
  leg, cos_s, sin_s = sa.synthesis_tables()
  S, c, s = B.synthesis_tables(LAT, LON, L)
  assert leg.dtype == cos_s.dtype == sin_s.dtype == np.float32 and leg.shape == (L, N_LAT, L) and cos_s.shape == sin_s.shape == (L, N_LON)
  # float32 rounding of values of magnitude <= max |table|, plus the last bits of two float64 recurrences
  for got, want in ((leg, S), (cos_s, c), (sin_s, s)):
    assert np.all(np.abs(got - want) <= 2.0 ** -24 * np.abs(want) + 1e-12 * np.abs(want).max())
  assert not np.transpose(leg, (0, 2, 1))[np.arange(L)[:, None] > np.arange(L)[None, :]].any()   # zero for l < m
  q = sa.device_tables()[0]
  for m in (0, 5, 19):                                                        # the synthesis is the matrix the analysis inverts
    np.testing.assert_allclose(q[m, m:, :].astype(np.float64) @ leg[m, :, m:].astype(np.float64), np.eye(L - m), rtol=0, atol=1e-5)


def test_scored_store_takes_one_plan():
  S = verification.ScoredStore
  h, src = object(), object()
  for two in (dict(plan={}, band_plan={}), dict(feature_plan={}, band_plan={})):
    with pytest.raises(ValueError, match="not two"):
      S(h, 4, None, source=src, **two)
  with pytest.raises(ValueError, match="go together"):
    S(h, 4, None, band_plan={})
  with pytest.raises(ValueError, match="go together"):
    S(h, 4, None, source=src)
  store = S(h, 4, None, band_plan={"c_src": 3}, source=src)
  assert store.band_plan == {"c_src": 3} and store.plan is None and store.feature_plan is None
