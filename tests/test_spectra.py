"""Spherical-harmonic power spectra without a GPU: the analysis tables, the float64 yardstick against closed forms
(tests/spectrum_reference.py), EnsembleSpectra arithmetic, the C ABI and the host plumbing on a recording handle."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from gencast_flax_nnx_amd import (EnsembleSampler, EnsembleSpectra, GenCast, NaNCleaner, Sampler, SphericalAnalysis, _lib, config,
                                  datasets, noise, rollout, spectra, synthetic)
from tests import spectrum_reference as R
from tests.test_verification import _RecordingNative, _host_sampler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(n_lat, n_lon):
  return np.linspace(-90.0, 90.0, n_lat), np.arange(n_lon) * (360.0 / n_lon)


# ---- tables ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lat,n_lon", [(13, 24), (19, 36), (73, 144)])
def test_analysis_tables_invert_the_synthesis_tables(n_lat, n_lon):
  lat, lon = _grid(n_lat, n_lon)
  sa = SphericalAnalysis(lat, lon)
  L = sa.lmax
  assert L == n_lon // 2 and sa.legendre_analysis.shape == (L, L, n_lat) and sa.cos_a.shape == sa.sin_a.shape == (L, n_lon)
  # Fourier rows against the synthesis tables of the noise generator (float32 there: 2^-24 per entry, n_lon entries)
  gen = noise.SphericalNoise(lat, lon)
  eye = np.eye(L)
  tol = 4 * 2.0 ** -24
  np.testing.assert_allclose(sa.cos_a @ gen._cos.astype(np.float64), eye, atol=tol)
  sin_eye = eye.copy()
  sin_eye[0, 0] = 0.0                                                      # no sine term at m = 0
  np.testing.assert_allclose(sa.sin_a @ gen._sin.astype(np.float64), sin_eye, atol=tol)
  np.testing.assert_allclose(sa.cos_a @ gen._sin.astype(np.float64), 0.0, atol=tol)
  np.testing.assert_allclose(sa.sin_a @ gen._cos.astype(np.float64), 0.0, atol=tol)
  # Q_m A_m = I in float64
  P = noise._normalized_legendre(np.sin(np.deg2rad(lat)), L)
  for m in range(L):
    np.testing.assert_allclose(sa.legendre_analysis[m, m:, :] @ P[m, m:, :].T, np.eye(L - m), atol=1e-12)
    assert not sa.legendre_analysis[m, :m].any()
  # the yardstick's own tables (scipy lpmv) are the same numbers
  Q, ca, sn = R.tables(lat, lon, L)
  np.testing.assert_allclose(sa.legendre_analysis, Q, atol=1e-9)
  np.testing.assert_allclose(sa.cos_a, ca, atol=1e-15)
  np.testing.assert_allclose(sa.sin_a, sn, atol=1e-15)
  q, c, s = sa.device_tables()
  assert q.dtype == c.dtype == s.dtype == np.float32 and q.flags.c_contiguous and q.shape == (L, L, n_lat)


@pytest.mark.parametrize("n_lat,n_lon,want", [(19, 36, 5.5), (73, 144, 10.9), (181, 360, 17.2)])
def test_condition_numbers_of_the_least_squares_fit(n_lat, n_lon, want):
  sa = SphericalAnalysis(*_grid(n_lat, n_lon))
  assert int(np.argmax(sa.condition_numbers)) == 0
  assert abs(sa.worst_condition - want) < 0.06, sa.worst_condition
  assert 0.05 < np.abs(sa.legendre_analysis).max() < 0.7                   # float32 tables are harmless


def test_builder_refuses_what_it_cannot_invert():
  lat, lon = _grid(13, 36)
  with pytest.raises(ValueError, match="condition"):
    SphericalAnalysis(lat, lon)                                            # n_lat = 13 < lmax = 18
  assert SphericalAnalysis(lat, lon, lmax=12).lmax == 12                   # the caller's band limit
  with pytest.raises(ValueError, match="lmax"):
    SphericalAnalysis(lat, lon, lmax=19)
  with pytest.raises(ValueError, match="lmax"):
    SphericalAnalysis(lat, lon, lmax=0)
  with pytest.raises(ValueError, match="sorted"):
    SphericalAnalysis(lat[::-1], lon)
  with pytest.raises(ValueError, match="longitudes"):
    SphericalAnalysis(lat, lon + 5.0)


# ---- the yardstick against closed forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lat,n_lon", [(13, 24), (73, 144)])
def test_reference_recovers_the_closed_form_power_of_a_synthesised_field(n_lat, n_lon):
  """Synthesis with the generator's float32 tables, analysis with the yardstick's own float64 tables.  What is left is
  the float32 rounding of the three synthesis tables (2^-24 each) amplified by the condition number of the fit (< 11)
  and doubled by the square: 2 * 11 * 3 * 2^-24 = 4e-6 of a wavenumber's power."""
  lat, lon = _grid(n_lat, n_lon)
  gen = noise.SphericalNoise(lat, lon)
  L, N = gen.lmax, 3
  rng = np.random.default_rng(n_lat)
  z = rng.standard_normal((2, L, L, N))
  z[1, 0] = 0.0
  field = gen.synthesize(z[0], z[1])                                        # [lat, lon, N] float64
  tabs = R.tables(lat, lon, L)
  a, _ = R.analyse(field, *tabs)
  got, want = R.power(a), R.noise_coefficient_power(z)
  rel = np.abs(got - want) / want
  print(f"{n_lat}x{n_lon}: closed form recovered to {rel.max():.2e} relative")
  assert rel.max() < 4e-6
  # the coefficients themselves, and the energy: sum_l power = sum a^2 / (4 pi)
  want_a = R.noise_coefficients(z)
  assert np.abs(a - want_a).max() < 4e-6 * np.abs(want_a).max()
  np.testing.assert_allclose(got.sum(axis=1), (want_a ** 2).sum(axis=(0, 1, 2)) / R.FOUR_PI, rtol=4e-6)
  # the float32 device tables change nothing beyond their own rounding
  a32, A = R.analyse(field.astype(np.float32), *SphericalAnalysis(lat, lon).device_tables())
  assert (np.abs(R.power(a32) - want) / want).max() < 8e-6
  assert np.all(np.abs(a32) <= A * (1 + 1e-12))


def test_reference_ensemble_identities_and_non_finite_columns():
  n_lat, n_lon, M, N = 13, 24, 5, 4
  lat, lon = _grid(n_lat, n_lon)
  tabs = SphericalAnalysis(lat, lon).device_tables()
  rng = np.random.default_rng(3)
  members = rng.standard_normal((M, n_lat * n_lon, 1, N)).astype(np.float32)
  truth = rng.standard_normal((n_lat * n_lon, 1, N)).astype(np.float32)
  ref = R.ensemble(members, truth, n_lat, n_lon, tabs)
  s = ref["sums"]
  cross = sum(R.power(0.5 * (x + ref["y"])) - R.power(0.5 * (x - ref["y"])) for x in ref["xs"])   # polarisation: <x, y>
  scale = s[..., 1] + M * s[..., 0]
  assert np.abs(s[..., 3] - (s[..., 1] + M * s[..., 0] - 2 * cross)).max() <= 64 * R.U * scale.max()
  assert np.abs(s[..., 5] - (s[..., 1] - M * s[..., 2])).max() <= 64 * R.U * scale.max()
  np.testing.assert_array_equal(ref["member_power"].sum(axis=0) if M == 1 else sum(ref["member_power"]), s[..., 1])
  assert (ref["tol"] > 0).all() and (ref["tol"] < 1e-9 * (1 + s)).all()
  # a column subset is the same numbers
  sub = R.ensemble(members, truth, n_lat, n_lon, tabs, cols=[3, 1])
  np.testing.assert_array_equal(sub["sums"], s[[3, 1]])
  # a NaN / an Inf anywhere poisons its column, and only it
  members[2, 17, 0, 1] = np.nan
  truth[5, 0, 3] = np.inf
  bad = R.ensemble(members, truth, n_lat, n_lon, tabs)
  assert bad["bad"].tolist() == [False, True, False, True]
  assert np.isnan(bad["sums"][[1, 3]]).all() and np.isnan(bad["member_power"][:, [1, 3]]).all()
  np.testing.assert_array_equal(bad["sums"][[0, 2]], s[[0, 2]])


# ---- EnsembleSpectra ------------------------------------------------------------------------------------------------------
def test_ensemble_spectra_arithmetic():
  rng = np.random.default_rng(0)
  B, C, L, M = 2, 82, 12, 4
  sums = rng.uniform(0.5, 2.0, (B, C, L, 6))
  sp = EnsembleSpectra(sums, M)
  np.testing.assert_array_equal(sp.truth_power, sums[..., 0])
  np.testing.assert_array_equal(sp.member_power, sums[..., 1] / M)
  np.testing.assert_array_equal(sp.mean_power, sums[..., 2])
  np.testing.assert_array_equal(sp.power_ratio, sums[..., 1] / M / sums[..., 0])
  np.testing.assert_array_equal(sp.error_power, sums[..., 3] / M)
  np.testing.assert_array_equal(sp.mean_error_power, sums[..., 4])
  np.testing.assert_array_equal(sp.spread_power, sums[..., 5] / (M - 1))
  np.testing.assert_allclose(sp.spectral_spread_skill, np.sqrt((M + 1) / M * sums[..., 5] / (M - 1) / sums[..., 4]), rtol=1e-15)
  assert sp.lmax == L and sp.n_dates == 1
  # dates merge by addition, the derived spectra become means over dates
  other = EnsembleSpectra(rng.uniform(0.5, 2.0, (B, C, L, 6)), M)
  both = EnsembleSpectra.merge([sp, other])
  assert both.n_dates == 2
  np.testing.assert_array_equal(both.sums, sums + other.sums)
  np.testing.assert_allclose(both.truth_power, 0.5 * (sp.truth_power + other.truth_power), rtol=1e-15)
  np.testing.assert_allclose(both.spread_power, 0.5 * (sp.spread_power + other.spread_power), rtol=1e-15)
  with pytest.raises(ValueError):
    EnsembleSpectra.merge([sp, EnsembleSpectra(sums, M + 1)])
  with pytest.raises(ValueError):
    EnsembleSpectra.merge([])
  # a x: every power times a^2; ratios do not move
  a = rng.uniform(-3, 3, C)
  sc = sp.scaled(a)
  np.testing.assert_array_equal(sc.sums, sums * (a * a)[None, :, None, None])
  np.testing.assert_allclose(sc.power_ratio, sp.power_ratio, rtol=1e-14)
  np.testing.assert_allclose(sc.spectral_spread_skill, sp.spectral_spread_skill, rtol=1e-14)
  assert "ffset" in EnsembleSpectra.scaled.__doc__                       # offsets are documented as unsupported
  for bad in (np.ones(C - 1), np.zeros(C), np.full(C, np.nan)):
    with pytest.raises(ValueError):
      sp.scaled(bad)
  with pytest.raises(ValueError):
    EnsembleSpectra(sums[..., :5], M)
  with pytest.raises(ValueError):
    EnsembleSpectra(sums, 1)
  # per variable
  lat, lon = _grid(13, 24)
  _, tgt, _ = synthetic.make_example(lat=lat, lon=lon, batch=B, seed=1)
  pv = sp.per_variable(tgt)
  assert set(pv) == set(EnsembleSpectra.NAMES)
  off = {name: (o, n) for name, o, n in datasets.channel_layout(tgt)}
  o, n = off["temperature"]
  assert n == 13 and pv["power_ratio"]["temperature"].shape == (B, 13, L)
  np.testing.assert_array_equal(pv["spread_power"]["temperature"], sp.spread_power[:, o:o + n])
  with pytest.raises(ValueError):
    EnsembleSpectra(sums[:, :5], M).per_variable(tgt)


# ---- the C ABI --------------------------------------------------------------------------------------------------------
_dp = ctypes.POINTER(ctypes.c_double)
_fp = ctypes.POINTER(ctypes.c_float)
ENTRIES = {
    "gc_spec_set_tables": [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _fp, _fp, _fp],
    "gc_spec_field": [ctypes.c_void_p, _fp, _dp],
    "gc_ens_spectrum": [ctypes.c_void_p, _fp, _dp, _dp],
}


def test_new_entries_are_declared_bound_and_exported():
  header = open(os.path.join(ROOT, "include", "gencast_hip.h")).read()
  lib = _lib.load_library()
  for name, args in ENTRIES.items():
    assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    res, bound = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and bound == args, name
    assert getattr(lib, name) is not None
  assert lib.gc_num_kernel_classes() == 13                                # the new kernels are filed under gc_pack
  for counter in ("spec_calls", "spec_device_us", "spec_invalid_columns"):
    assert counter in header
  for method in ("spec_set_tables", "spec_field", "ens_spectrum"):
    assert callable(getattr(_lib.NativeDenoiser, method))
  assert list(inspect.signature(_lib.NativeDenoiser.spec_field).parameters) == ["self", "field"]
  assert list(inspect.signature(_lib.NativeDenoiser.ens_spectrum).parameters) == ["self", "truth", "want_member_power"]
  assert callable(Sampler.sample_spectrum) and callable(EnsembleSampler.spectra) and callable(EnsembleSampler.scores_and_spectra)
  assert callable(GenCast.ensemble_spectra) and callable(rollout.InputsAndResiduals.ensemble_spectra)
  assert callable(NaNCleaner.ensemble_spectra)
  # compiled and linked by both build scripts: both read the one list (test_abi.py holds them to it)
  assert open(os.path.join(ROOT, "gencast-flax-nnx_amd/csrc/SOURCES")).read().split().count("gc_spectrum.hip") == 1
  for script in ("gencast-flax-nnx_amd/csrc/build.sh", "tools/build_variant.sh"):
    assert "< <(grep -v '^#' SOURCES)" in open(os.path.join(ROOT, script)).read(), script
  src = open(os.path.join(ROOT, "gencast-flax-nnx_amd", "spectra.py")).read()
  assert "spectrum_reference" not in src.replace("tests/spectrum_reference.py", "") and "fft" not in src and "matmul" not in src


# ---- the host path, on a recording stand-in for the handle ------------------------------------------------------------------
class _SpecNative(_RecordingNative):
  def spec_set_tables(self, q, c, s):
    self.log.append(("tables", q.shape, c.shape, s.shape, q.dtype))
    self.lmax = q.shape[0]

  def ens_spectrum(self, truth=None, want_member_power=False):
    self.log.append(("spectrum", truth is None))
    self.spec_truth = truth
    return np.full(self.shape[1:] + (self.lmax, 6), 2.0)

  def ens_score(self, truth=None, want_fields=False):
    self.log.append(("score",))
    return super().ens_score(truth, want_fields)

  def spec_field(self, field=None):
    self.log.append(("spec_field", field is None))
    return np.ones(self.shape[1:] + (self.lmax,))


def _spec_sampler(log):
  gc = _host_sampler(log)
  gc.denoiser.native = _SpecNative(log, "lane0")
  return gc


def test_sampler_spectra_push_every_member_and_download_none():
  lat, lon = _grid(9, 16)
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  log = []
  gc = _spec_sampler(log)
  ens = EnsembleSampler(gc._sampler, base_seed=1, concurrent_members=2)
  sp = ens.spectra(inp, tgt, frc, 4)
  assert isinstance(sp, EnsembleSpectra) and sp.n_members == 4 and sp.sums.shape == (1, 82, 8, 6)
  assert log[0] == ("reserve", 4) and log[1] == ("tables", (8, 8, 9), (8, 16), (8, 16), np.float32)
  assert [e for e in log if e[0] == "push"] == [("push", 0, "lane0"), ("push", 1, "lane1"), ("push", 2, "lane0"), ("push", 3, "lane1")]
  assert ("score",) not in log and log[-1] == ("spectrum", False)
  native = gc.denoiser.native
  want_truth = np.transpose(datasets.dataset_to_stacked(tgt, tgt.sizes), (1, 2, 0, 3)).reshape(9 * 16, 1, 82)
  np.testing.assert_array_equal(native.spec_truth, want_truth)
  # the tables go over once per (grid, lmax); another band limit replaces them
  del log[:]
  ens.spectra(inp, tgt, frc, 4)
  assert not [e for e in log if e[0] == "tables"]
  assert ens.spectra(inp, tgt, frc, 4, lmax=5).lmax == 5
  assert [e for e in log if e[0] == "tables"] == [("tables", (5, 5, 9), (5, 16), (5, 16), np.float32)]
  # scores and spectra from the same members, sampled once: one truth upload, the spectrum call reuses it
  del log[:]
  out = ens.scores_and_spectra(inp, tgt, frc, 4)
  assert len(out) == 2 and out[0].n_members == 4 and isinstance(out[1], EnsembleSpectra)
  assert [e[0] for e in log if e[0] in ("sample", "score", "spectrum")] == ["sample"] * 4 + ["score", "spectrum"]
  assert log[-1] == ("spectrum", True)
  scores, mean, var, sp2 = ens.scores_and_spectra(inp, tgt, frc, 4, fields=True)
  assert isinstance(mean, datasets.Dataset) and isinstance(sp2, EnsembleSpectra)
  # scores() itself is what it was
  assert ens.scores(inp, tgt, frc, 4).n_members == 4 and log[-1] == ("score",)
  # through GenCast and the wrappers: physical units are a^2
  def stats(v):
    names = set(config.TASK.input_variables) | set(config.TASK.target_variables)
    return datasets.Dataset({n: (datasets.Variable(("level",), np.full(13, v, np.float32)) if n in config.ALL_ATMOSPHERIC_VARS
                                 else datasets.Variable((), np.float32(v))) for n in names})
  norm = rollout.InputsAndResiduals(gc, stats(2.0), stats(0.5), stats(0.25))
  stack = NaNCleaner(norm, "2m_temperature", datasets.Dataset({"2m_temperature": datasets.Variable((), np.float32(0))}))
  plain = gc.ensemble_spectra(inp, tgt, frc, num_members=4, lmax=5)
  phys = stack.ensemble_spectra(inp, tgt, frc, num_members=4, lmax=5)
  np.testing.assert_array_equal(phys.sums, plain.sums * 0.0625)
  both = stack.ensemble_spectra(inp, tgt, frc, num_members=4, lmax=5, scores=True)
  np.testing.assert_array_equal(both[1].sums, plain.sums * 0.0625)
  np.testing.assert_array_equal(both[0].sums, gc.ensemble_scores(inp, tgt, frc, num_members=4).sums *
                                np.array([1.0, 0.25, 0.0625, 0.0625, 0.25, 0.25]))
  assert "offset" in rollout.InputsAndResiduals.ensemble_spectra.__doc__
  # the spectrum of the last resident sample
  with pytest.raises(ValueError, match="no sample"):
    gc._sampler.sample_spectrum()
  native.download_sample = lambda: np.zeros((9 * 16, 1, 82), np.float32)
  native.set_churn = lambda *a: None
  native.sample_resident = lambda *a, **k: None
  gc._sampler(inp, tgt, frc, rngs=3)
  del log[:]
  p = gc._sampler.sample_spectrum()
  assert p.shape == (1, 82, 8) and log[-1] == ("spec_field", True)


def test_argument_errors_that_need_no_gpu():
  log = []
  gc = _spec_sampler(log)
  for call in ("spectra", "scores_and_spectra"):
    with pytest.raises(ValueError, match="ens_push_host"):
      getattr(EnsembleSampler(gc._sampler, rank=0, world_size=2), call)(None, None, None, 4)
  assert log == []
  with pytest.raises(ValueError, match="lat"):
    spectra.ensure_tables(gc.denoiser.native, datasets.Dataset({"a": datasets.Variable(("batch",), np.zeros(1))}))
