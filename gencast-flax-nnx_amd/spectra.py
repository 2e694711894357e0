"""Spherical-harmonic power spectra: whether a sample is sharp, scale by scale, from sums the GPU formed.

`gc_spec_field` / `gc_ens_spectrum` (include/gencast_hip.h) analyse fields on the model's
equiangular grid with poles into the real orthonormal Y_lm that `noise.py` synthesises with and return the power per
total wavenumber l.  This module builds the analysis tables (`SphericalAnalysis`) and keeps what comes back
(`EnsembleSpectra`).  Per (batch, channel, l) the device hands over six raw sums over the M members x_i, the truth y
and the ensemble mean (formed on the coefficients):

  P0 = power(y)               P1 = sum_i power(x_i)      P2 = power(mean)
  P3 = sum_i power(x_i - y)   P4 = power(mean - y)       P5 = sum_i power(x_i - mean)

They are additive over initial dates (`merge`); everything else is derived on demand:

  member_power = P1/M    power_ratio = member_power/P0    error_power = P3/M    spread_power = P5/(M-1)
  spectral spread/skill = sqrt((M+1)/M spread_power / P4)

There is no NumPy transform in here: the analysis exists on the device only (the float64 yardstick of the tests is
tests/spectrum_reference.py).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from . import datasets
from .noise import _normalized_legendre
from .verification import AdditiveScores

MAX_CONDITION = 1e3


class SphericalAnalysis:
  """The tables of the analysis on a lat/lon grid (degrees; latitudes ascending with the poles, lon_j = 360 j / n_lon),
  band limit 0 <= m <= l < lmax <= n_lon / 2 (default n_lon / 2: the band of the noise generator).

  Fourier step, exact on this grid for m < n_lon / 2:  cos_a[m, j] = amp_m cos(m phi_j) / n_lon (amp_0 = 1, else sqrt 2),
  sin_a likewise.  Legendre step by least squares, not quadrature -- the latitudes cannot integrate products of degree
  2 lmax: for every m, A_m[lat, l] = N_lm P_l^m(sin lat), l = m .. lmax-1, and legendre_analysis[m, l, :] = pinv(A_m)
  (zero for l < m).  A field band-limited below lmax is recovered exactly.  Built in float64, handed over as float32.
  Raises ValueError when a condition number of an A_m exceeds 1e3 (e.g. n_lat < lmax)."""

  def __init__(self, lat, lon, lmax: Optional[int] = None):
    lat = np.asarray(lat, np.float64)
    lon = np.asarray(lon, np.float64)
    if lat.ndim != 1 or lon.ndim != 1 or not np.all(np.diff(lat) > 0):
      raise ValueError("Latitude values are expected to be sorted.")
    self.n_lat, self.n_lon = lat.shape[0], lon.shape[0]
    if not np.allclose(lon, lon[0] + np.arange(self.n_lon) * (360.0 / self.n_lon), atol=1e-4) or abs(lon[0]) > 1e-4:
      raise ValueError("longitudes must be 360 j / n_lon, j = 0 .. n_lon - 1")
    self.lmax = max(1, self.n_lon // 2) if lmax is None else int(lmax)
    if not 1 <= self.lmax <= self.n_lon // 2:
      raise ValueError(f"lmax must be in 1 .. n_lon / 2 = {self.n_lon // 2}, got {self.lmax}")
    L = self.lmax
    P = _normalized_legendre(np.sin(np.deg2rad(lat)), L)                       # [m, l, lat]
    self.legendre = P                                                          # [m, l, lat]: N_lm P_l^m(sin lat), zero for l < m
    self.legendre_analysis = np.zeros((L, L, self.n_lat), np.float64)
    self.condition_numbers = np.zeros(L, np.float64)
    for m in range(L):
      A = P[m, m:, :].T                                                        # [lat, l - m]
      sv = np.linalg.svd(A, compute_uv=False)
      self.condition_numbers[m] = np.inf if sv[-1] == 0.0 or A.shape[0] < A.shape[1] else sv[0] / sv[-1]
      if not self.condition_numbers[m] <= MAX_CONDITION:
        raise ValueError(f"the Legendre synthesis matrix of m = {m} has condition number {self.condition_numbers[m]:.3g} "
                         f"> {MAX_CONDITION:g} on {self.n_lat} latitudes with lmax = {L}: lower lmax")
      self.legendre_analysis[m, m:, :] = np.linalg.pinv(A)
    phi = 2.0 * np.pi * np.arange(self.n_lon) / self.n_lon
    m = np.arange(L, dtype=np.float64)
    amp = np.where(m == 0, 1.0, np.sqrt(2.0)) / self.n_lon
    self.cos_a = np.cos(m[:, None] * phi[None, :]) * amp[:, None]              # [m, lon]
    self.sin_a = np.sin(m[:, None] * phi[None, :]) * amp[:, None]              # [m, lon] (m = 0: zeros)
    amp_s = np.where(m == 0, 1.0, np.sqrt(2.0))
    self.cos_s = np.cos(m[:, None] * phi[None, :]) * amp_s[:, None]            # [m, lon]: amp_m cos(m phi_j), the synthesis rows
    self.sin_s = np.sin(m[:, None] * phi[None, :]) * amp_s[:, None]

  @property
  def worst_condition(self) -> float:
    return float(self.condition_numbers.max())

  def device_tables(self):
    """(legendre_analysis [lmax, lmax, n_lat], cos_a [lmax, n_lon], sin_a [lmax, n_lon]) float32, for
    `gc_spec_set_tables` / `NativeDenoiser.spec_set_tables`."""
    return (np.ascontiguousarray(self.legendre_analysis, np.float32), np.ascontiguousarray(self.cos_a, np.float32),
            np.ascontiguousarray(self.sin_a, np.float32))

  def synthesis_tables(self):
    """(legendre_synthesis [lmax m, n_lat, lmax l] (the plain A_m, zero for l < m), cos_s [lmax, n_lon], sin_s [lmax, n_lon])
    float32, for `gc_ens_band_set` / `NativeDenoiser.ens_band_set`: the way back from the coefficients of `device_tables`
    onto the grid, cos_s[m, j] = amp_m cos(m phi_j)."""
    leg = np.where((np.arange(self.lmax)[:, None] <= np.arange(self.lmax)[None, :])[:, :, None], self.legendre[:self.lmax, :self.lmax], 0.0)
    return (np.ascontiguousarray(np.transpose(leg, (0, 2, 1)), np.float32), np.ascontiguousarray(self.cos_s, np.float32),
            np.ascontiguousarray(self.sin_s, np.float32))

  @staticmethod
  def for_template(template, lmax: Optional[int] = None) -> "SphericalAnalysis":
    template = datasets.as_dataset(template)
    lat, lon = template.coords.get("lat"), template.coords.get("lon")
    if lat is None or lon is None:
      raise ValueError("template must have 'lat' and 'lon' coordinates")
    return SphericalAnalysis(lat, lon, lmax)


def ensure_tables(native, template, lmax: Optional[int] = None) -> int:
  """Hands the analysis tables of the template's grid to `native` unless it holds them already; -> lmax."""
  template = datasets.as_dataset(template)
  lat, lon = template.coords.get("lat"), template.coords.get("lon")
  if lat is None or lon is None:
    raise ValueError("template must have 'lat' and 'lon' coordinates")
  want = max(1, len(lon) // 2) if lmax is None else int(lmax)
  key = (len(lat), len(lon), want)
  if getattr(native, "_spec_key", None) != key:
    native.spec_set_tables(*SphericalAnalysis(lat, lon, want).device_tables())
    native._spec_key = key  # pylint: disable=protected-access
  return want


class EnsembleSpectra(AdditiveScores):
  """Raw sums [B, c_out, lmax, 6] float64, the member count M and the number of dates merged (`merge`: spectra over the union
  of the dates the parts covered: raw sums and date counts add)."""

  NAMES = ("truth_power", "member_power", "mean_power", "power_ratio", "error_power", "mean_error_power", "spread_power",
           "spectral_spread_skill")
  _adds = ("sums", "n_dates")
  _listed = NAMES
  _what = "spectra"

  def __init__(self, sums, n_members: int, n_dates: int = 1):
    self.sums = np.asarray(sums, dtype=np.float64)
    self.n_members, self.n_dates = int(n_members), int(n_dates)
    if self.n_members < 2:
      raise ValueError("n_members must be >= 2")
    if self.n_dates < 1:
      raise ValueError("n_dates must be >= 1")
    if self.sums.ndim != 4 or self.sums.shape[-1] != 6:
      raise ValueError(f"sums must be [batch, channels, lmax, 6], got {self.sums.shape}")

  def _p(self, k: int) -> np.ndarray:
    return self.sums[..., k] / self.n_dates

  @property
  def lmax(self) -> int:
    return self.sums.shape[2]

  @property
  def truth_power(self) -> np.ndarray:
    return self._p(0)

  @property
  def member_power(self) -> np.ndarray:
    """The mean over members (and dates) of a member's power: what `truth_power` is to be compared with."""
    return self._p(1) / self.n_members

  @property
  def mean_power(self) -> np.ndarray:
    """Of the ensemble mean: below `member_power` wherever the members disagree."""
    return self._p(2)

  @property
  def power_ratio(self) -> np.ndarray:
    """member_power / truth_power: 1 for members as sharp as the truth, < 1 blurred, > 1 over-sharpened."""
    return self.member_power / self.truth_power

  @property
  def error_power(self) -> np.ndarray:
    """Of a member's error x_i - y, mean over members."""
    return self._p(3) / self.n_members

  @property
  def mean_error_power(self) -> np.ndarray:
    """Of the ensemble mean's error."""
    return self._p(4)

  @property
  def spread_power(self) -> np.ndarray:
    """sum_i power(x_i - mean) / (M - 1): the ensemble variance, scale by scale."""
    return self._p(5) / (self.n_members - 1)

  @property
  def spectral_spread_skill(self) -> np.ndarray:
    """sqrt((M+1)/M spread_power / mean_error_power): 1 at every l for a calibrated ensemble of any size."""
    m = float(self.n_members)
    return np.sqrt((m + 1.0) / m * self.spread_power / self.mean_error_power)

  def scaled(self, channel_scale) -> "EnsembleSpectra":
    """The spectra of a x in place of x (members and truth alike), a = channel_scale [c_out]: every power times a^2.
    Offsets are not supported: a constant b added to a field moves l = 0 only, through a cross term with the field's
    own mean that the sums do not hold (the error and spread spectra P3, P4, P5 do not depend on b at all)."""
    a = np.asarray(channel_scale, dtype=np.float64).reshape(-1)
    if a.shape != (self.sums.shape[1],):
      raise ValueError(f"channel_scale must have shape ({self.sums.shape[1]},)")
    if np.any(a == 0.0) or not np.all(np.isfinite(a)):
      raise ValueError("channel_scale must be finite and non-zero")
    return EnsembleSpectra(self.sums * (a * a)[None, :, None, None], self.n_members, self.n_dates)

  def per_variable(self, template) -> Dict[str, Dict[str, np.ndarray]]:
    """{spectrum: {variable: [batch, channels of the variable, lmax]}} in the channel order of
    `datasets.channel_layout`."""
    with np.errstate(divide="ignore", invalid="ignore"):
      return super().per_variable(template)
