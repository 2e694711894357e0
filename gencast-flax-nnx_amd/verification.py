"""Ensemble verification: the scores a probabilistic forecaster is judged by, from sums the GPU formed.

`gc_ens_score` (include/gencast_hip.h) reduces M members against one truth on the device and hands back, per
(batch, channel) column, six raw double sums over the valid grid nodes and the integer rank counts:

  S0 = sum w          S1 = sum w (m - y)     S2 = sum w (m - y)^2
  S3 = sum w s2       S4 = sum w mean_i |x_i - y|      S5 = sum w mean_{i<j} |x_i - x_j|

(m: ensemble mean, s2: the M-1 variance, w: node weight).  `EnsembleScores` keeps them raw, because raw sums are
additive -- batches, initial dates and ranks merge by `merge` -- and derives everything else on demand:

  rmse = sqrt(S2/S0)    spread = sqrt(S3/S0)    spread/skill = sqrt((M+1)/M) spread / rmse    bias = S1/S0
  fair CRPS = (S4 - S5/2)/S0      ensemble CRPS = (S4 - (M-1)/M S5/2)/S0

There is no NumPy implementation of the metrics in here: the per-point work exists on the device only.

Events (`gc_ens_event_score`): for T threshold fields with a direction each, the device counts at
every valid point k = the members inside the event and o = whether the truth is, and hands back per (threshold, batch,
channel) the integer table `weighted[o][k]` = sum of the quantised node weights (`quantize_node_weights`) and `counts[o][k]`.
`EventScores` keeps the tables raw (they add over dates, exactly) and derives the Brier score with its decomposition,
the reliability curve, the ROC and the relative economic value; `EventSpec` carries thresholds given per variable in
physical units down to the packed fields; `event_probability` decodes the per-point bytes the device keeps.

Derived fields (`gc_ens_derive`): `DerivedSpec` names variables that are no model channels (wind speed:
the norm of two components, in physical units) and one spatial pooling (max, min or area-weighted mean over a neighbourhood
of fixed great-circle radius); the device forms them from a member store into the store of a second handle, where every
scorer above works unchanged.  The same spec forms combinations across pressure levels (sums and norms of terms coef a b:
thickness, shear, column integrals, integrated vapour transport, one level of a variable) and horizontal derivatives on the
sphere (relative vorticity, divergence), through `gc_ens_derive_set_expr`.

Band views (`gc_ens_band`): `BandSpec` names bands of total wavenumbers; the device analyses the members
and the truth of a store into spherical harmonics, weights the coefficients with the band's response and synthesises them back
into the store of a second handle -- low-, band- and true high-pass fields, on which every scorer works unchanged.

Order statistics (`gc_ens_order_score`): the device sorts the M members of every point and hands back,
per (batch, channel), the bin sums `bins[k] = (sum w alpha_k, sum w beta_k)` of Hersbach's (2000) decomposition of the
ensemble CRPS, the outlier weights, and for Q probabilities the pinball-loss sums and below-quantile counts of the quantile
fields it leaves on the device.  `OrderScores` keeps them raw and derives reliability and potential CRPS.

Skill against a climatology (`gc_ens_clim_score`): the device reads the M members and, from the store
of a second handle, K climatological samples of every point, and hands back twelve raw sums per (batch, channel).
`ClimatologyScores` keeps them raw and derives the anomaly correlation of the ensemble mean and the CRPS skill score.

Multivariate scores (`gc_ens_energy_score`, `gc_ens_variogram_score`): every score above is marginal.
For `EnergySpec` groups of channels the device hands back the weighted squared distances D2 between every pair of the
M + 1 fields (members and truth) and `EnergyScores` derives the energy score; for `VariogramSpec` grid offsets it hands
back four additive sums per (batch, channel, offset) and `VariogramScores` derives the variogram score and the roughness
of the members against the truth's.

Tail skill (`gc_ens_tail_score`): the threshold-weighted CRPS of Gneiting & Ranjan (2011) in the
chaining form of Allen et al. (2023) -- the plain CRPS of members and truth clamped at a threshold from one side.  The
thresholds and directions are an `EventSpec`; the device sorts the members of a point once and hands back four raw sums per
(threshold, batch, channel).  `TailScores` keeps them raw and derives the fair and the ensemble twCRPS.

Fractions (`gc_ens_fss_score`): every event score above is point-wise.  An `EventSpec` with `scales_km`
also gets, from the code bytes of the events, the neighbourhood ensemble probability against the observed fraction at up to
eight radii; `FractionsScores` keeps the four raw sums per (threshold, scale, batch, channel) and derives the fractions skill
score and the smallest skilful scale.  It rides on `EventScores.fractions`.

The Extreme Forecast Index (`gc_ens_efi_*`): the members ranked, point by point, in the K samples of that
second handle -- how far the forecast distribution is shifted against the climatological one, weighted towards the tails.
`efi_table` makes the table the device looks up, `EfiSpec` names the climatological events of the truth the index is verified
against, `EfiScores` keeps the raw sums and integer tables and derives the mean index, its correlation with the observed
index and the ROC.

Score maps (`gc_ens_map_*`): the marginal scores kept per grid point and added up over dates on the
device, one set of planes per slot (a lead time).  `MapSpec` selects the channels, `ScoreMaps` keeps the raw planes and
derives bias, RMSE, spread/skill, the fair CRPS with its standard error and the outlier frequencies per point, `EventMaps`
the Brier score, base rate and forecast probability per point; both merge over dates and reduce to any region after the fact.

Regions (`gc_ens_region_score`): the sums of `EnsembleScores` per named set of grid nodes -- tropics,
extratropics, land, sea, boxes -- every region from one pass over the nodes that belong to any.  `RegionSpec` holds the masks
and builds boxes from bounds; `RegionScores[name]` is the region's `EnsembleScores`.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import datasets, losses


class AdditiveScores:
  """What the score classes made of raw, additive sums share.  A class states `_adds`: the attributes that add (the first of
  them the array whose shape the parts must share and whose `_channel_axis` is the channel axis), `_same`: {attribute that must
  be equal across parts: the word for it in the message}, and `_listed`: the properties `per_variable` lists.  The constructor
  takes all of them by these names."""
  _adds: Tuple[str, ...] = ()
  _same: Mapping[str, str] = {"n_members": "members"}
  _listed: Tuple[str, ...] = ()
  _channel_axis = 1
  _what = "scores"

  @classmethod
  def merge(cls, parts):
    """Scores over the union of what the parts covered (other nodes, other dates): raw sums and counts add."""
    parts = list(parts)
    if not parts:
      raise ValueError("merge: nothing to merge")
    first = parts[0]
    for p in parts[1:]:
      if (any(getattr(p, f) != getattr(first, f) for f in cls._same)
          or getattr(p, cls._adds[0]).shape != getattr(first, cls._adds[0]).shape):
        raise ValueError(f"merge: the parts differ in {', '.join(cls._same.values())} or shape")
    total = {a: np.copy(getattr(first, a)) for a in cls._adds}
    for p in parts[1:]:
      for a in cls._adds:
        total[a] += getattr(p, a)
    return cls(**total, **{f: getattr(first, f) for f in cls._same})

  def per_variable(self, template) -> Dict[str, Dict[str, np.ndarray]]:
    """{score: {variable: [leading axes, channels of the variable, ...]}} in the channel order of `datasets.channel_layout`
    (`EnsembleScores`, for a variable with levels and one time step: (batch, level)); the leading axes are batch, after the
    thresholds where the class has them."""
    layout = datasets.channel_layout(datasets.as_dataset(template))
    channels = getattr(self, self._adds[0]).shape[self._channel_axis]
    if sum(n for _, _, n in layout) != channels:
      raise ValueError(f"template has {sum(n for _, _, n in layout)} channels, the {self._what} {channels}")
    lead = (slice(None),) * self._channel_axis
    out: Dict[str, Dict[str, np.ndarray]] = {}
    for score in self._listed:
      values = getattr(self, score)
      out[score] = {name: values[lead + (slice(off, off + n),)] for name, off, n in layout}
    return out


class EnsembleScores(AdditiveScores):
  """Raw sums [B, c_out, 6] float64, rank histogram [B, c_out, M + 1] uint64 and the member count M."""
  _adds = ("sums", "rank_histogram")
  _listed = ("rmse", "spread", "spread_skill_ratio", "crps", "crps_ensemble", "bias", "valid_weight", "rank_histogram")

  def __init__(self, sums, rank_histogram, n_members: int):
    self.sums = np.asarray(sums, dtype=np.float64)
    self.rank_histogram = np.asarray(rank_histogram, dtype=np.uint64)
    self.n_members = int(n_members)
    if self.n_members < 2:
      raise ValueError("n_members must be >= 2")
    if self.sums.ndim != 3 or self.sums.shape[-1] != 6:
      raise ValueError(f"sums must be [batch, channels, 6], got {self.sums.shape}")
    if self.rank_histogram.shape != self.sums.shape[:2] + (self.n_members + 1,):
      raise ValueError(f"rank_histogram must be {self.sums.shape[:2] + (self.n_members + 1,)}, "
                       f"got {self.rank_histogram.shape}")

  def _s(self, k: int) -> np.ndarray:
    return self.sums[..., k]

  @property
  def valid_weight(self) -> np.ndarray:
    """S0: the node weight of the points that counted, per (batch, channel)."""
    return self._s(0)

  @property
  def valid_points(self) -> np.ndarray:
    return self.rank_histogram.sum(axis=-1)

  @property
  def bias(self) -> np.ndarray:
    return self._s(1) / self._s(0)

  @property
  def rmse(self) -> np.ndarray:
    """Of the ensemble mean."""
    return np.sqrt(self._s(2) / self._s(0))

  @property
  def spread(self) -> np.ndarray:
    return np.sqrt(self._s(3) / self._s(0))

  @property
  def spread_skill_ratio(self) -> np.ndarray:
    """sqrt((M+1)/M) spread / rmse: 1 for a calibrated ensemble of any size."""
    m = float(self.n_members)
    return np.sqrt((m + 1.0) / m) * self.spread / self.rmse

  @property
  def crps(self) -> np.ndarray:
    """The fair CRPS: unbiased for the CRPS of the distribution the members were drawn from."""
    return (self._s(4) - 0.5 * self._s(5)) / self._s(0)

  @property
  def crps_ensemble(self) -> np.ndarray:
    """The CRPS of the M-member empirical distribution (pair term normalised by M^2)."""
    m = float(self.n_members)
    return (self._s(4) - 0.5 * (m - 1.0) / m * self._s(5)) / self._s(0)

  def scaled(self, channel_scale) -> "EnsembleScores":
    """The scores of a x + b in place of x (members and truth alike), a = channel_scale [c_out], any b: S1, S4 and S5
    scale with |a| (S1 with a), S2 and S3 with a^2; ranks are unchanged for a > 0 and mirrored for a < 0."""
    a = np.asarray(channel_scale, dtype=np.float64).reshape(-1)
    if a.shape != (self.sums.shape[1],):
      raise ValueError(f"channel_scale must have shape ({self.sums.shape[1]},)")
    if np.any(a == 0.0) or not np.all(np.isfinite(a)):
      raise ValueError("channel_scale must be finite and non-zero")
    f = np.stack([np.ones_like(a), a, a * a, a * a, np.abs(a), np.abs(a)], axis=-1)
    hist = np.where((a < 0.0)[None, :, None], self.rank_histogram[..., ::-1], self.rank_histogram)
    return EnsembleScores(self.sums * f[None], hist, self.n_members)

  @staticmethod
  def node_weights(template) -> np.ndarray:
    return node_weights(template)


def node_weights(template) -> np.ndarray:
  """[G] float32: `losses.normalized_latitude_weights` (unit mean), the same for every longitude of a latitude row
  (node = lat_i * n_lon + lon_j)."""
  template = datasets.as_dataset(template)
  sizes = template.sizes
  if "lat" not in sizes or "lon" not in sizes:
    raise ValueError("template must have 'lat' and 'lon' dimensions")
  return np.repeat(losses.normalized_latitude_weights(template), sizes["lon"]).astype(np.float32)


# ---------------------------------------------------------------------------------------------
# order statistics: quantiles and the reliability / potential split of the CRPS (gc_ens_order_*)
# ---------------------------------------------------------------------------------------------
class OrderScores(AdditiveScores):
  """The raw sums of `gc_ens_order_score`: `bins` [B, c_out, M + 1, 2] float64 (A_k = sum w alpha_k, B_k = sum w beta_k),
  `extra` [B, c_out, 3] (S0 = sum w, O_lo = sum w [y < x_(1)], O_hi = sum w [y > x_(M)]), `pinball` [B, c_out, Q],
  `counts` [B, c_out, Q + 1] uint64 (points with y < Q_q; last: the counted points), with the member count M and the
  probabilities [Q].  With p_k = k / M (Hersbach 2000):

    g_k = (A_k + B_k) / S0,  o_k = B_k / (A_k + B_k)                 0 < k < M
    o_0 = O_lo / S0,  g_0 = B_0 / O_lo;    o_M = 1 - O_hi / S0,  g_M = A_M / O_hi        (a zero denominator: g = 0)
    reliability = sum g_k (o_k - p_k)^2      crps_potential = sum g_k o_k (1 - o_k)
    crps_ensemble = sum (A_k p_k^2 + B_k (1 - p_k)^2) / S0 = reliability + crps_potential

  `crps_ensemble` is `EnsembleScores.crps_ensemble` of the same store.  Hersbach's further split of the potential CRPS into
  uncertainty and resolution needs the climatological distribution of the observations, which is not additive over dates:
  it is not formed here."""
  _adds = ("bins", "extra", "pinball", "counts")
  _same = {"n_members": "members", "probs": "probabilities"}
  _listed = ("crps_ensemble", "reliability", "crps_potential", "outlier_low", "outlier_high", "bin_width", "bin_frequency",
             "quantile_score", "quantile_coverage", "valid_weight", "valid_points")

  def __init__(self, bins, extra, pinball, counts, n_members: int, probs):
    self.bins = np.asarray(bins, dtype=np.float64)
    self.extra = np.asarray(extra, dtype=np.float64)
    self.n_members = int(n_members)
    self.probs = tuple(float(p) for p in np.asarray([] if probs is None else probs, dtype=np.float64).reshape(-1))
    if self.n_members < 2:
      raise ValueError("n_members must be >= 2")
    if self.bins.ndim != 4 or self.bins.shape[-2:] != (self.n_members + 1, 2):
      raise ValueError(f"bins must be [batch, channels, {self.n_members + 1}, 2], got {self.bins.shape}")
    lead, nq = self.bins.shape[:2], len(self.probs)
    if self.extra.shape != lead + (3,):
      raise ValueError(f"extra must be {lead + (3,)}, got {self.extra.shape}")
    self.pinball = np.asarray(pinball, dtype=np.float64).reshape(lead + (nq,)) if nq == 0 else np.asarray(pinball, dtype=np.float64)
    self.counts = np.asarray(counts, dtype=np.uint64)
    if self.pinball.shape != lead + (nq,):
      raise ValueError(f"pinball must be {lead + (nq,)}, got {self.pinball.shape}")
    if self.counts.shape != lead + (nq + 1,):
      raise ValueError(f"counts must be {lead + (nq + 1,)}, got {self.counts.shape}")

  @staticmethod
  def _ratio0(a, b) -> np.ndarray:
    """a / b, zero where b is zero."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    out = np.zeros(a.shape)
    np.divide(a, b, out=out, where=b != 0.0)
    return out

  @property
  def _p(self) -> np.ndarray:
    return np.arange(self.n_members + 1, dtype=np.float64) / float(self.n_members)

  @property
  def valid_weight(self) -> np.ndarray:
    """S0: the node weight of the points that counted, per (batch, channel)."""
    return self.extra[..., 0]

  @property
  def valid_points(self) -> np.ndarray:
    return self.counts[..., -1]

  @property
  def outlier_low(self) -> np.ndarray:
    """The weighted frequency of a truth below every member."""
    return self.extra[..., 1] / self.extra[..., 0]

  @property
  def outlier_high(self) -> np.ndarray:
    return self.extra[..., 2] / self.extra[..., 0]

  @property
  def bin_width(self) -> np.ndarray:
    """g_k [B, c_out, M + 1]: the mean width of bin k (for the two end bins: the mean distance of an outlier)."""
    a, b = self.bins[..., 0], self.bins[..., 1]
    g = (a + b) / self.extra[..., 0:1]
    g[..., 0] = self._ratio0(b[..., 0], self.extra[..., 1])
    g[..., -1] = self._ratio0(a[..., -1], self.extra[..., 2])
    return g

  @property
  def bin_frequency(self) -> np.ndarray:
    """o_k [B, c_out, M + 1]: how often the truth lay below the middle of bin k -- p_k = k / M for a reliable ensemble."""
    a, b = self.bins[..., 0], self.bins[..., 1]
    o = self._ratio0(b, a + b)
    o[..., 0] = self.extra[..., 1] / self.extra[..., 0]
    o[..., -1] = 1.0 - self.extra[..., 2] / self.extra[..., 0]
    return o

  @property
  def reliability(self) -> np.ndarray:
    return (self.bin_width * (self.bin_frequency - self._p) ** 2).sum(axis=-1)

  @property
  def crps_potential(self) -> np.ndarray:
    o = self.bin_frequency
    return (self.bin_width * o * (1.0 - o)).sum(axis=-1)

  @property
  def crps_ensemble(self) -> np.ndarray:
    """The CRPS of the M-member empirical distribution, from the bin sums: reliability + crps_potential."""
    p = self._p
    return (self.bins[..., 0] * p ** 2 + self.bins[..., 1] * (1.0 - p) ** 2).sum(axis=-1) / self.extra[..., 0]

  @property
  def quantile_score(self) -> np.ndarray:
    """[B, c_out, Q]: the mean pinball loss of quantile field q."""
    return self.pinball / self.extra[..., 0:1]

  @property
  def quantile_coverage(self) -> np.ndarray:
    """[B, c_out, Q]: the fraction of counted points with the truth below quantile field q (p_q when reliable)."""
    return self.counts[..., :-1].astype(np.float64) / self.counts[..., -1:].astype(np.float64)

  def scaled(self, channel_scale) -> "OrderScores":
    """The scores of a x + b in place of x (members and truth alike), a = channel_scale [c_out] > 0, any b: the bin sums and
    the pinball sums scale with a; weights and counts do not change.  (a < 0 would reverse the order of the members.)"""
    a = np.asarray(channel_scale, dtype=np.float64).reshape(-1)
    if a.shape != (self.bins.shape[1],):
      raise ValueError(f"channel_scale must have shape ({self.bins.shape[1]},)")
    if not np.all(np.isfinite(a) & (a > 0.0)):
      raise ValueError("channel_scale must be finite and > 0")
    return OrderScores(self.bins * a[None, :, None, None], self.extra, self.pinball * a[None, :, None], self.counts,
                       self.n_members, self.probs)


# ---------------------------------------------------------------------------------------------
# skill against a climatology: anomaly correlation and CRPS skill score (gc_ens_clim_score)
# ---------------------------------------------------------------------------------------------
class ClimatologyScores(AdditiveScores):
  """The raw sums of `gc_ens_clim_score`: `sums` [B, c_out, 12] float64 and `counts` [B, c_out] uint64 (counted points),
  with the member count M, the number K of climatological samples and the points `invalid` that did not count.  With m
  the ensemble mean, cbar the mean of the K samples, fa = m - cbar, oa = y - cbar, ae the mean |. - y| and d the mean
  absolute difference over the pairs, of the members (x) and of the samples (c):

    sums[..., 0:8]  = A0 .. A7 = sum w (1, fa, oa, fa oa, fa^2, oa^2, mean_i (x_i - cbar)^2, (m - y)^2)
    sums[..., 8:12] = F4, F5, C4, C5 = sum w (ae_x, d_x, ae_c, d_c)

  Every derived score is [B, c_out]; a zero denominator gives NaN, not an error."""

  N_SUMS = 12
  _adds = ("sums", "counts", "invalid")
  _same = {"n_members": "members", "n_climatology": "climatological samples"}
  _listed = ("acc", "acc_centred", "acc_members", "crps", "crps_climatology", "crpss", "crps_ensemble",
             "crps_climatology_ensemble", "crpss_ensemble", "msss", "rmse", "rmse_climatology", "valid_weight", "valid_points")

  def __init__(self, sums, counts, n_members: int, n_climatology: int, invalid: int = 0):
    self.sums = np.asarray(sums, dtype=np.float64)
    self.counts = np.asarray(counts, dtype=np.uint64)
    self.n_members, self.n_climatology, self.invalid = int(n_members), int(n_climatology), int(invalid)
    if self.n_members < 2 or self.n_climatology < 2:
      raise ValueError("n_members and n_climatology must be >= 2")
    if self.sums.ndim != 3 or self.sums.shape[-1] != self.N_SUMS:
      raise ValueError(f"sums must be [batch, channels, {self.N_SUMS}], got {self.sums.shape}")
    if self.counts.shape != self.sums.shape[:2]:
      raise ValueError(f"counts must be {self.sums.shape[:2]}, got {self.counts.shape}")

  def _s(self, k: int) -> np.ndarray:
    return self.sums[..., k]

  @staticmethod
  def _ratio(a, b) -> np.ndarray:
    """a / b, NaN where b is zero (or not a number)."""
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    out = np.full(a.shape, np.nan)
    np.divide(a, b, out=out, where=(b != 0.0) & ~np.isnan(b))
    return out

  @classmethod
  def _root(cls, a) -> np.ndarray:
    """sqrt(a), NaN where a < 0 (a variance that rounding made negative)."""
    a = np.asarray(a, np.float64)
    return np.sqrt(np.where(a >= 0.0, a, np.nan))

  @property
  def valid_weight(self) -> np.ndarray:
    """A0: the node weight of the points that counted, per (batch, channel)."""
    return self._s(0)

  @property
  def valid_points(self) -> np.ndarray:
    return self.counts

  @property
  def acc(self) -> np.ndarray:
    """The anomaly correlation coefficient of the ensemble mean, uncentred (the form WeatherBench uses):
    sum w fa oa / sqrt(sum w fa^2 sum w oa^2)."""
    return self._ratio(self._s(3), self._root(self._s(4) * self._s(5)))

  @property
  def acc_centred(self) -> np.ndarray:
    """The anomaly correlation with the weighted mean anomalies removed from both sides."""
    a0 = self._s(0)
    mf, mo = self._ratio(self._s(1), a0), self._ratio(self._s(2), a0)
    cov = self._ratio(self._s(3), a0) - mf * mo
    vf, vo = self._ratio(self._s(4), a0) - mf * mf, self._ratio(self._s(5), a0) - mo * mo
    return self._ratio(cov, self._root(vf * vo))

  @property
  def acc_members(self) -> np.ndarray:
    """The anomaly correlation with the mean square member anomaly in place of the square of the mean anomaly: what a
    single member scores on average, where `acc` gains from the averaging."""
    return self._ratio(self._s(3), self._root(self._s(6) * self._s(5)))

  @property
  def crps(self) -> np.ndarray:
    """The fair CRPS of the forecast (`EnsembleScores.crps` of the same store)."""
    return self._ratio(self._s(8) - 0.5 * self._s(9), self._s(0))

  @property
  def crps_ensemble(self) -> np.ndarray:
    """The CRPS of the M-member empirical distribution (pair term times (M - 1) / M)."""
    m = float(self.n_members)
    return self._ratio(self._s(8) - 0.5 * (m - 1.0) / m * self._s(9), self._s(0))

  @property
  def crps_climatology(self) -> np.ndarray:
    """The fair CRPS of the K climatological samples taken as a forecast."""
    return self._ratio(self._s(10) - 0.5 * self._s(11), self._s(0))

  @property
  def crps_climatology_ensemble(self) -> np.ndarray:
    """The CRPS of the K-sample empirical distribution (pair term times (K - 1) / K)."""
    k = float(self.n_climatology)
    return self._ratio(self._s(10) - 0.5 * (k - 1.0) / k * self._s(11), self._s(0))

  @property
  def crpss(self) -> np.ndarray:
    """The CRPS skill score 1 - crps / crps_climatology: 1 perfect, 0 no better than the climatology."""
    return 1.0 - self._ratio(self.crps, self.crps_climatology)

  @property
  def crpss_ensemble(self) -> np.ndarray:
    return 1.0 - self._ratio(self.crps_ensemble, self.crps_climatology_ensemble)

  @property
  def msss(self) -> np.ndarray:
    """The mean-square skill score of the ensemble mean against the climatological mean, 1 - A7 / A5."""
    return 1.0 - self._ratio(self._s(7), self._s(5))

  @property
  def rmse(self) -> np.ndarray:
    """Of the ensemble mean (`EnsembleScores.rmse` of the same store where the climatology is finite)."""
    return self._root(self._ratio(self._s(7), self._s(0)))

  @property
  def rmse_climatology(self) -> np.ndarray:
    """Of the climatological mean taken as a forecast."""
    return self._root(self._ratio(self._s(5), self._s(0)))

  def scaled(self, channel_scale) -> "ClimatologyScores":
    """The sums of a x + b in place of x (members, samples and truth alike), a = channel_scale [c_out], any b(point): A1
    and A2 scale with a, F4, F5, C4 and C5 with |a|, A3 .. A7 with a^2; b drops out of every term."""
    a = np.asarray(channel_scale, dtype=np.float64).reshape(-1)
    if a.shape != (self.sums.shape[1],):
      raise ValueError(f"channel_scale must have shape ({self.sums.shape[1]},)")
    if np.any(a == 0.0) or not np.all(np.isfinite(a)):
      raise ValueError("channel_scale must be finite and non-zero")
    one, sq, ab = np.ones_like(a), a * a, np.abs(a)
    f = np.stack([one, a, a, sq, sq, sq, sq, sq, ab, ab, ab, ab], axis=-1)
    return ClimatologyScores(self.sums * f[None], self.counts, self.n_members, self.n_climatology, self.invalid)


# ---------------------------------------------------------------------------------------------
# events: exceedance probabilities against thresholds (gc_ens_event_*)
# ---------------------------------------------------------------------------------------------
_U32_MAX = 4294967295


def quantize_node_weights(w) -> Tuple[np.ndarray, float]:
  """-> (wq [G] uint32, scale): wq = rint(w scale) in float64, scale = 2^e with e the largest integer for which
  max(w) 2^e <= 2^32 - 1.  The device adds wq as integers, so sums are exact and have no order; a column total is at most
  G (2^32 - 1), below 2^53 for G <= 2^21, so `total / scale` in float64 is exact too.  `w` must be finite, >= 0 and not
  all zero (ValueError)."""
  w = np.asarray(w, dtype=np.float64).reshape(-1)
  if w.size == 0 or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not np.any(w > 0.0):
    raise ValueError("node weights must be finite, >= 0 and not all zero")
  top = float(w.max())
  e = int(math.floor(math.log2(_U32_MAX / top)))
  while math.ldexp(top, e + 1) <= _U32_MAX:               # (ldexp by a power of two is exact: the comparisons are)
    e += 1
  while math.ldexp(top, e) > _U32_MAX:
    e -= 1
  scale = math.ldexp(1.0, e)
  return np.rint(w * scale).astype(np.uint32), scale


def quantize_row_weights(w, bits: int = 24) -> np.ndarray:
  """-> row_wq [n_lat] uint32: max(1, rint(w 2^e)) in float64 with e the largest integer for which max(w) 2^e <= 2^bits - 1:
  the integer latitude weights of the fractions windows (`gc_ens_fss_set`).  A row whose weight rounds to 0 -- the poles of
  an equiangular grid -- keeps 1: a counted centre always has a window of positive weight.  `w` must be finite, >= 0 and not
  all zero (ValueError), as in `quantize_node_weights`."""
  w = np.asarray(w, dtype=np.float64).reshape(-1)
  if w.size == 0 or not np.all(np.isfinite(w)) or np.any(w < 0.0) or not np.any(w > 0.0):
    raise ValueError("row weights must be finite, >= 0 and not all zero")
  if not 1 <= int(bits) <= 32:
    raise ValueError("bits must lie in 1..32")
  top, cap = float(w.max()), float(2 ** int(bits) - 1)
  e = int(math.floor(math.log2(cap / top)))
  while math.ldexp(top, e + 1) <= cap:                    # (ldexp by a power of two is exact: the comparisons are)
    e += 1
  while math.ldexp(top, e) > cap:
    e -= 1
  return np.maximum(1.0, np.rint(w * math.ldexp(1.0, e))).astype(np.uint32)


def event_probability(code, n_members: int) -> Tuple[np.ndarray, np.ndarray]:
  """The per-point bytes of `NativeDenoiser.ens_event_codes` -> (probability k / M as float32, NaN where the point did
  not count; observed flag as bool, False there)."""
  code = np.asarray(code, dtype=np.uint8)
  valid = code != 255
  k = (code & 127).astype(np.float32)
  prob = np.where(valid, k / np.float32(n_members), np.float32(np.nan)).astype(np.float32)
  return prob, valid & ((code >> 7) == 1)


class EventSpec:
  """Thresholds of T events, per target variable and in the physical units of the targets, with one direction per
  event (> 0: the event is `value > threshold`, < 0: `value < threshold`; both strict).

  `thresholds`: {variable: array}, leading axis T; the remaining axes broadcast, right-aligned, against the variable's
  dims other than batch and time (a scalar per event: shape (T,); per level: (T, level, 1, 1); a climatological map:
  (T, lat, lon)).  An array with one axis per dim of the variable after the leading one (batch and time included) is
  taken as the full field it is.  A target variable left out is NaN: not evaluated.  Values are cast to the dtype of the
  target variable, so a threshold and a target of equal value stay equal through every map both go through.

  `scales_km`: None, or 1..8 neighbourhood radii in km, ascending (0: the point itself; in a pole row, whose nodes are one
  point, the whole row, as `DerivedSpec.window` has it).  With them every `EventScores` of
  the spec carries `.fractions` (`FractionsScores`): the fractions skill score of the neighbourhood ensemble probability at
  each scale, over the great-circle windows of `DerivedSpec.window`."""

  def __init__(self, thresholds: Mapping[str, np.ndarray], directions: Sequence[int], scales_km: Optional[Sequence[float]] = None):
    self.directions = tuple(int(np.sign(d)) for d in directions)
    if not self.directions or any(d == 0 for d in self.directions):
      raise ValueError("directions must be non-empty and non-zero")
    self.scales_km = None
    self.fractions_plan = None                             # `windows(template)` of the last `packed(template)`
    if scales_km is not None:
      scales = tuple(float(r) for r in np.asarray(scales_km, dtype=np.float64).reshape(-1))
      if (not 1 <= len(scales) <= 8 or not all(math.isfinite(r) and r >= 0.0 for r in scales)
          or any(b <= a for a, b in zip(scales, scales[1:]))):
        raise ValueError("scales_km must be 1..8 finite radii >= 0 in ascending order")
      self.scales_km = scales
    self.thresholds = {k: np.asarray(v, dtype=np.float64) for k, v in thresholds.items()}
    for k, v in self.thresholds.items():
      if v.ndim < 1 or v.shape[0] != len(self.directions):
        raise ValueError(f"thresholds[{k!r}] must have a leading axis of length {len(self.directions)}, got {v.shape}")

  @property
  def n_thresholds(self) -> int:
    return len(self.directions)

  def fields(self, template) -> List[datasets.Dataset]:
    """T Datasets shaped like `template` (one per event), NaN for a variable without thresholds."""
    template = datasets.as_dataset(template)
    for name in self.thresholds:
      if name not in template:
        raise ValueError(f"thresholds given for {name!r}, which is not a target variable")
    out: List[Dict[str, datasets.Variable]] = [{} for _ in self.directions]
    for name, var in template.items():
      shape, dtype = np.shape(var.data), np.asarray(var.data).dtype
      thr = self.thresholds.get(name)
      if thr is None:
        full = np.full((self.n_thresholds,) + shape, np.nan, dtype)
      else:
        rest = [d for d in var.dims if d not in ("batch", "time")]
        if thr.ndim - 1 == len(var.dims) and len(var.dims) > len(rest):
          view = thr
        else:
          if thr.ndim - 1 > len(rest):
            raise ValueError(f"thresholds[{name!r}] has shape {thr.shape}: more axes than {tuple(rest)}")
          tail = (1,) * (len(rest) - (thr.ndim - 1)) + thr.shape[1:]
          sizes = dict(zip(rest, tail))
          view = thr.reshape((thr.shape[0],) + tuple(sizes.get(d, 1) for d in var.dims))
        full = np.broadcast_to(view, (self.n_thresholds,) + shape).astype(dtype)
      for t in range(self.n_thresholds):
        out[t][name] = datasets.Variable(var.dims, full[t])
    return [datasets.Dataset(v, template.coords) for v in out]

  def mapped(self, template, fn) -> "EventSpec":
    """The spec with every threshold field sent through `fn(name, Variable) -> Variable` (the map the targets go
    through under a normalisation wrapper); the result holds full fields."""
    fields = self.fields(template)
    names = list(datasets.as_dataset(template).keys())
    return EventSpec({name: np.stack([np.asarray(fn(name, f[name]).data) for f in fields]) for name in names},
                     self.directions, self.scales_km)

  def windows(self, template) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(r_lat [S] int32, r_lon [S, n_lat] int32, row_wq [n_lat] uint32): the arguments of `NativeDenoiser.ens_fss_set` --
    `DerivedSpec.window` of every scale on the grid of `template`, and its latitude weights
    (`losses.normalized_latitude_weights`) through `quantize_row_weights`."""
    if self.scales_km is None:
      raise ValueError("windows: the spec has no scales_km")
    coords = datasets.as_dataset(template).coords
    lat, lon = np.asarray(coords["lat"], np.float64), np.asarray(coords["lon"], np.float64)
    per_scale = [DerivedSpec.window(lat, lon, r) for r in self.scales_km]
    return (np.array([w[0] for w in per_scale], np.int32), np.stack([w[1] for w in per_scale]).astype(np.int32),
            quantize_row_weights(losses.normalized_latitude_weights(lat)))

  def packed(self, template) -> np.ndarray:
    """[T, G, B, c_out] float32 in the channel order of `datasets.channel_layout` (node = lat_i n_lon + lon_j).  With
    `scales_km` the windows of the same grid are kept as `fractions_plan`, for the store that counts the events."""
    template = datasets.as_dataset(template)
    if self.scales_km is not None:
      self.fractions_plan = self.windows(template)
    sizes = template.sizes
    out = []
    for f in self.fields(template):
      st = np.transpose(datasets.dataset_to_stacked(f, sizes), (1, 2, 0, 3))
      out.append(st.reshape((st.shape[0] * st.shape[1],) + st.shape[2:]))
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


class EventScores(AdditiveScores):
  """The integer tables of `gc_ens_event_score`: `weighted` and `counts` [T, B, c_out, 2, M + 1] uint64 (axis -2: the
  truth outside / inside the event, axis -1: k members inside), `invalid` [T] points skipped, with the member count M,
  the directions [T] and the `scale` of the quantised node weights.  Every derived score is [T, B, c_out] float64 (curves
  carry one more axis); a ratio whose denominator is zero -- the event never or always observed -- is NaN, not an error.

  With n_k = (weighted[0][k] + weighted[1][k]) / scale, o_k = weighted[1][k] / scale, N = sum n_k, O = sum o_k, s = O / N
  and p_k = k / M.  The bins are the distinct forecast values, so brier = reliability - resolution + uncertainty holds
  exactly in exact arithmetic."""
  _adds = ("weighted", "counts", "invalid")
  _same = {"n_members": "members", "directions": "directions", "scale": "scale"}
  _listed = ("base_rate", "brier", "brier_fair", "reliability", "resolution", "uncertainty", "brier_skill", "roc_area",
             "valid_weight", "valid_points")
  _channel_axis = 2
  fractions: Optional["FractionsScores"] = None            # the neighbourhood scores of an `EventSpec` with `scales_km`

  def __init__(self, weighted, counts, n_members: int, directions: Sequence[int], scale: float, invalid=None, *,
               fractions: Optional["FractionsScores"] = None):
    if fractions is not None:                              # (absent from `vars(scores)` unless the spec had `scales_km`)
      self.fractions = fractions
    self.weighted = np.asarray(weighted, dtype=np.uint64)
    self.counts = np.asarray(counts, dtype=np.uint64)
    self.n_members = int(n_members)
    self.directions = tuple(int(np.sign(d)) for d in directions)
    self.scale = float(scale)
    if self.n_members < 2:
      raise ValueError("n_members must be >= 2")
    if self.weighted.ndim != 5 or self.weighted.shape[-2:] != (2, self.n_members + 1):
      raise ValueError(f"weighted must be [T, batch, channels, 2, {self.n_members + 1}], got {self.weighted.shape}")
    if self.counts.shape != self.weighted.shape:
      raise ValueError(f"counts must be {self.weighted.shape}, got {self.counts.shape}")
    if len(self.directions) != self.weighted.shape[0] or any(d == 0 for d in self.directions):
      raise ValueError(f"directions must be {self.weighted.shape[0]} non-zero signs")
    if not (self.scale > 0.0 and math.isfinite(self.scale)):
      raise ValueError("scale must be positive and finite")
    self.invalid = (np.zeros(self.weighted.shape[0], np.uint64) if invalid is None
                    else np.asarray(invalid, dtype=np.uint64).reshape(self.weighted.shape[0]))

  @classmethod
  def merge(cls, parts):
    """The tables add; `fractions` merge with them (`FractionsScores.merge`), and every part carries them or none does."""
    parts = list(parts)
    total = super().merge(parts)
    carrying = [p.fractions for p in parts if p.fractions is not None]
    if carrying:
      if len(carrying) != len(parts):
        raise ValueError("merge: only some of the event scores carry fractions scores")
      total.fractions = FractionsScores.merge(carrying)
    return total

  # -- the table in float64 (exact: see quantize_node_weights) -------------------------------------------------
  @property
  def _n(self) -> np.ndarray:
    return (self.weighted[..., 0, :] + self.weighted[..., 1, :]).astype(np.float64) / self.scale

  @property
  def _o(self) -> np.ndarray:
    return self.weighted[..., 1, :].astype(np.float64) / self.scale

  @property
  def _p(self) -> np.ndarray:
    return np.arange(self.n_members + 1, dtype=np.float64) / float(self.n_members)

  @staticmethod
  def _ratio(a, b) -> np.ndarray:
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    out = np.full(a.shape, np.nan)
    np.divide(a, b, out=out, where=b != 0.0)
    return out

  @property
  def valid_weight(self) -> np.ndarray:
    """N: the node weight of the points that counted."""
    return self._n.sum(axis=-1)

  @property
  def valid_points(self) -> np.ndarray:
    return self.counts.sum(axis=(-1, -2))

  @property
  def base_rate(self) -> np.ndarray:
    return self._ratio(self._o.sum(axis=-1), self._n.sum(axis=-1))

  @property
  def brier(self) -> np.ndarray:
    n, o, p = self._n, self._o, self._p
    return self._ratio(((n - o) * p ** 2 + o * (1.0 - p) ** 2).sum(axis=-1), n.sum(axis=-1))

  @property
  def brier_fair(self) -> np.ndarray:
    """Ferro's fair Brier score: unbiased for the score of the distribution the members were drawn from."""
    m = float(self.n_members)
    k = np.arange(self.n_members + 1, dtype=np.float64)
    n = self._n
    return self.brier - self._ratio((n * (k * (m - k) / (m * m * (m - 1.0)))).sum(axis=-1), n.sum(axis=-1))

  @property
  def reliability(self) -> np.ndarray:
    n, o, p = self._n, self._o, self._p
    obar = np.where(n > 0.0, self._ratio(o, n), 0.0)
    return self._ratio((n * (p - obar) ** 2).sum(axis=-1), n.sum(axis=-1))    # (an empty bin has n = 0: it adds 0)

  @property
  def resolution(self) -> np.ndarray:
    n, o = self._n, self._o
    s = self.base_rate[..., None]
    obar = np.where(n > 0.0, self._ratio(o, n), 0.0)
    return self._ratio(np.where(n > 0.0, n * (obar - s) ** 2, 0.0).sum(axis=-1), n.sum(axis=-1))

  @property
  def uncertainty(self) -> np.ndarray:
    s = self.base_rate
    return s * (1.0 - s)

  @property
  def brier_skill(self) -> np.ndarray:
    return 1.0 - self._ratio(self.brier, self.uncertainty)

  @property
  def reliability_curve(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(p_k [M + 1], observed frequency o_k / n_k [T, B, c_out, M + 1] (NaN for an empty bin), n_k (same shape))."""
    return self._p, self._ratio(self._o, self._n), self._n

  def _hits_and_false_alarms(self) -> Tuple[np.ndarray, np.ndarray]:
    """H_j, F_j for the decision levels j = 0 .. M + 1 ("warn when k >= j"): [T, B, c_out, M + 2]."""
    n, o = self._n, self._o
    zero = np.zeros(n.shape[:-1] + (1,))
    tail = lambda a: np.concatenate([np.cumsum(a[..., ::-1], axis=-1)[..., ::-1], zero], axis=-1)
    return tail(o), tail(n - o)

  @property
  def hit_rate(self) -> np.ndarray:
    h, _ = self._hits_and_false_alarms()
    return self._ratio(h, self._o.sum(axis=-1)[..., None])

  @property
  def false_alarm_rate(self) -> np.ndarray:
    _, f = self._hits_and_false_alarms()
    return self._ratio(f, (self._n.sum(axis=-1) - self._o.sum(axis=-1))[..., None])

  @property
  def roc_area(self) -> np.ndarray:
    """The trapezoid rule through the M + 2 points (false_alarm_rate_j, hit_rate_j)."""
    h, f = self.hit_rate, self.false_alarm_rate
    return (0.5 * (f[..., :-1] - f[..., 1:]) * (h[..., :-1] + h[..., 1:])).sum(axis=-1)

  def economic_value(self, alpha) -> np.ndarray:
    """The relative economic value at cost/loss ratios `alpha` in (0, 1): [T, B, c_out] + alpha.shape.  Per decision
    level E_j = alpha (H_j + F_j) / N + (O - H_j) / N; value = max_j (E_clim - E_j) / (E_clim - E_perf) with
    E_clim = min(alpha, s), E_perf = alpha s."""
    alpha = np.asarray(alpha, dtype=np.float64)
    if np.any(alpha <= 0.0) or np.any(alpha >= 1.0):
      raise ValueError("alpha must lie in (0, 1)")
    h, f = self._hits_and_false_alarms()
    big_n, big_o = self._n.sum(axis=-1), self._o.sum(axis=-1)
    extra = (None,) * alpha.ndim
    lev = lambda a: a[(Ellipsis,) + extra]                 # [T, B, c_out, M + 2] -> [..., M + 2, alpha...]
    col = lambda a: a[(Ellipsis, None) + extra]            # [T, B, c_out]        -> [..., 1, alpha...]
    e = self._ratio(alpha * lev(h + f), col(big_n)) + self._ratio(col(big_o) - lev(h), col(big_n))
    s = col(self.base_rate)
    e_clim, e_perf = np.minimum(alpha, s), alpha * s
    value = self._ratio(e_clim - e, e_clim - e_perf)
    return np.max(value, axis=3)                           # (the denominators do not depend on j: NaN at all levels or none)


class FractionsScores(AdditiveScores):
  """The raw sums of `gc_ens_fss_score`: `sums` [T, S, B, c_out, 4] float64 -- over the counted centres, with P the
  neighbourhood ensemble probability, O the observed fraction of the neighbourhood and w the quantised node weight,
  sum w (P - O)^2, sum w (P^2 + O^2), sum w P, sum w O -- and `weight` [T, B, c_out] uint64, the valid weight of the event
  table (quantised, the same at every scale), with the member count M, the directions [T], the radii `scales_km` [S] and the
  `scale` of the quantised node weights.  The sums are additive: the FSS over several dates is 1 - sum S0 / sum S1, never a
  mean of scores.  Every score is [T, S, B, c_out] float64; a ratio whose denominator is zero is NaN, not an error."""
  _adds = ("sums", "weight")
  _same = {"n_members": "members", "directions": "directions", "scales_km": "scales", "scale": "scale"}
  _listed = ("fss", "fbs", "fss_uniform", "forecast_fraction", "observed_fraction", "frequency_bias")
  _channel_axis = 3
  _what = "fractions scores"

  def __init__(self, sums, weight, n_members: int, directions: Sequence[int], scales_km: Sequence[float], scale: float):
    self.sums = np.asarray(sums, dtype=np.float64)
    self.weight = np.asarray(weight, dtype=np.uint64)
    self.n_members = int(n_members)
    self.directions = tuple(int(np.sign(d)) for d in directions)
    self.scales_km = tuple(float(r) for r in scales_km)
    self.scale = float(scale)
    if self.n_members < 2:
      raise ValueError("n_members must be >= 2")
    if self.sums.ndim != 5 or self.sums.shape[-1] != 4:
      raise ValueError(f"sums must be [T, S, batch, channels, 4], got {self.sums.shape}")
    if self.weight.shape != self.sums.shape[:1] + self.sums.shape[2:4]:
      raise ValueError(f"weight must be {self.sums.shape[:1] + self.sums.shape[2:4]}, got {self.weight.shape}")
    if len(self.directions) != self.sums.shape[0] or any(d == 0 for d in self.directions):
      raise ValueError(f"directions must be {self.sums.shape[0]} non-zero signs")
    if len(self.scales_km) != self.sums.shape[1]:
      raise ValueError(f"scales_km must hold {self.sums.shape[1]} radii")
    if not (self.scale > 0.0 and math.isfinite(self.scale)):
      raise ValueError("scale must be positive and finite")

  @property
  def _w(self) -> np.ndarray:
    """W [T, 1, B, c_out]: the valid weight in the units of the sums (the quantised weights as they are)."""
    return self.weight.astype(np.float64)[:, None]

  @property
  def valid_weight(self) -> np.ndarray:
    """[T, B, c_out]: the node weight of the points that counted, as `EventScores.valid_weight`."""
    return self.weight.astype(np.float64) / self.scale

  @property
  def fss(self) -> np.ndarray:
    return 1.0 - EventScores._ratio(self.sums[..., 0], self.sums[..., 1])

  @property
  def fbs(self) -> np.ndarray:
    """The fractions Brier score: the weighted mean of (P - O)^2."""
    return EventScores._ratio(self.sums[..., 0], self._w)

  @property
  def forecast_fraction(self) -> np.ndarray:
    return EventScores._ratio(self.sums[..., 2], self._w)

  @property
  def observed_fraction(self) -> np.ndarray:
    return EventScores._ratio(self.sums[..., 3], self._w)

  @property
  def fss_uniform(self) -> np.ndarray:
    """0.5 + f0 / 2: the FSS of a uniform forecast of the observed fraction, the usual bar for "skilful"."""
    return 0.5 + self.observed_fraction / 2.0

  @property
  def frequency_bias(self) -> np.ndarray:
    return EventScores._ratio(self.sums[..., 2], self.sums[..., 3])

  @property
  def skilful_scale_km(self) -> np.ndarray:
    """[T, B, c_out]: the smallest of `scales_km` at which fss >= fss_uniform, NaN if none."""
    with np.errstate(invalid="ignore"):
      ok = self.fss >= self.fss_uniform                    # (NaN compares False)
    radii = np.asarray(self.scales_km, np.float64)[None, :, None, None]
    return np.where(ok.any(axis=1), np.min(np.where(ok, radii, np.inf), axis=1), np.nan)


class TailScores(AdditiveScores):
  """The raw sums of `gc_ens_tail_score`: `sums` [T, B, c_out, 4] float64 -- S0 = sum w, S1 = sum w ae, S2 = sum w d,
  S3 = sum w o over the counted nodes, with ae the mean absolute difference between the clamped members and the clamped
  truth, d the mean absolute difference between two clamped members (the Gini mean difference) and o whether the truth lies
  in the event -- `counts` [T, B, c_out] uint64 (counted points) and `invalid` [T] points skipped, with the member count M
  and the directions [T] (> 0: the upper tail, weight 1{z >= threshold}; < 0: the lower tail).  The sums are additive.
  Every score is [T, B, c_out] float64; where nothing counted (S0 = 0: a NaN threshold) it is NaN, not an error."""
  _adds = ("sums", "counts", "invalid")
  _same = {"n_members": "members", "directions": "directions"}
  _listed = ("twcrps", "twcrps_ensemble", "abs_error", "pair_distance", "base_rate", "valid_weight", "valid_points")
  _channel_axis = 2

  def __init__(self, sums, counts, n_members: int, directions: Sequence[int], invalid=None):
    self.sums = np.asarray(sums, dtype=np.float64)
    self.counts = np.asarray(counts, dtype=np.uint64)
    self.n_members = int(n_members)
    self.directions = tuple(int(np.sign(d)) for d in directions)
    if self.n_members < 2:
      raise ValueError("n_members must be >= 2")
    if self.sums.ndim != 4 or self.sums.shape[-1] != 4:
      raise ValueError(f"sums must be [T, batch, channels, 4], got {self.sums.shape}")
    if self.counts.shape != self.sums.shape[:3]:
      raise ValueError(f"counts must be {self.sums.shape[:3]}, got {self.counts.shape}")
    if len(self.directions) != self.sums.shape[0] or any(d == 0 for d in self.directions):
      raise ValueError(f"directions must be {self.sums.shape[0]} non-zero signs")
    self.invalid = (np.zeros(self.sums.shape[0], np.uint64) if invalid is None
                    else np.asarray(invalid, dtype=np.uint64).reshape(self.sums.shape[0]))

  def _over_weight(self, a) -> np.ndarray:
    out = np.full(self.sums.shape[:3], np.nan)
    np.divide(a, self.sums[..., 0], out=out, where=self.sums[..., 0] != 0.0)
    return out

  @property
  def valid_weight(self) -> np.ndarray:
    """S0: the node weight of the points that counted."""
    return self.sums[..., 0]

  @property
  def valid_points(self) -> np.ndarray:
    return self.counts

  @property
  def abs_error(self) -> np.ndarray:
    """S1 / S0: the mean absolute difference between a clamped member and the clamped truth."""
    return self._over_weight(self.sums[..., 1])

  @property
  def pair_distance(self) -> np.ndarray:
    """S2 / S0: the mean absolute difference between two clamped members."""
    return self._over_weight(self.sums[..., 2])

  @property
  def twcrps(self) -> np.ndarray:
    """The fair threshold-weighted CRPS: unbiased for that of the distribution the members were drawn from."""
    return self._over_weight(self.sums[..., 1] - 0.5 * self.sums[..., 2])

  @property
  def twcrps_ensemble(self) -> np.ndarray:
    """The threshold-weighted CRPS of the M-member empirical distribution (pair term normalised by M^2)."""
    m = float(self.n_members)
    return self._over_weight(self.sums[..., 1] - 0.5 * (m - 1.0) / m * self.sums[..., 2])

  @property
  def base_rate(self) -> np.ndarray:
    """S3 / S0: how often the truth lay in the event."""
    return self._over_weight(self.sums[..., 3])

  def scaled(self, channel_scale) -> "TailScores":
    """The scores of a x + b in place of x (members, truth and thresholds alike), a = channel_scale [c_out] > 0, any b: S1
    and S2 scale with a; weights, base rates and counts do not change.  a <= 0 is a ValueError: a negative scale swaps the
    tails."""
    a = np.asarray(channel_scale, dtype=np.float64).reshape(-1)
    if a.shape != (self.sums.shape[2],):
      raise ValueError(f"channel_scale must have shape ({self.sums.shape[2]},)")
    if not np.all(np.isfinite(a) & (a > 0.0)):
      raise ValueError("channel_scale must be finite and > 0 (a negative scale swaps the tails)")
    f = np.stack([np.ones_like(a), a, a, np.ones_like(a)], axis=-1)
    return TailScores(self.sums * f[None, None], self.counts, self.n_members, self.directions, self.invalid)


# ---------------------------------------------------------------------------------------------
# regions: the ensemble scores per set of grid nodes, every region from one pass (gc_ens_region_*)
# ---------------------------------------------------------------------------------------------
class RegionSpec:
  """Named regions of the grid: an ordered {name: mask}, at most 32.  A mask is boolean, [lat, lon] or [G] with
  node = lat_i * n_lon + lon_j; regions may overlap, and a node in no mask is never read by the device.  `masks` exposes the
  plain arrays, so a caller can combine them with a land-sea mask before building another spec."""

  MAX_REGIONS = 32

  def __init__(self, regions: Mapping[str, np.ndarray]):
    self.masks: Dict[str, np.ndarray] = {}
    for name, mask in regions.items():
      m = np.asarray(mask)
      if m.dtype != np.bool_ or m.ndim not in (1, 2):
        raise ValueError(f"region {name!r}: a mask is a boolean [lat, lon] or [G] array, got {m.dtype} {m.shape}")
      self.masks[name] = m
    if not 1 <= len(self.masks) <= self.MAX_REGIONS:
      raise ValueError(f"a RegionSpec holds 1..{self.MAX_REGIONS} regions, got {len(self.masks)}")
    if len({m.size for m in self.masks.values()}) != 1:
      raise ValueError("the masks cover grids of different sizes")

  @property
  def names(self) -> Tuple[str, ...]:
    return tuple(self.masks)

  @property
  def n_regions(self) -> int:
    return len(self.masks)

  @classmethod
  def from_bounds(cls, template, bounds: Mapping[str, Mapping[str, Tuple[float, float]]]) -> "RegionSpec":
    """Latitude-longitude boxes on the template's own `lat` / `lon` coordinates: {name: dict(lat=(lat0, lat1), lon=(lon0,
    lon1))}, either key optional (absent: all of them).  Bounds are inclusive.  Longitudes are taken modulo 360; a box
    wraps through 0 degrees when lon0 > lon1 after that (`lon=(-12.5, 42.5)` is 347.5 .. 360 and 0 .. 42.5); a span of 360
    degrees or more is the whole circle."""
    coords = datasets.as_dataset(template).coords
    if "lat" not in coords or "lon" not in coords:
      raise ValueError("template must have 'lat' and 'lon' coordinates")
    lat = np.asarray(coords["lat"], dtype=np.float64)
    lon = np.mod(np.asarray(coords["lon"], dtype=np.float64), 360.0)
    masks = {}
    for name, box in bounds.items():
      if set(box) - {"lat", "lon"}:
        raise ValueError(f"region {name!r}: bounds are given by 'lat' and 'lon', got {sorted(box)}")
      in_lat = np.ones(lat.shape, bool)
      if box.get("lat") is not None:
        lat0, lat1 = (float(v) for v in box["lat"])
        if lat0 > lat1:
          raise ValueError(f"region {name!r}: lat bounds must be ascending, got {(lat0, lat1)}")
        in_lat = (lat >= lat0) & (lat <= lat1)
      in_lon = np.ones(lon.shape, bool)
      if box.get("lon") is not None:
        lon0, lon1 = (float(v) for v in box["lon"])
        if lon1 - lon0 < 360.0:
          lon0, lon1 = lon0 % 360.0, lon1 % 360.0
          in_lon = (lon >= lon0) & (lon <= lon1) if lon0 <= lon1 else (lon >= lon0) | (lon <= lon1)
      masks[name] = in_lat[:, None] & in_lon[None, :]
    return cls(masks)

  def node_bits(self, template) -> np.ndarray:
    """[G] uint32 for `NativeDenoiser.ens_region_set`: bit r set = the node belongs to the r-th region.  The masks must fit
    the template's grid."""
    sizes = datasets.as_dataset(template).sizes
    if "lat" not in sizes or "lon" not in sizes:
      raise ValueError("template must have 'lat' and 'lon' dimensions")
    n_lat, n_lon = int(sizes["lat"]), int(sizes["lon"])
    bits = np.zeros(n_lat * n_lon, np.uint32)
    for r, (name, m) in enumerate(self.masks.items()):
      if m.shape not in ((n_lat, n_lon), (n_lat * n_lon,)):
        raise ValueError(f"region {name!r}: mask {m.shape} does not fit the {n_lat} x {n_lon} grid")
      bits |= m.reshape(-1).astype(np.uint32) << np.uint32(r)
    return bits


class RegionScores:
  """The results of `gc_ens_region_score`: per region r the raw sums [R, B, c_out, 6] float64, rank histogram [R, B, c_out,
  M + 1] uint64 and skipped points `invalid` [R] of `EnsembleScores`, restricted to the region's nodes.  `scores[name]` is the
  region's `EnsembleScores` (`.crps`, `.rmse`, `.spread_skill_ratio`, `.rank_histogram`, ...: no formula of its own); a region
  in which nothing counted has NaN scores."""

  def __init__(self, names: Sequence[str], sums, hist, n_members: int, invalid=None):
    self.names = tuple(names)
    self.sums = np.asarray(sums, dtype=np.float64)
    self.rank_histogram = np.asarray(hist, dtype=np.uint64)
    self.n_members = int(n_members)
    R = len(self.names)
    if len(set(self.names)) != R:
      raise ValueError("region names must be distinct")
    if self.sums.ndim != 4 or self.sums.shape[0] != R or self.sums.shape[-1] != 6:
      raise ValueError(f"sums must be [{R}, batch, channels, 6], got {self.sums.shape}")
    if self.rank_histogram.shape != self.sums.shape[:3] + (self.n_members + 1,):
      raise ValueError(f"hist must be {self.sums.shape[:3] + (self.n_members + 1,)}, got {self.rank_histogram.shape}")
    self.invalid = np.zeros(R, np.uint64) if invalid is None else np.asarray(invalid, dtype=np.uint64).reshape(R)

  def __getitem__(self, name: str) -> EnsembleScores:
    r = self.names.index(name) if name in self.names else None
    if r is None:
      raise KeyError(name)
    return EnsembleScores(self.sums[r], self.rank_histogram[r], self.n_members)

  def __len__(self) -> int:
    return len(self.names)

  def __iter__(self):
    return iter(self.names)

  def items(self):
    return [(name, self[name]) for name in self.names]

  def scaled(self, channel_scale) -> "RegionScores":
    """`EnsembleScores.scaled` of every region."""
    parts = [self[name].scaled(channel_scale) for name in self.names]
    return RegionScores(self.names, np.stack([p.sums for p in parts]), np.stack([p.rank_histogram for p in parts]),
                        self.n_members, self.invalid)

  @staticmethod
  def merge(parts: Sequence["RegionScores"]) -> "RegionScores":
    """Scores over the union of what the parts covered (other dates): raw sums and counts add, region by region."""
    parts = list(parts)
    if not parts:
      raise ValueError("merge: nothing to merge")
    first = parts[0]
    for p in parts[1:]:
      if p.names != first.names or p.n_members != first.n_members or p.sums.shape != first.sums.shape:
        raise ValueError("merge: the parts differ in region names, members or shape")
    sums, hist, invalid = first.sums.copy(), first.rank_histogram.copy(), first.invalid.copy()
    for p in parts[1:]:
      sums += p.sums
      hist += p.rank_histogram
      invalid += p.invalid
    return RegionScores(first.names, sums, hist, first.n_members, invalid)

  def per_variable(self, template) -> Dict[str, Dict[str, Dict[str, np.ndarray]]]:
    """{region: `EnsembleScores.per_variable(template)`}."""
    return {name: self[name].per_variable(template) for name in self.names}


# ---------------------------------------------------------------------------------------------
# derived and pooled fields: wind speed, neighbourhood maxima, area means (gc_ens_derive_*)
# ---------------------------------------------------------------------------------------------
_KM_PER_DEGREE = 111.195                                   # one degree of a great circle on the mean Earth radius 6371 km
_POOLS = {None: 0, "none": 0, "max": 1, "min": 2, "mean": 3}
_DERIVE_OPS = {"copy": 0, "norm2": 1, "sum": 2, "norm": 3, "vorticity": 4, "divergence": 5}


class DerivedSpec:
  """What `gc_ens_derive` makes of a member store (DESIGN.md sections 8g and 8p): an ordered list of derived variables, then
  one spatial pooling for all of them.

  `outputs`: `("copy", name)` keeps a target variable; `("norm2", new_name, name_a, name_b)` is sqrt(a^2 + b^2) of two
  target variables IN PHYSICAL UNITS, channel by channel (10 m wind speed from the two 10 m components: one channel; wind
  speed on 13 levels from the two components on levels: 13) -- `name_a` and `name_b` must have equal channel counts.

  Across levels, in physical units (section 8p): `("sum", new_name, terms)` is sum_t coef_t a_t [b_t] and `("norm", new_name,
  terms_1, terms_2)` the norm of two such sums.  A term is `(coef, (variable, level))` or `(coef, (variable, level), (variable,
  level))`, the level by INDEX as in `FeatureSpec`, None only for a variable of one channel; at most 64 terms in a list.  The
  result is one channel with the dims of the first source without `level`.  `select`, `thickness`, `shear`,
  `column_integral` and `ivt` build such tuples.  Along the grid: `("vorticity", new_name, u, v[, level])` and `("divergence",
  ...)` by centred differences on the sphere -- without a level channel by channel like norm2, with one a single channel
  without the `level` dim.  They need an equiangular grid of at least 3 longitudes round the whole circle.

  The derived channels are packed like every Dataset here, in sorted-name order (`datasets.channel_layout(self.template(...))`).
  `pool`: None, "max", "min" or "mean" over a window of `r_lat` rows either side (clipped at the poles) and `r_lon[i']`
  longitudes either side in row i' (wrapping) -- given as they are, or as `radius_km` (`window`).  The mean is weighted with
  `losses.normalized_latitude_weights`."""

  MAX_LIST_TERMS, MAX_PLAN_TERMS = 64, 1024              # the caps of gc_ens_derive_set_expr
  EARTH_RADIUS_M = 6371000.0

  def __init__(self, outputs, pool: Optional[str] = None, radius_km: Optional[float] = None, r_lat: Optional[int] = None,
               r_lon: Optional[Sequence[int]] = None):
    self.outputs = [tuple(o) for o in outputs]
    if not self.outputs:
      raise ValueError("outputs must name at least one derived variable")
    names = []
    for k, o in enumerate(self.outputs):
      if len(o) == 2 and o[0] == "copy":
        pass
      elif len(o) == 4 and o[0] == "norm2":
        pass
      elif len(o) == 3 and o[0] == "sum":
        self.outputs[k] = o[:2] + (self._terms(o[1], o[2]),)
      elif len(o) == 4 and o[0] == "norm":
        self.outputs[k] = o[:2] + (self._terms(o[1], o[2]), self._terms(o[1], o[3]))
      elif len(o) in (4, 5) and o[0] in ("vorticity", "divergence"):
        if len(o) == 5 and o[4] is not None and (isinstance(o[4], bool) or int(o[4]) != o[4]):
          raise ValueError(f"{o[1]!r}: the level must be an index or None, got {o[4]!r}")
      else:
        raise ValueError("an output must be ('copy', name), ('norm2', new_name, name_a, name_b), ('sum', new_name, terms), "
                         "('norm', new_name, terms_1, terms_2) or ('vorticity' | 'divergence', new_name, u_name, v_name[, level]), "
                         f"got {o!r}")
      names.append(o[1])
    if len(set(names)) != len(names):
      raise ValueError(f"derived variable names must be distinct, got {names}")
    if pool not in _POOLS:
      raise ValueError(f"pool must be None, 'max', 'min' or 'mean', got {pool!r}")
    self.pool = None if pool in (None, "none") else pool
    explicit = r_lat is not None or r_lon is not None
    if self.pool is None:
      if radius_km is not None or explicit:
        raise ValueError("a window (radius_km, or r_lat and r_lon) needs a pool")
    else:
      if (radius_km is not None) == explicit:
        raise ValueError("a pool needs either radius_km or r_lat and r_lon")
      if explicit and (r_lat is None or r_lon is None):
        raise ValueError("r_lat and r_lon must be given together")
      if radius_km is not None and not (float(radius_km) >= 0.0 and math.isfinite(float(radius_km))):
        raise ValueError("radius_km must be finite and >= 0")
      if explicit and int(r_lat) < 0:
        raise ValueError("r_lat must be >= 0")
    self.radius_km = None if radius_km is None else float(radius_km)
    self.r_lat = None if r_lat is None else int(r_lat)
    self.r_lon = None if r_lon is None else np.asarray(r_lon, dtype=np.int64).reshape(-1)

  @classmethod
  def _terms(cls, name, terms):
    """One term list, checked and normalised to ((coef, (variable, level), (variable, level) or None), ...)."""
    try:
      terms = [tuple(t) for t in terms]
    except TypeError:
      raise ValueError(f"{name!r}: a term list is a sequence of (coef, (variable, level)[, (variable, level)])") from None
    if not 1 <= len(terms) <= cls.MAX_LIST_TERMS:
      raise ValueError(f"{name!r}: a term list has 1 .. {cls.MAX_LIST_TERMS} terms, got {len(terms)}")
    out = []
    for t in terms:
      if len(t) not in (2, 3):
        raise ValueError(f"{name!r}: a term is (coef, (variable, level)) or (coef, (variable, level), (variable, level)), got {t!r}")
      if isinstance(t[0], (str, bytes)) or not math.isfinite(float(t[0])):
        raise ValueError(f"{name!r}: the coefficient of {t!r} is not a finite number")
      factors = []
      for f in t[1:]:
        if isinstance(f, str) or len(tuple(f)) != 2 or not isinstance(f[0], str) or \
           not (f[1] is None or (not isinstance(f[1], bool) and int(f[1]) == f[1])):
          raise ValueError(f"{name!r}: a factor is (variable, level index or None), got {f!r}")
        factors.append((f[0], None if f[1] is None else int(f[1])))
      out.append((float(t[0]), factors[0], factors[1] if len(factors) == 2 else None))
    return tuple(out)

  # ---- helpers that only build output tuples --------------------------------------------------------------------------
  @staticmethod
  def select(name, var, level):
    """One level of a multi-level variable as a variable of its own, in physical units."""
    return ("sum", name, [(1.0, (var, level))])

  @staticmethod
  def thickness(name, var, upper, lower, g: float = 9.80665):
    """(var[upper] - var[lower]) / g: the thickness in metres of the layer between two levels of the geopotential."""
    return ("sum", name, [(1.0 / g, (var, upper)), (-1.0 / g, (var, lower))])

  @staticmethod
  def shear(name, u, v, upper, lower):
    """|(u, v)[upper] - (u, v)[lower]|: the vertical wind shear between two levels."""
    return ("norm", name, [(1.0, (u, upper)), (-1.0, (u, lower))], [(1.0, (v, upper)), (-1.0, (v, lower))])

  @staticmethod
  def pressure_weights(levels_hPa, g: float = 9.80665) -> np.ndarray:
    """The trapezoid weights dp / g of a column integral, dp in Pa: half the distance between the neighbouring levels, half
    intervals at the two ends.  Either order of the levels."""
    p = 100.0 * np.asarray(levels_hPa, np.float64).reshape(-1)
    if p.size < 2 or not np.isfinite(p).all() or np.any(np.diff(p) == 0) or np.any(np.sign(np.diff(p)) != np.sign(p[1] - p[0])):
      raise ValueError("levels_hPa must be at least two finite pressures in ascending or descending order")
    d = np.abs(np.diff(p))
    return np.concatenate([[d[0]], d[:-1] + d[1:], [d[-1]]]) / (2.0 * g)

  @staticmethod
  def column_integral(name, var, levels_hPa):
    """(1 / g) int var dp over all levels of `var` (total column water vapour from the specific humidity)."""
    return ("sum", name, [(float(w), (var, k)) for k, w in enumerate(DerivedSpec.pressure_weights(levels_hPa))])

  @staticmethod
  def ivt(name, q, u, v, levels_hPa):
    """|(1 / g) int q (u, v) dp|: the integrated vapour transport."""
    w = DerivedSpec.pressure_weights(levels_hPa)
    return ("norm", name, [(float(x), (q, k), (u, k)) for k, x in enumerate(w)], [(float(x), (q, k), (v, k)) for k, x in enumerate(w)])

  @property
  def names(self) -> List[str]:
    return [o[1] for o in self.outputs]

  @property
  def legacy(self) -> bool:
    """Only copy / norm2 outputs: the plan of gc_ens_derive_set."""
    return all(o[0] in ("copy", "norm2") for o in self.outputs)

  @staticmethod
  def _channel(where, who, var, level) -> int:
    """The source channel of (variable, level index or None) in the packed order `where`."""
    if var not in where:
      raise ValueError(f"{var!r} is not a target variable")
    off, n = where[var]
    if level is None:
      if n != 1:
        raise ValueError(f"{who!r}: {var!r} has {n} levels: name one (level index)")
      return off
    if not 0 <= level < n:
      raise ValueError(f"{who!r}: level {level!r} of {var!r} outside 0 .. {n - 1}")
    return off + level

  def _sources(self, template0):
    """{derived name: (op, [(offset, n) of each source] | the term lists with channels | (u, v) first channels, count)},
    with the variables, levels and channel counts checked."""
    template0 = datasets.as_dataset(template0)
    where = {name: (off, n) for name, off, n in datasets.channel_layout(template0)}
    out = {}
    for o in self.outputs:
      if o[0] in ("sum", "norm"):
        out[o[1]] = (o[0], [[(c, self._channel(where, o[1], *fa), -1 if fb is None else self._channel(where, o[1], *fb))
                             for c, fa, fb in terms] for terms in o[2:]])
        continue
      srcs = o[1:] if o[0] == "copy" else o[2:4]
      for s in srcs:
        if s not in where:
          raise ValueError(f"{s!r} is not a target variable")
      if o[0] in ("vorticity", "divergence") and len(o) == 5 and o[4] is not None:
        out[o[1]] = (o[0], [(self._channel(where, o[1], s, int(o[4])), 1) for s in srcs])
        continue
      if o[0] != "copy" and where[srcs[0]][1] != where[srcs[1]][1]:
        raise ValueError(f"{srcs[0]!r} has {where[srcs[0]][1]} channels, {srcs[1]!r} {where[srcs[1]][1]}: the "
                         f"{'norm' if o[0] == 'norm2' else o[0]} is taken channel by channel")
      out[o[1]] = (o[0], [where[s] for s in srcs])
    return out

  def template(self, template0) -> datasets.Dataset:
    """A Dataset of the derived variables (zeros) with the dims of their (first) source variable -- without `level` where the
    output is one channel formed across or at a level -- and the source's coordinates: `EventSpec.packed`,
    `EnsembleScores.per_variable` and `EventScores.per_variable` work on it unchanged."""
    template0 = datasets.as_dataset(template0)
    self._sources(template0)
    out = {}
    for o in self.outputs:
      flat = o[0] in ("sum", "norm") or (o[0] in ("vorticity", "divergence") and len(o) == 5 and o[4] is not None)
      src = template0[o[1] if o[0] == "copy" else o[2][0][1][0] if o[0] in ("sum", "norm") else o[2]]
      data = np.asarray(src.data)
      if flat and "level" in src.dims:
        data = np.take(data, 0, axis=src.dims.index("level"))
        out[o[1]] = datasets.Variable(tuple(d for d in src.dims if d != "level"), np.zeros_like(data))
      else:
        out[o[1]] = datasets.Variable(src.dims, np.zeros_like(data))
    return datasets.Dataset(out, template0.coords)

  def _per_channel(self, template0):
    """[(op, channel of source a, channel of source b, term lists or None)] per derived channel, in the packed order of
    `template`."""
    srcs = self._sources(template0)
    rows = []
    for name, _, n in datasets.channel_layout(self.template(template0)):
      op, where = srcs[name]
      if op in ("sum", "norm"):
        if n != 1:
          raise ValueError(f"{name!r}: its first source has dims beyond 'level': a {op} is one channel")
        rows.append((op, 0, 0, where))
        continue
      for k in range(n):
        rows.append((op, where[0][0] + k, where[-1][0] + k, None))
    return rows

  @staticmethod
  def window(lat, lon, radius_km: float) -> Tuple[int, np.ndarray]:
    """(r_lat, r_lon [n_lat]) of a great-circle radius on an equiangular grid: r_lat = rint(radius / (111.195 dlat)),
    r_lon[i] = min((n_lon - 1) // 2, floor(radius / (111.195 dlon cos lat_i))); the pole rows take the cap (the whole row)."""
    lat, lon = np.asarray(lat, np.float64).reshape(-1), np.asarray(lon, np.float64).reshape(-1)
    if lat.size < 2 or lon.size < 2:
      raise ValueError("window needs at least two latitudes and two longitudes")
    dlat, dlon = abs(float(lat[1] - lat[0])), abs(float(lon[1] - lon[0]))
    cap = (lon.size - 1) // 2
    coslat = np.cos(np.deg2rad(lat))
    r_lon = np.full(lat.size, cap, np.int64)
    inside = np.abs(lat) < 90.0 - 1e-9
    with np.errstate(divide="ignore", over="ignore"):
      r_lon[inside] = np.minimum(float(cap), np.floor(float(radius_km) / (_KM_PER_DEGREE * dlon * coslat[inside]))).astype(np.int64)
    return int(np.rint(float(radius_km) / (_KM_PER_DEGREE * dlat))), r_lon.astype(np.int32)

  def plan(self, template0, scale=None, loc=None) -> Dict[str, object]:
    """The keyword arguments of `NativeDenoiser.ens_derive_set`.  `scale`, `loc` [c_src]: the members hold (x - loc) / scale
    per source channel (None: 1 and 0), so a norm2 channel gets (sa, la, sb, lb) = the sources' scale and location and
    comes out in physical units."""
    template0 = datasets.as_dataset(template0)
    c_src = sum(n for _, _, n in datasets.channel_layout(template0))
    scale = np.ones(c_src) if scale is None else np.asarray(scale, np.float64).reshape(-1)
    loc = np.zeros(c_src) if loc is None else np.asarray(loc, np.float64).reshape(-1)
    if scale.shape != (c_src,) or loc.shape != (c_src,):
      raise ValueError(f"scale and loc must have shape ({c_src},)")
    rows = self._per_channel(template0)
    op = np.array([_DERIVE_OPS[r[0]] for r in rows], np.int32)
    src_a = np.array([r[1] for r in rows], np.int32)
    src_b = np.array([r[2] for r in rows], np.int32)
    affine = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (len(rows), 1))
    for j, r in enumerate(rows):
      if r[0] == "norm2":
        affine[j] = (scale[r[1]], loc[r[1]], scale[r[2]], loc[r[2]])
    sizes = template0.sizes
    if "lat" not in sizes or "lon" not in sizes:
      raise ValueError("template must have 'lat' and 'lon' dimensions")
    n_lat, n_lon = int(sizes["lat"]), int(sizes["lon"])
    out = dict(c_src=c_src, op=op, src_a=src_a, src_b=src_b, affine=affine, pool=_POOLS[self.pool], n_lat=n_lat, n_lon=n_lon,
               r_lat=0, r_lon=None, row_weight=None)
    if not self.legacy:
      out.update(self._expr_tables(template0, rows, scale, loc))
    if self.pool is not None:
      if self.radius_km is not None:
        r_lat, r_lon = self.window(template0.coords["lat"], template0.coords["lon"], self.radius_km)
      else:
        r_lat, r_lon = self.r_lat, self.r_lon
      r_lon = np.asarray(r_lon, np.int64)
      if r_lon.shape != (n_lat,):
        raise ValueError(f"r_lon must have one entry per latitude row ({n_lat}), got {r_lon.shape}")
      if np.any((r_lon < 0) | (r_lon > (n_lon - 1) // 2)):
        raise ValueError(f"r_lon must lie in 0 .. {(n_lon - 1) // 2}")
      out.update(r_lat=int(r_lat), r_lon=r_lon.astype(np.int32),
                 row_weight=np.asarray(losses.normalized_latitude_weights(template0), np.float64))
    return out

  def _expr_tables(self, template0, rows, scale, loc) -> Dict[str, object]:
    """The further keywords of a plan with a sum, norm, vorticity or divergence channel (gc_ens_derive_set_expr): the
    statistics, the term table, and for the last two ops the row tables of the grid."""
    starts, coef, ta, tb = np.zeros((len(rows), 3), np.int32), [], [], []
    for j, r in enumerate(rows):
      if r[3] is not None:
        starts[j, 0] = len(coef)
        for k, terms in enumerate(r[3]):
          coef += [t[0] for t in terms]
          ta += [t[1] for t in terms]
          tb += [t[2] for t in terms]
          starts[j, k + 1:] = len(coef)
    if len(coef) > self.MAX_PLAN_TERMS:
      raise ValueError(f"the plan has {len(coef)} terms: at most {self.MAX_PLAN_TERMS}")
    out = dict(scale=scale.copy(), loc=loc.copy(), term_start=starts, term_coef=np.asarray(coef, np.float64),
               term_a=np.asarray(ta, np.int32), term_b=np.asarray(tb, np.int32), coslat=None, inv_rcos=None, inv_dphi=None,
               inv_2dlam=None, pole_row=None)
    if not any(r[0] in ("vorticity", "divergence") for r in rows):
      return out
    if "lat" not in template0.coords or "lon" not in template0.coords:
      raise ValueError("vorticity and divergence need the template's 'lat' and 'lon' coordinates")
    lat, lon = (np.asarray(template0.coords[k], np.float64).reshape(-1) for k in ("lat", "lon"))
    if lon.size < 3:
      raise ValueError(f"vorticity and divergence need at least 3 longitudes, got {lon.size}")
    if lat.size < 2:
      raise ValueError(f"vorticity and divergence need at least 2 latitudes, got {lat.size}")
    dlat, dlon = np.diff(lat), np.diff(lon)
    if dlat[0] == 0 or not np.allclose(dlat, dlat[0], rtol=1e-6, atol=0.0):
      raise ValueError("vorticity and divergence need equally spaced latitudes (the centred difference is second order only there)")
    if dlon[0] == 0 or not np.allclose(dlon, dlon[0], rtol=1e-6, atol=0.0) or not np.isclose(abs(dlon[0]) * lon.size, 360.0, rtol=1e-6):
      raise ValueError("vorticity and divergence need equally spaced longitudes round the whole circle")
    pole = np.abs(lat) >= 90.0 - 1e-9
    if pole[1:-1].any() or (pole[0] and pole[1]) or (pole[-1] and pole[-2]):
      raise ValueError("only an end row of the grid can be a pole row, next to a row that is none")
    phi = np.deg2rad(lat)
    cos = np.where(pole, 0.0, np.cos(phi))
    idx = np.arange(lat.size)
    with np.errstate(divide="ignore"):
      inv_rcos = np.where(pole, 0.0, 1.0 / (self.EARTH_RADIUS_M * np.where(pole, 1.0, cos)))
    out.update(coslat=cos, inv_rcos=inv_rcos, inv_dphi=1.0 / (phi[np.minimum(idx + 1, lat.size - 1)] - phi[np.maximum(idx - 1, 0)]),
               inv_2dlam=float(1.0 / (2.0 * np.deg2rad(dlon[0]))), pole_row=pole.astype(np.int32))
    return out

  def channel_stats(self, template0, scale=None, loc=None) -> Tuple[np.ndarray, np.ndarray]:
    """(scale_d, loc_d) [c_d]: a copy channel keeps its source's, every other channel is in physical units already: (1, 0)."""
    template0 = datasets.as_dataset(template0)
    c_src = sum(n for _, _, n in datasets.channel_layout(template0))
    scale = np.ones(c_src) if scale is None else np.asarray(scale, np.float64).reshape(-1)
    loc = np.zeros(c_src) if loc is None else np.asarray(loc, np.float64).reshape(-1)
    if scale.shape != (c_src,) or loc.shape != (c_src,):
      raise ValueError(f"scale and loc must have shape ({c_src},)")
    rows = self._per_channel(template0)
    return (np.array([scale[r[1]] if r[0] == "copy" else 1.0 for r in rows]),
            np.array([loc[r[1]] if r[0] == "copy" else 0.0 for r in rows]))


# ---------------------------------------------------------------------------------------------
# spectral band views: the members and the truth, scale by scale (gc_ens_band_*)
# ---------------------------------------------------------------------------------------------
class BandSpec:
  """What `gc_ens_band` makes of a member store: every chosen target variable low-, band- or
  high-pass filtered per total wavenumber l of the spherical harmonics -- the route analysis -> response -> synthesis of
  `spectra.SphericalAnalysis` -- as a derived variable `f"{variable}_{band}"` with the dims of the variable.  Every scorer
  then works on the band-limited fields unchanged.

  `bands`: {name: (l_lo, l_hi)} with inclusive bounds, `l_hi` None: up to lmax - 1; or {name: dict(l=(l_lo, l_hi),
  complement=True)}: the field MINUS that band, f - synth(w a), which also keeps what the basis below lmax cannot
  represent (a grid field is not band-limited: this is the true high-pass); or {name: response}, an array [lmax] of finite
  weights (or dict(response=..., complement=...)).  1 to 8 bands.  `variables`: the target variables to filter (None: all).
  `lmax`: the band limit (None: n_lon / 2).  `taper`: the half-width in wavenumbers of a raised-cosine edge around
  l_lo - 1/2 and l_hi + 1/2 (0: sharp; no edge below l = 0 or above lmax - 1); two bands that meet at an edge still sum
  to one there.

  The filter is linear and Y_00 lies in the band with weight w[0]: a view of `x s + l` is `s view(x) + l w[0]`, with
  `complement` `s view(x) + l (1 - w[0])` -- `channel_stats` returns the source scale and that location, and no affine
  goes to the device.  With float32 tables a constant comes back within a few 1e-7 relative."""

  MAX_BANDS = 8
  EARTH_RADIUS_KM = 6371.0

  def __init__(self, bands, variables: Optional[Sequence[str]] = None, lmax: Optional[int] = None, taper: float = 0):
    if not isinstance(bands, Mapping) or not 1 <= len(bands) <= self.MAX_BANDS:
      raise ValueError(f"bands must be a mapping of 1 .. {self.MAX_BANDS} named bands")
    if lmax is not None and (isinstance(lmax, bool) or int(lmax) != lmax or int(lmax) < 1):
      raise ValueError(f"lmax must be a positive integer or None, got {lmax!r}")
    if not (math.isfinite(float(taper)) and float(taper) >= 0.0):
      raise ValueError(f"taper must be finite and >= 0, got {taper!r}")
    self.lmax = None if lmax is None else int(lmax)
    self.taper = float(taper)
    self.bands = {}                                        # name -> ("l", lo, hi or None, complement) | ("w", response, complement)
    for name, b in bands.items():
      if not isinstance(name, str) or not name:
        raise ValueError(f"a band name must be a non-empty string, got {name!r}")
      complement = False
      if isinstance(b, Mapping):
        extra = set(b) - {"l", "response", "complement"}
        if extra or ("l" in b) == ("response" in b):
          raise ValueError(f"band {name!r}: a dict takes either l=(lo, hi) or response=, and complement=; got {sorted(b)}")
        complement = bool(b.get("complement", False))
        b = b["l"] if "l" in b else np.asarray(b["response"], np.float64)
      if isinstance(b, np.ndarray) or (isinstance(b, (list, tuple)) and len(b) != 2):
        w = np.asarray(b, np.float64).reshape(-1)
        if w.size < 1 or not np.isfinite(w).all():
          raise ValueError(f"band {name!r}: a response is a non-empty array of finite weights")
        if self.lmax is not None and w.size != self.lmax:
          raise ValueError(f"band {name!r}: the response has {w.size} weights, lmax is {self.lmax}")
        self.bands[name] = ("w", w.copy(), complement)
        continue
      try:
        lo, hi = b
      except (TypeError, ValueError):
        raise ValueError(f"band {name!r}: a band is (l_lo, l_hi), a dict or a response array, got {b!r}") from None
      for v in (lo, hi):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
          raise ValueError(f"band {name!r}: the bounds are wavenumbers (integers; l_hi may be None), got {b!r}")
      if lo is None or int(lo) < 0 or (hi is not None and int(hi) < int(lo)):
        raise ValueError(f"band {name!r}: 0 <= l_lo <= l_hi, got {b!r}")
      if self.lmax is not None and (int(lo) >= self.lmax or (hi is not None and int(hi) >= self.lmax)):
        raise ValueError(f"band {name!r}: the bounds {b!r} lie beyond lmax - 1 = {self.lmax - 1}")
      self.bands[name] = ("l", int(lo), None if hi is None else int(hi), complement)
    self.variables = None if variables is None else [str(v) for v in variables]
    if self.variables is not None and (not self.variables or len(set(self.variables)) != len(self.variables)):
      raise ValueError(f"variables must be distinct names, at least one, got {variables!r}")

  @classmethod
  def from_wavelengths_km(cls, bands, variables=None, lmax=None, taper=0) -> "BandSpec":
    """`bands`: {name: (longest_km, shortest_km)} (or dict(km=(longest, shortest), complement=...)); a wavelength maps to
    l = round(2 pi R / wavelength) with R = 6371 km; `longest_km` None: from l = 0, `shortest_km` None: up to lmax - 1."""
    def wavenumber(km):
      if km is None:
        return None
      if not (math.isfinite(float(km)) and float(km) > 0.0):
        raise ValueError(f"a wavelength must be finite and > 0 km, got {km!r}")
      return int(round(2.0 * math.pi * cls.EARTH_RADIUS_KM / float(km)))
    out = {}
    for name, b in bands.items():
      complement = None
      if isinstance(b, Mapping):
        if set(b) - {"km", "complement"} or "km" not in b:
          raise ValueError(f"band {name!r}: a dict takes km=(longest, shortest) and complement=, got {sorted(b)}")
        complement, b = bool(b.get("complement", False)), b["km"]
      longest, shortest = b
      l = (wavenumber(longest) or 0, wavenumber(shortest))
      out[name] = l if complement is None else dict(l=l, complement=complement)
    return cls(out, variables, lmax, taper)

  @property
  def band_names(self) -> List[str]:
    return list(self.bands)

  @property
  def names(self) -> List[str]:
    """The derived variables, `f"{variable}_{band}"`, where `variables` were named; else the band names alone (the
    variables are then those of the template: `template(template0)` has the full list)."""
    if self.variables is None:
      return self.band_names
    return [f"{v}_{b}" for v in self.variables for b in self.bands]

  def _lmax(self, template0) -> int:
    n_lon = int(datasets.as_dataset(template0).sizes["lon"])
    lmax = max(1, n_lon // 2) if self.lmax is None else self.lmax
    if not 1 <= lmax <= n_lon // 2:
      raise ValueError(f"lmax must be in 1 .. n_lon / 2 = {n_lon // 2}, got {lmax}")
    return lmax

  @staticmethod
  def _edge(l, at, taper, rising):
    """A raised-cosine step around `at` (between two wavenumbers) of half-width `taper`: 0 -> 1 when `rising`."""
    if taper <= 0.0:
      r = (l > at).astype(np.float64)
    else:
      r = 0.5 * (1.0 - np.cos(np.pi * np.clip((l - (at - taper)) / (2.0 * taper), 0.0, 1.0)))
    return r if rising else 1.0 - r

  def responses(self, lmax: int) -> Tuple[np.ndarray, np.ndarray]:
    """(response [K, lmax] float64, complement [K] int32), the bands in the order given."""
    l = np.arange(lmax, dtype=np.float64)
    w = np.ones((len(self.bands), lmax))
    comp = np.zeros(len(self.bands), np.int32)
    for k, (name, b) in enumerate(self.bands.items()):
      comp[k] = int(b[-1])
      if b[0] == "w":
        if b[1].size != lmax:
          raise ValueError(f"band {name!r}: the response has {b[1].size} weights, lmax is {lmax}")
        w[k] = b[1]
        continue
      lo, hi = b[1], lmax - 1 if b[2] is None else b[2]
      if lo >= lmax or hi >= lmax:
        raise ValueError(f"band {name!r}: the bounds ({b[1]}, {b[2]}) lie beyond lmax - 1 = {lmax - 1}")
      if lo > 0:
        w[k] *= self._edge(l, lo - 0.5, self.taper, True)
      if hi < lmax - 1:
        w[k] *= self._edge(l, hi + 0.5, self.taper, False)
    return w, comp

  def _rows(self, template0):
    """[(derived name, variable, band index, (offset, n) of the variable)] in the order given: variables, then bands."""
    template0 = datasets.as_dataset(template0)
    where = {name: (off, n) for name, off, n in datasets.channel_layout(template0)}
    variables = list(where) if self.variables is None else self.variables
    for v in variables:
      if v not in where:
        raise ValueError(f"{v!r} is not a target variable")
    rows = [(f"{v}_{b}", v, k, where[v]) for v in variables for k, b in enumerate(self.bands)]
    names = [r[0] for r in rows]
    if len(set(names)) != len(names):
      raise ValueError(f"the derived variable names are not distinct: {sorted(n for n in set(names) if names.count(n) > 1)}")
    return rows

  def template(self, template0) -> datasets.Dataset:
    """A Dataset of the derived variables `f"{variable}_{band}"` (zeros) with the dims and coordinates of the variable."""
    template0 = datasets.as_dataset(template0)
    out = {}
    for name, v, _, _ in self._rows(template0):
      out[name] = datasets.Variable(template0[v].dims, np.zeros_like(np.asarray(template0[v].data)))
    return datasets.Dataset(out, template0.coords)

  def _per_channel(self, template0):
    """(src_channel [c_d], band [c_d]) in the packed order of `template`."""
    rows = {r[0]: r for r in self._rows(template0)}
    src, band = [], []
    for name, _, n in datasets.channel_layout(self.template(template0)):
      _, _, k, (off, n_src) = rows[name]
      assert n == n_src
      src += [off + c for c in range(n)]
      band += [k] * n
    return np.asarray(src, np.int32), np.asarray(band, np.int32)

  def plan(self, template0, scale=None, loc=None) -> Dict[str, object]:
    """The keyword arguments of `NativeDenoiser.ens_band_set`, the synthesis tables of the template's grid among them.
    `scale` and `loc` are taken for the interface of `DerivedSpec.plan` and not used: the filter is linear, the members stay
    in their own units (`channel_stats`)."""
    from . import spectra                                 # (spectra imports this module)
    template0 = datasets.as_dataset(template0)
    c_src = sum(n for _, _, n in datasets.channel_layout(template0))
    lmax = self._lmax(template0)
    response, complement = self.responses(lmax)
    src, band = self._per_channel(template0)
    leg, cos_s, sin_s = spectra.SphericalAnalysis.for_template(template0, lmax).synthesis_tables()
    return dict(c_src=c_src, response=response, complement=complement, src_channel=src, band=band, legendre_synthesis=leg,
                cos_s=cos_s, sin_s=sin_s)

  def channel_stats(self, template0, scale=None, loc=None) -> Tuple[np.ndarray, np.ndarray]:
    """(scale_d, loc_d) [c_d]: the source channel's scale, and its location times w[0] (times 1 - w[0] with complement)."""
    template0 = datasets.as_dataset(template0)
    c_src = sum(n for _, _, n in datasets.channel_layout(template0))
    scale = np.ones(c_src) if scale is None else np.asarray(scale, np.float64).reshape(-1)
    loc = np.zeros(c_src) if loc is None else np.asarray(loc, np.float64).reshape(-1)
    if scale.shape != (c_src,) or loc.shape != (c_src,):
      raise ValueError(f"scale and loc must have shape ({c_src},)")
    response, complement = self.responses(self._lmax(template0))
    src, band = self._per_channel(template0)
    w0 = np.where(complement[band] != 0, 1.0 - response[band, 0], response[band, 0])
    return scale[src].copy(), loc[src] * w0


# ---------------------------------------------------------------------------------------------
# feature detection: cyclone centres, strike fields, tracks (gc_ens_feature_*)
# ---------------------------------------------------------------------------------------------
_EARTH_RADIUS_KM = 6371.0
_FEATURE_KEYS = ("variable", "level", "kind", "radius_km", "threshold", "ring_km", "depth", "strike_km")


class FeaturePlan(dict):
  """The keyword arguments of `NativeDenoiser.ens_feature_set` (a dict), and beside them what turns a list of centres into
  physical units: `names` [D] (the detectors in channel order), `lat`, `lon` (the grid's coordinates) and `scale`, `loc` [D]
  (a listed value x is `x * scale + loc` in physical units)."""
  names: Tuple[str, ...] = ()
  lat = lon = scale = loc = None


class FeatureSpec:
  """What `gc_ens_feature` looks for in a member store: named detectors, each a local extremum of one
  channel with a depth test, whose centres come back as lists and as 0 / 1 strike fields -- one derived variable per
  detector, named like it, which every scorer reads as it is (its ensemble mean is the strike probability).

  `detectors`: {name: dict(variable=, level=None, kind="min" | "max", radius_km=, threshold=None, ring_km=None, depth=None,
  strike_km=)}, 1 to 8 of them.  `variable`: a target variable; `level`: the index of its level (None: a surface variable).
  `radius_km`: the centre is the extremum of the window of that great-circle radius (`DerivedSpec.window`); `ring_km`,
  `depth`: the smallest value on the boundary of the window of radius `ring_km` lies at least `depth` above the centre (for
  a maximum: below) -- a closed low; `threshold`: the centre's value is at most (for a maximum: at least) this;
  `strike_km`: a node is struck by a centre within this radius.  Every radius is a number of km, or the window itself as
  (r_lat, r_lon) with r_lon one integer or one per latitude row.  Thresholds and depths are in physical units.
  `max_centres` (1..1024): the entries a list keeps; the count and the strike field see all centres.
  `scales_km`: the neighbourhood radii of `event_spec()` (None: none) -- the fractions skill score of the strikes."""

  def __init__(self, detectors: Mapping[str, Mapping[str, object]], max_centres: int = 64,
               scales_km: Optional[Sequence[float]] = None):
    self.detectors = {str(k): dict(v) for k, v in detectors.items()}
    self.scales_km = EventSpec({}, [1], scales_km).scales_km   # (validated as an EventSpec's)
    if not 1 <= len(self.detectors) <= 8:
      raise ValueError(f"a FeatureSpec holds 1 to 8 detectors, got {len(self.detectors)}")
    if isinstance(max_centres, bool) or int(max_centres) != max_centres or not 1 <= int(max_centres) <= 1024:
      raise ValueError(f"max_centres must be an integer in 1 .. 1024, got {max_centres!r}")
    self.max_centres = int(max_centres)
    for name, det in self.detectors.items():
      unknown = set(det) - set(_FEATURE_KEYS)
      if unknown:
        raise ValueError(f"detector {name!r}: unknown keys {sorted(unknown)} (known: {list(_FEATURE_KEYS)})")
      if "variable" not in det:
        raise ValueError(f"detector {name!r} names no variable")
      det.setdefault("kind", "min")
      if det["kind"] not in ("min", "max"):
        raise ValueError(f"detector {name!r}: kind must be 'min' or 'max', got {det['kind']!r}")
      for key in ("radius_km", "strike_km"):
        if det.get(key) is None:
          raise ValueError(f"detector {name!r} needs {key}")
      for key in ("radius_km", "strike_km", "ring_km"):
        r = det.get(key)
        if r is not None and not isinstance(r, (tuple, list)) and not (math.isfinite(float(r)) and float(r) >= 0.0):
          raise ValueError(f"detector {name!r}: {key} must be finite and >= 0")
        if isinstance(r, (tuple, list)) and (len(r) != 2 or int(r[0]) < 0):
          raise ValueError(f"detector {name!r}: {key} as a window is (r_lat >= 0, r_lon)")
      if det.get("depth") is not None and det.get("ring_km") is None:
        raise ValueError(f"detector {name!r}: a depth needs ring_km")
      if det.get("ring_km") is not None and det.get("depth") is None:
        raise ValueError(f"detector {name!r}: ring_km needs a depth")
      for key in ("threshold", "depth"):
        if det.get(key) is not None and not math.isfinite(float(det[key])):
          raise ValueError(f"detector {name!r}: {key} must be finite")
      ring, radius = det.get("ring_km"), det["radius_km"]
      if ring is not None and not isinstance(ring, (tuple, list)) and not isinstance(radius, (tuple, list)) and float(ring) <= float(radius):
        raise ValueError(f"detector {name!r}: the ring ({ring} km) must be larger than the extremum radius ({radius} km)")

  @property
  def names(self) -> List[str]:
    """The detectors in the channel order of the strike store: sorted, as every Dataset here is packed."""
    return sorted(self.detectors)

  def _channel(self, template0, name: str) -> int:
    """The source channel of detector `name` in the packed order of `template0`."""
    det = self.detectors[name]
    where = {v: (off, n) for v, off, n in datasets.channel_layout(template0)}
    if det["variable"] not in where:
      raise ValueError(f"detector {name!r}: {det['variable']!r} is not a target variable")
    off, n = where[det["variable"]]
    level = det.get("level")
    if level is None:
      if n != 1:
        raise ValueError(f"detector {name!r}: {det['variable']!r} has {n} levels: name one (level=index)")
      return off
    if isinstance(level, bool) or int(level) != level or not 0 <= int(level) < n:
      raise ValueError(f"detector {name!r}: level {level!r} outside 0 .. {n - 1}")
    return off + int(level)

  def template(self, template0) -> datasets.Dataset:
    """A Dataset with one variable per detector (zeros), with the dims of a surface variable -- the source's without its
    level -- and the source's coordinates: `EventSpec.packed` and every `per_variable` work on it unchanged."""
    template0 = datasets.as_dataset(template0)
    out = {}
    for name in self.names:
      self._channel(template0, name)
      src = template0[self.detectors[name]["variable"]]
      data = np.asarray(src.data)
      if "level" in src.dims:
        data = np.take(data, 0, axis=src.dims.index("level"))
      out[name] = datasets.Variable(tuple(d for d in src.dims if d != "level"), np.zeros_like(data))
    return datasets.Dataset(out, template0.coords)

  @staticmethod
  def _window(given, lat, lon) -> Tuple[int, np.ndarray]:
    if not isinstance(given, (tuple, list)):
      return DerivedSpec.window(lat, lon, float(given))
    r_lon = np.asarray(given[1], dtype=np.int64)
    r_lon = np.full(len(lat), int(r_lon), np.int64) if r_lon.ndim == 0 else r_lon.reshape(-1)
    if r_lon.shape != (len(lat),):
      raise ValueError(f"r_lon must be one integer or one per latitude row ({len(lat)}), got {r_lon.shape}")
    if np.any((r_lon < 0) | (r_lon > (len(lon) - 1) // 2)):
      raise ValueError(f"r_lon must lie in 0 .. {(len(lon) - 1) // 2}")
    return int(given[0]), r_lon.astype(np.int32)

  def plan(self, template0, scale=None, loc=None) -> FeaturePlan:
    """The keyword arguments of `NativeDenoiser.ens_feature_set`, as a `FeaturePlan`.  `scale`, `loc` [c_src]: the members
    hold (x - loc) / scale per source channel (None: 1 and 0); a threshold t becomes (t - loc) / scale and a depth
    depth / scale of the detector's channel (scale > 0: a minimum stays a minimum)."""
    template0 = datasets.as_dataset(template0)
    c_src = sum(n for _, _, n in datasets.channel_layout(template0))
    scale = np.ones(c_src) if scale is None else np.asarray(scale, np.float64).reshape(-1)
    loc = np.zeros(c_src) if loc is None else np.asarray(loc, np.float64).reshape(-1)
    if scale.shape != (c_src,) or loc.shape != (c_src,):
      raise ValueError(f"scale and loc must have shape ({c_src},)")
    if not np.all(scale > 0.0):
      raise ValueError("scale must be positive")
    sizes = template0.sizes
    if "lat" not in sizes or "lon" not in sizes:
      raise ValueError("template must have 'lat' and 'lon' dimensions")
    lat, lon = np.asarray(template0.coords["lat"], np.float64), np.asarray(template0.coords["lon"], np.float64)
    n_lat, n_lon = int(sizes["lat"]), int(sizes["lon"])
    names = self.names
    D = len(names)
    zeros = np.zeros(n_lat, np.int32)
    out = FeaturePlan(c_src=c_src, channel=np.zeros(D, np.int32), direction=np.zeros(D, np.int32),
                      use_threshold=np.zeros(D, np.int32), threshold=np.zeros(D, np.float32), n_lat=n_lat, n_lon=n_lon,
                      r_lat=np.zeros(D, np.int32), r_lon=np.zeros((D, n_lat), np.int32), ring_lat=np.zeros(D, np.int32),
                      ring_lon=np.zeros((D, n_lat), np.int32), depth=np.zeros(D, np.float64), strike_lat=np.zeros(D, np.int32),
                      strike_lon=np.zeros((D, n_lat), np.int32), max_centres=self.max_centres)
    for d, name in enumerate(names):
      det = self.detectors[name]
      ch = self._channel(template0, name)
      out["channel"][d] = ch
      out["direction"][d] = -1 if det["kind"] == "min" else 1
      if det.get("threshold") is not None:
        out["use_threshold"][d] = 1
        out["threshold"][d] = np.float32((float(det["threshold"]) - loc[ch]) / scale[ch])
      out["r_lat"][d], out["r_lon"][d] = self._window(det["radius_km"], lat, lon)
      out["strike_lat"][d], out["strike_lon"][d] = self._window(det["strike_km"], lat, lon)
      if det.get("ring_km") is not None:
        ring_lat, ring_lon = self._window(det["ring_km"], lat, lon)
        if ring_lat <= int(out["r_lat"][d]):
          raise ValueError(f"detector {name!r}: the ring (r_lat {ring_lat}) is not larger than the extremum radius "
                           f"(r_lat {int(out['r_lat'][d])}) on this grid")
        out["ring_lat"][d], out["ring_lon"][d] = ring_lat, ring_lon
        out["depth"][d] = float(det["depth"]) / scale[ch]
      else:
        out["ring_lon"][d] = zeros
    out.names, out.lat, out.lon = tuple(names), lat, lon
    out.scale, out.loc = scale[out["channel"]], loc[out["channel"]]
    return out

  def channel_stats(self, template0=None, scale=None, loc=None) -> Tuple[np.ndarray, np.ndarray]:
    """(scale_d, loc_d) [D]: a strike field is 0 / 1 whatever the units of its source: (1, 0)."""
    del template0, scale, loc
    return np.ones(len(self.detectors)), np.zeros(len(self.detectors))

  def event_spec(self) -> "EventSpec":
    """The one event of every strike field, `value > 0.5`: the Brier score, reliability curve, ROC area and economic value
    of the strike probability."""
    return EventSpec({name: np.array([0.5]) for name in self.names}, [1], self.scales_km)


def unpack_centres(count, node, value, plan=None) -> Dict[str, list]:
  """The arrays of `NativeDenoiser.ens_feature_centres` as {detector: [B][M + 1] entries}, field M the truth; an entry is
  dict(count=the true number, node=, lat=, lon=, value=) over the listed centres, ascending in node.  With a `FeaturePlan`
  lat, lon and value are physical (degrees; `x * scale + loc`); with a plain plan they are the row, the column and the
  value in the members' units."""
  count, node, value = np.asarray(count), np.asarray(node), np.asarray(value)
  n_lon = int(plan["n_lon"]) if plan is not None else None
  names = getattr(plan, "names", None) or tuple(str(d) for d in range(count.shape[2]))
  physical = getattr(plan, "lat", None) is not None
  out = {}
  for d, name in enumerate(names):
    out[name] = []
    for b in range(count.shape[1]):
      row = []
      for z in range(count.shape[0]):
        k = min(int(count[z, b, d]), node.shape[-1])
        at, x = node[z, b, d, :k].astype(np.int64), value[z, b, d, :k]
        i, j = (at // n_lon, at % n_lon) if n_lon else (at, np.zeros_like(at))
        if physical:
          entry = dict(lat=plan.lat[i], lon=plan.lon[j], value=x.astype(np.float64) * plan.scale[d] + plan.loc[d])
        else:
          entry = dict(lat=i, lon=j, value=x.copy())
        row.append(dict(count=int(count[z, b, d]), node=at, **entry))
      out[name].append(row)
  return out


def great_circle_km(lat_a, lon_a, lat_b, lon_b) -> np.ndarray:
  """The great-circle distance (haversine, mean Earth radius 6371 km) between points in degrees; broadcasts."""
  pa, pb = np.deg2rad(np.asarray(lat_a, np.float64)), np.deg2rad(np.asarray(lat_b, np.float64))
  dl = np.deg2rad(np.asarray(lon_b, np.float64) - np.asarray(lon_a, np.float64))
  h = np.sin((pb - pa) / 2.0) ** 2 + np.cos(pa) * np.cos(pb) * np.sin(dl / 2.0) ** 2
  return 2.0 * _EARTH_RADIUS_KM * np.arcsin(np.sqrt(np.clip(h, 0.0, 1.0)))


def link_tracks(centres_per_lead, max_km: float) -> List[List[Tuple[int, float, float, float]]]:
  """Greedy linking of the centres of ONE member (or the truth) and ONE detector over lead times into tracks, on the host.
  `centres_per_lead[k]`: dict(lat=, lon=, value=[, node=]) of lead k (an entry of `unpack_centres`; without `node` the
  position in the list stands in).  Between every two consecutive leads all pairs within `max_km` great-circle distance
  are formed and taken in ascending distance -- ties by ascending node index of the earlier centre, then of the later --
  each centre being used at most once on either side.  -> the tracks, each a list of (lead, lat, lon, value), in the order
  of their first centre (lead, then node).  Pure NumPy, deterministic."""
  if not (float(max_km) >= 0.0 and math.isfinite(float(max_km))):
    raise ValueError("max_km must be finite and >= 0")
  leads = []
  for c in centres_per_lead:
    lat, lon = np.asarray(c["lat"], np.float64).reshape(-1), np.asarray(c["lon"], np.float64).reshape(-1)
    val = np.asarray(c["value"], np.float64).reshape(-1)
    node = np.asarray(c["node"], np.int64).reshape(-1) if c.get("node") is not None else np.arange(lat.size)
    if not lat.size == lon.size == val.size == node.size:
      raise ValueError("lat, lon, value and node of a lead must have equal lengths")
    leads.append((lat, lon, val, node))
  nxt = [np.full(l[0].size, -1, np.int64) for l in leads]          # per centre: its successor at the next lead
  has_prev = [np.zeros(l[0].size, bool) for l in leads]
  for k in range(len(leads) - 1):
    (la, lo, _, na), (lb, lob, _, nb) = leads[k], leads[k + 1]
    if la.size == 0 or lb.size == 0:
      continue
    dist = great_circle_km(la[:, None], lo[:, None], lb[None, :], lob[None, :])
    a, b = np.nonzero(dist <= float(max_km))
    for p in np.lexsort((nb[b], na[a], dist[a, b])):               # distance, then the earlier node, then the later
      if nxt[k][a[p]] < 0 and not has_prev[k + 1][b[p]]:
        nxt[k][a[p]] = b[p]
        has_prev[k + 1][b[p]] = True
  tracks = []
  for k, (lat, lon, val, node) in enumerate(leads):
    for c in np.argsort(node, kind="stable"):
      if has_prev[k][c]:
        continue
      track, kk, cc = [], k, int(c)
      while cc >= 0:
        track.append((kk, float(leads[kk][0][cc]), float(leads[kk][1][cc]), float(leads[kk][2][cc])))
        cc, kk = int(nxt[kk][cc]), kk + 1
      tracks.append(track)
  return tracks


class FeatureScores:
  """What `GenCast.ensemble_features` returns.  `centres`: {detector: [B][M] entries}, `truth_centres`: {detector: [B]
  entries}, an entry dict(count=, node=, lat=, lon=, value=) (`unpack_centres`); `strike_probability`: a Dataset with one
  variable per detector, the fraction of members that put a centre within the strike radius of a node (NaN where a source
  value is not finite); `scores`: the `EnsembleScores` of the strike store; `events`: its `EventScores` at threshold 0.5 --
  Brier score, reliability curve, ROC area and `economic_value` of the strike probability against where the truth had one;
  `template`: the Dataset of the detectors for `per_variable`."""

  def __init__(self, scores, events, centres=None, truth_centres=None, strike_probability=None, template=None):
    self.scores, self.events, self.template = scores, events, template
    self.centres, self.truth_centres, self.strike_probability = centres, truth_centres, strike_probability

  @classmethod
  def merge(cls, parts: Sequence["FeatureScores"]) -> "FeatureScores":
    """Over several dates: the raw sums and the tables add; centres and the probability map belong to one date."""
    parts = list(parts)
    return cls(EnsembleScores.merge([p.scores for p in parts]), EventScores.merge([p.events for p in parts]),
               template=parts[0].template)


def split_centres(unpacked: Dict[str, list]) -> Tuple[Dict[str, list], Dict[str, list]]:
  """{detector: [B][M + 1]} -> ({detector: [B][M]} of the members, {detector: [B]} of the truth)."""
  return ({k: [row[:-1] for row in v] for k, v in unpacked.items()}, {k: [row[-1] for row in v] for k, v in unpacked.items()})


# ---------------------------------------------------------------------------------------------
# time windows: accumulations, means, changes and extremes over lead times (gc_ens_window_*)
# ---------------------------------------------------------------------------------------------
_WINDOW_KINDS = {"sum": 0, "mean": 0, "change": 0, "linear": 0, "max": 1, "min": 2}


class WindowSpec:
  """What `gc_ens_window_emit` makes of the last `steps` lead times of a member store: per member,
  and for the truth, one field over time.

  `kind`: "sum" (an accumulation: 24 h precipitation from two 12 h steps), "mean", "max", "min", "change" (newest minus
  oldest; `steps` >= 2) or "linear" with `coef` [steps], oldest lead time first.  sum, mean and change are linear windows
  with coefficients 1, 1 / steps and (-1, 0, .., 0, +1).  `steps`: 1..64 lead times.  `stride`: lead times between the ends of
  two windows; `steps` (the default) gives windows that tile the rollout, 1 a window ending at every lead time from the
  first full one on.  `source`: None, the main store, or the name of an entry of `derived` ("the highest pooled wind speed
  within three days").  Variable names and the template are the source's.  A lead time at which any of the `steps` values
  is not finite gives NaN: an accumulation with a missing step is not an accumulation."""

  def __init__(self, kind: str, steps: int, stride: Optional[int] = None, source: Optional[str] = None, coef=None):
    if kind not in _WINDOW_KINDS:
      raise ValueError(f"kind must be one of {sorted(_WINDOW_KINDS)}, got {kind!r}")
    if isinstance(steps, bool) or int(steps) != steps or not 1 <= int(steps) <= 64:
      raise ValueError(f"steps must be an integer in 1 .. 64, got {steps!r}")
    self.kind, self.steps = kind, int(steps)
    if kind == "change" and self.steps < 2:
      raise ValueError("a change needs steps >= 2")
    if stride is not None and (isinstance(stride, bool) or int(stride) != stride or int(stride) < 1):
      raise ValueError(f"stride must be a positive integer, got {stride!r}")
    self.stride = self.steps if stride is None else int(stride)
    if source is not None and not isinstance(source, str):
      raise ValueError("source must be None (the main store) or the name of a derived entry")
    self.source = source
    if kind == "linear":
      if coef is None:
        raise ValueError("a linear window needs coef")
      c = np.asarray(coef, dtype=np.float64).reshape(-1)
      if c.shape != (self.steps,):
        raise ValueError(f"coef must have {self.steps} entries, got {c.shape[0]}")
      if not np.all(np.isfinite(c)):
        raise ValueError("coef must be finite")
      self.coef = c.copy()
    else:
      if coef is not None:
        raise ValueError("only kind 'linear' takes coef")
      self.coef = None

  def coefficients(self) -> Optional[np.ndarray]:
    """a [steps] float64, oldest lead time first, of a linear window; None for max and min."""
    L = self.steps
    if self.kind == "sum":
      return np.ones(L)
    if self.kind == "mean":
      return np.full(L, 1.0 / L)
    if self.kind == "change":
      a = np.zeros(L)
      a[0], a[-1] = -1.0, 1.0
      return a
    return None if self.coef is None else self.coef.copy()

  def plan(self) -> Dict[str, object]:
    """The keyword arguments of `NativeDenoiser.ens_window_set`."""
    return dict(kind=_WINDOW_KINDS[self.kind], length=self.steps, coef=self.coefficients())

  def leads(self, horizon: int) -> List[int]:
    """The lead times k < horizon that end a window: k + 1 >= steps and (k + 1 - steps) % stride == 0."""
    return [k for k in range(int(horizon)) if k + 1 >= self.steps and (k + 1 - self.steps) % self.stride == 0]

  def channel_stats(self, scale, loc) -> Tuple[np.ndarray, np.ndarray]:
    """(scale_w, loc_w): the affine map from a windowed value of members that hold (x - loc) / scale to physical units.  A
    linear window of x is scale * (the window of the members) + loc * sum(a): (scale, loc * sum(a)); the extreme of x is
    scale * (the extreme of the members) + loc: (scale, loc)."""
    scale, loc = np.asarray(scale, np.float64).reshape(-1), np.asarray(loc, np.float64).reshape(-1)
    if scale.shape != loc.shape:
      raise ValueError("scale and loc must have the same shape")
    a = self.coefficients()
    return scale.copy(), loc.copy() if a is None else loc * float(np.sum(a))


# ---------------------------------------------------------------------------------------------
# multivariate scores: energy over channel groups, variogram over grid offsets (gc_ens_energy_*, gc_ens_variogram_*)
# ---------------------------------------------------------------------------------------------
class EnergySpec:
  """Groups of target variables whose joint forecast the energy score judges: `groups` {group name: [variable, ..]}, 1 to
  32 of them, every variable in at most one group; a variable brings all its channels (levels).  `weights` {variable:
  a scalar or one value per channel of the variable}, finite and > 0 (default 1): the a[c] of the norm -- level or variable
  weights.  The score is formed in the units of the member store (normalised residuals under the usual wrappers), which is
  what makes a norm over several variables meaningful."""

  def __init__(self, groups: Mapping[str, Sequence[str]], weights: Optional[Mapping[str, object]] = None):
    self.groups = {str(k): tuple(str(v) for v in vs) for k, vs in groups.items()}
    self.weights = {str(k): np.asarray(v, dtype=np.float64) for k, v in (weights or {}).items()}
    if not 1 <= len(self.groups) <= 32:
      raise ValueError("an EnergySpec has 1 to 32 groups")
    seen = set()
    for g, vs in self.groups.items():
      if not vs:
        raise ValueError(f"group {g!r} is empty")
      for v in vs:
        if v in seen:
          raise ValueError(f"variable {v!r} is in more than one group")
        seen.add(v)
    for v, w in self.weights.items():
      if v not in seen:
        raise ValueError(f"a weight is given for {v!r}, which is in no group")
      if not np.all(np.isfinite(w) & (w > 0.0)):
        raise ValueError(f"weights[{v!r}] must be finite and > 0")

  @property
  def names(self) -> Tuple[str, ...]:
    return tuple(self.groups)

  def restricted(self, template) -> Optional["EnergySpec"]:
    """The spec of the groups whose variables are all variables of `template` (None: there is no such group)."""
    have = set(datasets.as_dataset(template).keys())
    groups = {g: vs for g, vs in self.groups.items() if set(vs) <= have}
    if not groups:
      return None
    used = {v for vs in groups.values() for v in vs}
    return EnergySpec(groups, {v: w for v, w in self.weights.items() if v in used})

  def plan(self, template) -> Dict[str, object]:
    """The arguments of `NativeDenoiser.ens_energy_set` in the channel order of `datasets.channel_layout(template)`, with
    the group `names`."""
    layout = {name: (off, n) for name, off, n in datasets.channel_layout(datasets.as_dataset(template))}
    C = sum(n for _, n in layout.values())
    group = np.full(C, -1, dtype=np.int32)
    scale = np.ones(C, dtype=np.float64)
    for k, vs in enumerate(self.groups.values()):
      for v in vs:
        if v not in layout:
          raise ValueError(f"{v!r} is not a target variable")
        off, n = layout[v]
        group[off:off + n] = k
        if v in self.weights:
          w = self.weights[v].reshape(-1)
          if w.shape[0] not in (1, n):
            raise ValueError(f"weights[{v!r}] must be a scalar or have {n} values, got {w.shape[0]}")
          scale[off:off + n] = w
    return {"n_groups": len(self.groups), "group": group, "scale": scale, "names": self.names}


class EnergyScores:
  """The energy score of F forecasts over K groups: `err` and `pair` [F, K] float64 with the member count M, where for one
  forecast, D[i][j] = sqrt(D2 / S0) the weighted root-mean-square distance between fields i and j (slot M: the truth),

    err = mean_i D[i][M]      pair = mean_{i<j<M} D[i][j]
    fair ES = err - pair / 2      ensemble ES = err - (M - 1) / M pair / 2

  -- the pairing of the fair and ensemble CRPS, to which both reduce for a group of one point.  ES is not additive in the
  raw sums, so the terms are kept per forecast (a batch member counts as a forecast); `merge` concatenates and the scores
  are means over forecasts.  A group without a valid point (S0 = 0) is NaN.  Units are the member store's own."""

  def __init__(self, err, pair, n_members: int, names: Optional[Sequence[str]] = None, invalid: int = 0):
    self.err = np.asarray(err, dtype=np.float64)
    self.pair = np.asarray(pair, dtype=np.float64)
    self.n_members = int(n_members)
    self.invalid = int(invalid)
    if self.n_members < 2:
      raise ValueError("n_members must be >= 2")
    if self.err.ndim != 2 or self.pair.shape != self.err.shape:
      raise ValueError(f"err and pair must be [forecasts, groups], got {self.err.shape} and {self.pair.shape}")
    self.names = tuple(f"group{k}" for k in range(self.err.shape[1])) if names is None else tuple(str(n) for n in names)
    if len(self.names) != self.err.shape[1]:
      raise ValueError(f"{len(self.names)} names for {self.err.shape[1]} groups")

  @staticmethod
  def pair_index(i: int, j: int) -> int:
    """The index of the pair i < j in the last axis of D2."""
    if not 0 <= i < j:
      raise ValueError("pair_index needs 0 <= i < j")
    return j * (j - 1) // 2 + i

  @classmethod
  def from_sums(cls, d2, s0, n_members: int, names: Optional[Sequence[str]] = None, invalid: int = 0) -> "EnergyScores":
    """From the raw sums of `gc_ens_energy_score`: `d2` [B, K, P], `s0` [B, K]."""
    M = int(n_members)
    d2, s0 = np.asarray(d2, dtype=np.float64), np.asarray(s0, dtype=np.float64)
    if d2.ndim != 3 or d2.shape[-1] != M * (M + 1) // 2 or s0.shape != d2.shape[:2]:
      raise ValueError(f"d2 must be [batch, groups, {M * (M + 1) // 2}] and s0 [batch, groups], got {d2.shape} and {s0.shape}")
    with np.errstate(invalid="ignore", divide="ignore"):
      D = np.sqrt(d2 / s0[..., None])
    truth = np.arange(M * (M - 1) // 2, M * (M + 1) // 2)        # the pairs (i, M)
    return cls(D[..., truth].mean(axis=-1), D[..., :truth[0]].mean(axis=-1), M, names, invalid)

  @property
  def n_forecasts(self) -> int:
    return self.err.shape[0]

  @property
  def per_forecast(self) -> np.ndarray:
    """[F, K]: the fair energy score of every forecast."""
    return self.err - 0.5 * self.pair

  @property
  def per_forecast_ensemble(self) -> np.ndarray:
    m = float(self.n_members)
    return self.err - 0.5 * (m - 1.0) / m * self.pair

  @property
  def energy_score(self) -> np.ndarray:
    """[K]: the fair energy score, the mean over the forecasts."""
    return self.per_forecast.mean(axis=0)

  @property
  def energy_score_ensemble(self) -> np.ndarray:
    """[K]: the energy score of the M-member empirical distribution."""
    return self.per_forecast_ensemble.mean(axis=0)

  @property
  def error_term(self) -> np.ndarray:
    return self.err.mean(axis=0)

  @property
  def pair_term(self) -> np.ndarray:
    return self.pair.mean(axis=0)

  @staticmethod
  def merge(parts: Sequence["EnergyScores"]) -> "EnergyScores":
    """The forecasts of all parts (other dates), one after the other."""
    parts = list(parts)
    if not parts:
      raise ValueError("merge: nothing to merge")
    first = parts[0]
    for p in parts[1:]:
      if p.n_members != first.n_members or p.names != first.names:
        raise ValueError("merge: the parts differ in members or groups")
    return EnergyScores(np.concatenate([p.err for p in parts]), np.concatenate([p.pair for p in parts]), first.n_members,
                        first.names, sum(p.invalid for p in parts))

  def per_group(self) -> Dict[str, Dict[str, float]]:
    """{score: {group name: value}}."""
    return {score: {n: float(v) for n, v in zip(self.names, getattr(self, score))}
            for score in ("energy_score", "energy_score_ensemble", "error_term", "pair_term")}


class VariogramSpec:
  """Pairs of grid points a fixed offset apart: `offsets` 1 to 16 pairs (di, dj) in rows and columns of the lat-lon grid,
  none (0, 0) -- the partner of (i, j) is (i + di, (j + dj) mod n_lon), and a pair whose partner row lies beyond a pole is
  left out -- and the order `p` in {0.5, 1, 2} of the variogram (0.5: Scheuerer and Hamill 2015)."""

  def __init__(self, offsets: Sequence[Tuple[int, int]], p: float = 0.5):
    o = np.asarray(offsets)
    if o.ndim != 2 or o.shape[1] != 2 or not 1 <= o.shape[0] <= 16 or not np.all(o == np.round(o)):
      raise ValueError("offsets must be 1 to 16 pairs of integers (di, dj)")
    self.offsets = tuple((int(a), int(b)) for a, b in o)
    if any(a == 0 and b == 0 for a, b in self.offsets):
      raise ValueError("the offset (0, 0) pairs a point with itself")
    self.p = float(p)
    if self.p not in (0.5, 1.0, 2.0):
      raise ValueError("p must be 0.5, 1 or 2")

  def plan(self, template) -> Dict[str, object]:
    """The arguments of `NativeDenoiser.ens_variogram_set` for the grid of `template`."""
    sizes = datasets.as_dataset(template).sizes
    if "lat" not in sizes or "lon" not in sizes:
      raise ValueError("template must have 'lat' and 'lon' dimensions")
    return self.grid_plan(int(sizes["lat"]), int(sizes["lon"]))

  def grid_plan(self, n_lat: int, n_lon: int) -> Dict[str, object]:
    for di, dj in self.offsets:
      if abs(di) >= n_lat or abs(dj) >= n_lon:
        raise ValueError(f"offset {(di, dj)} reaches beyond the {n_lat} x {n_lon} grid")
    return {"n_lat": int(n_lat), "n_lon": int(n_lon), "offsets": np.asarray(self.offsets, dtype=np.int32), "p": self.p}


class VariogramScores(AdditiveScores):
  """The raw sums of `gc_ens_variogram_score`: `sums` [4, B, c_out, O] float64 -- V0 = sum omega, V1 = sum omega (vy - vx)^2,
  V2 = sum omega vx, V3 = sum omega vy over the valid pairs, v(u) = |u_g - u_g'|^p, vx the members' mean of it, vy the
  truth's -- and `counts` [B, c_out, O] uint64 (valid pairs), with the member count, the offsets [O] and p.  The sums are
  additive.  Every score is [B, c_out, O]."""
  _adds = ("counts", "sums")                                # (the counts first: they have the shape of a score)
  _same = {"n_members": "members", "offsets": "offsets", "p": "order"}
  _listed = ("variogram_score", "ensemble_variogram", "truth_variogram", "roughness_ratio", "valid_weight", "valid_pairs")

  def __init__(self, sums, counts, n_members: int, offsets, p: float):
    self.sums = np.asarray(sums, dtype=np.float64)
    self.counts = np.asarray(counts, dtype=np.uint64)
    self.n_members = int(n_members)
    self.offsets = tuple((int(a), int(b)) for a, b in offsets)
    self.p = float(p)
    if self.sums.ndim != 4 or self.sums.shape[0] != 4 or self.sums.shape[-1] != len(self.offsets):
      raise ValueError(f"sums must be [4, batch, channels, {len(self.offsets)}], got {self.sums.shape}")
    if self.counts.shape != self.sums.shape[1:]:
      raise ValueError(f"counts must be {self.sums.shape[1:]}, got {self.counts.shape}")

  @property
  def valid_weight(self) -> np.ndarray:
    return self.sums[0]

  @property
  def valid_pairs(self) -> np.ndarray:
    return self.counts

  @property
  def variogram_score(self) -> np.ndarray:
    """V1 / V0: the weighted mean squared difference between the truth's variogram term and the ensemble's."""
    return self.sums[1] / self.sums[0]

  @property
  def ensemble_variogram(self) -> np.ndarray:
    return self.sums[2] / self.sums[0]

  @property
  def truth_variogram(self) -> np.ndarray:
    return self.sums[3] / self.sums[0]

  @property
  def roughness_ratio(self) -> np.ndarray:
    """V2 / V3: below 1 the members are smoother than the truth at that separation."""
    return self.sums[2] / self.sums[3]

  def scaled(self, channel_scale) -> "VariogramScores":
    """The scores of a x + b in place of x (members and truth alike), a = channel_scale [c_out], any b: V1 scales with
    |a|^(2p), V2 and V3 with |a|^p; weights and counts do not change."""
    a = np.asarray(channel_scale, dtype=np.float64).reshape(-1)
    if a.shape != (self.sums.shape[2],):
      raise ValueError(f"channel_scale must have shape ({self.sums.shape[2]},)")
    if np.any(a == 0.0) or not np.all(np.isfinite(a)):
      raise ValueError("channel_scale must be finite and non-zero")
    ap = np.abs(a) ** self.p
    f = np.stack([np.ones_like(a), ap * ap, ap, ap])[:, None, :, None]
    return VariogramScores(self.sums * f, self.counts, self.n_members, self.offsets, self.p)


# ---------------------------------------------------------------------------------------------
# extreme forecast index: the members ranked in the climatological samples (gc_ens_efi_*)
# ---------------------------------------------------------------------------------------------
def efi_table(n_climatology: int) -> np.ndarray:
  """a[n] = asin(2 n / K - 1) / pi for n = 0 .. K, float64 [K + 1]: the table `gc_ens_efi_score` looks up.  The upper half
  is formed with `np.arcsin` and mirrored, so a[K - n] == -a[n] to the bit, a[K / 2] == 0 for even K, a[0] = -0.5 and
  a[K] = 0.5 exactly: a member above every sample adds a[K] + a[K] = 1."""
  K = int(n_climatology)
  if not 2 <= K <= 64:
    raise ValueError(f"the number of climatological samples must be in 2..64, got {n_climatology}")
  a = np.zeros(K + 1, dtype=np.float64)
  upper = np.arange(K // 2 + 1, K + 1)
  a[upper] = np.arcsin((2.0 * upper - K) / K) / np.pi
  a[K - upper] = -a[upper]
  return a


class EfiSpec:
  """What `gc_ens_efi_score` verifies the index against: T (0..4) climatological events of the truth and E (2..32) equal EFI
  bins.  `quantiles` [T] in (0, 1) with `directions` [T]: +1 is "the truth lies above the q-quantile of the samples"
  (lt(y) >= ceil(q K - 1e-9)), -1 "below it" (le(y) <= floor(q K + 1e-9)); or `ranks` [T], the integers themselves, for every
  K.  No units: ranks are unchanged by any increasing map applied to members, samples and truth alike."""

  def __init__(self, quantiles: Optional[Sequence[float]] = (0.9, 0.1), directions: Sequence[int] = (+1, -1), bins: int = 20, *,
               ranks: Optional[Sequence[int]] = None):
    if ranks is not None:
      if any(isinstance(r, bool) or int(r) != r for r in ranks):
        raise ValueError("ranks must be integers")
      self.ranks, self.quantiles = tuple(int(r) for r in ranks), None
    else:
      self.ranks, self.quantiles = None, tuple(float(q) for q in quantiles)
      if not all(0.0 < q < 1.0 for q in self.quantiles):
        raise ValueError("quantiles must lie in (0, 1)")
    self.directions = tuple(int(np.sign(d)) for d in directions)
    T = len(self.ranks if self.quantiles is None else self.quantiles)
    if T > 4:
      raise ValueError(f"at most 4 events, got {T}")
    if len(self.directions) != T or any(d == 0 for d in self.directions):
      raise ValueError(f"directions must be {T} non-zero signs")
    if isinstance(bins, bool) or int(bins) != bins or not 2 <= int(bins) <= 32:
      raise ValueError(f"bins must be an integer in 2..32, got {bins!r}")
    self.bins = int(bins)

  @property
  def n_events(self) -> int:
    return len(self.directions)

  def ranks_for(self, n_climatology: int) -> Tuple[int, ...]:
    """The integer rank of every event for K samples: ceil(q K - 1e-9) upwards, floor(q K + 1e-9) downwards (0.9 * 30 is 27,
    whatever the product rounds to)."""
    if self.quantiles is None:
      return self.ranks
    K = int(n_climatology)
    return tuple(int(math.ceil(q * K - 1e-9)) if d > 0 else int(math.floor(q * K + 1e-9))
                 for q, d in zip(self.quantiles, self.directions))


class EfiScores(AdditiveScores):
  """The raw results of `gc_ens_efi_score`: `sums` [B, c_out, 6] float64 = sum w (1, f, o, f o, f^2, o^2) over the counted
  nodes -- f the EFI, o the observed index -- and the integer tables `weighted` / `counts` [T, B, c_out, 2, E] uint64 (axis -2:
  the truth outside / inside event t, axis -1: the EFI bin [-1 + 2 e / E, -1 + 2 (e + 1) / E), f = 1 in the last), with M,
  K, the ranks and directions of the events, the `scale` of the quantised node weights and the points `invalid`.  All of
  it adds over dates.  Scores of the sums are [B, c_out], scores of the tables [T, B, c_out]; a zero denominator gives NaN.
  The ROC is that of the warning "f >= threshold" for an upper event (direction +1) and "f < threshold" for a lower one."""
  _adds = ("sums", "weighted", "counts", "invalid")
  _same = {"n_members": "members", "n_climatology": "climatological samples", "ranks": "ranks", "directions": "directions",
           "scale": "scale"}
  _listed = ("efi_mean", "observed_mean", "correlation", "valid_weight")
  _what = "EFI scores"

  def __init__(self, sums, weighted, counts, n_members: int, n_climatology: int, ranks: Sequence[int] = (),
               directions: Sequence[int] = (), scale: float = 1.0, invalid: int = 0):
    self.sums = np.asarray(sums, dtype=np.float64)
    self.weighted = np.asarray(weighted, dtype=np.uint64)
    self.counts = np.asarray(counts, dtype=np.uint64)
    self.n_members, self.n_climatology, self.invalid = int(n_members), int(n_climatology), int(invalid)
    self.ranks, self.directions = tuple(int(r) for r in ranks), tuple(int(np.sign(d)) for d in directions)
    self.scale = float(scale)
    if self.n_members < 2 or self.n_climatology < 2:
      raise ValueError("n_members and n_climatology must be >= 2")
    if self.sums.ndim != 3 or self.sums.shape[-1] != 6:
      raise ValueError(f"sums must be [batch, channels, 6], got {self.sums.shape}")
    T = len(self.ranks)
    if len(self.directions) != T or any(d == 0 for d in self.directions):
      raise ValueError(f"directions must be {T} non-zero signs")
    if (self.weighted.ndim != 5 or self.weighted.shape[:4] != (T,) + self.sums.shape[:2] + (2,)
        or not 2 <= self.weighted.shape[4] <= 32):
      raise ValueError(f"weighted must be [{T}, {self.sums.shape[0]}, {self.sums.shape[1]}, 2, E] with E in 2..32, "
                       f"got {self.weighted.shape}")
    if self.counts.shape != self.weighted.shape:
      raise ValueError(f"counts must be {self.weighted.shape}, got {self.counts.shape}")
    if not (self.scale > 0.0 and math.isfinite(self.scale)):
      raise ValueError("scale must be positive and finite")

  _ratio = staticmethod(ClimatologyScores._ratio)

  @property
  def n_bins(self) -> int:
    return int(self.weighted.shape[-1])

  @property
  def valid_weight(self) -> np.ndarray:
    return self.sums[..., 0]

  @property
  def efi_mean(self) -> np.ndarray:
    """The weighted mean EFI over the counted nodes."""
    return self._ratio(self.sums[..., 1], self.sums[..., 0])

  @property
  def observed_mean(self) -> np.ndarray:
    return self._ratio(self.sums[..., 2], self.sums[..., 0])

  @property
  def correlation(self) -> np.ndarray:
    """The weighted (centred) correlation of the EFI and the observed index."""
    s0 = self.sums[..., 0]
    mf, mo = self.efi_mean, self.observed_mean
    cov = self._ratio(self.sums[..., 3], s0) - mf * mo
    vf, vo = self._ratio(self.sums[..., 4], s0) - mf * mf, self._ratio(self.sums[..., 5], s0) - mo * mo
    prod = vf * vo
    return self._ratio(cov, np.sqrt(np.where(prod > 0.0, prod, np.nan)))

  # -- the tables in float64 (exact: see quantize_node_weights), the bins in the order of rising alarm ---------
  def _tables(self) -> Tuple[np.ndarray, np.ndarray]:
    """(o_e, n_e - o_e) [T, B, c_out, E]: the weight of the truth inside / outside the event per bin, the bins of a lower
    event reversed so that the warning is always "bin >= j"."""
    inside = self.weighted[..., 1, :].astype(np.float64) / self.scale
    outside = self.weighted[..., 0, :].astype(np.float64) / self.scale
    for t, d in enumerate(self.directions):
      if d < 0:
        inside[t], outside[t] = inside[t, ..., ::-1].copy(), outside[t, ..., ::-1].copy()
    return inside, outside

  @property
  def base_rate(self) -> np.ndarray:
    """How often the truth lay in the event, [T, B, c_out]."""
    inside, outside = self._tables()
    return self._ratio(inside.sum(-1), inside.sum(-1) + outside.sum(-1))

  def _rates(self) -> Tuple[np.ndarray, np.ndarray]:
    """Hit rate and false-alarm rate of the warnings j = 0 .. E ("bin >= j" in the order of rising alarm): [T, B, c_out, E + 1]."""
    inside, outside = self._tables()
    zero = np.zeros(inside.shape[:-1] + (1,))
    tail = lambda a: np.concatenate([np.cumsum(a[..., ::-1], axis=-1)[..., ::-1], zero], axis=-1)
    return self._ratio(tail(inside), inside.sum(-1)[..., None]), self._ratio(tail(outside), outside.sum(-1)[..., None])

  def _level(self, threshold: float) -> np.ndarray:
    """The warning level j [T] of an EFI threshold, which must be a bin edge -1 + 2 j / E."""
    E = self.n_bins
    edge = (float(threshold) + 1.0) * 0.5 * E
    j = int(round(edge))
    if abs(edge - j) > 1e-9 or not 0 <= j <= E:
      raise ValueError(f"threshold must be a bin edge -1 + 2 j / {E}, j = 0 .. {E}, got {threshold}")
    return np.array([j if d > 0 else E - j for d in self.directions], dtype=np.int64)   # (a lower event: bins reversed)

  def hit_rate(self, threshold: float) -> np.ndarray:
    """Of the warning at EFI `threshold` (a bin edge): the weight of the warned events over that of all events, [T, B, c_out]."""
    h, _ = self._rates()
    return np.stack([h[t, ..., j] for t, j in enumerate(self._level(threshold))]) if len(self.ranks) else h[..., 0]

  def false_alarm_rate(self, threshold: float) -> np.ndarray:
    _, f = self._rates()
    return np.stack([f[t, ..., j] for t, j in enumerate(self._level(threshold))]) if len(self.ranks) else f[..., 0]

  @property
  def roc_area(self) -> np.ndarray:
    """The trapezoid rule through the E + 1 points (false-alarm rate, hit rate) of the bin edges, [T, B, c_out]."""
    h, f = self._rates()
    return (0.5 * (f[..., :-1] - f[..., 1:]) * (h[..., :-1] + h[..., 1:])).sum(axis=-1)


# ---------------------------------------------------------------------------------------------
# score maps: the marginal scores per grid point, added up over dates (gc_ens_map_*)
# ---------------------------------------------------------------------------------------------
class MapSpec:
  """What the score maps of a store cover: `variables` (None: every target variable), `levels` (None: every level; else the
  values of the `level` coordinate to keep, for the variables that have levels), and with `events` the event planes of the
  store's `EventSpec` (its T thresholds, from the codes its event score leaves on the device)."""

  def __init__(self, variables: Optional[Sequence[str]] = None, levels: Optional[Sequence[float]] = None, events: bool = False):
    if isinstance(variables, str):
      variables = (variables,)
    self.variables = None if variables is None else tuple(str(v) for v in variables)
    self.levels = None if levels is None else tuple(float(v) for v in np.asarray(levels, dtype=np.float64).reshape(-1))
    self.events = bool(events)
    if self.variables is not None and (not self.variables or len(set(self.variables)) != len(self.variables)):
      raise ValueError("variables must be a non-empty list of distinct names (or None for all)")
    if self.levels is not None and (not self.levels or len(set(self.levels)) != len(self.levels)):
      raise ValueError("levels must be a non-empty list of distinct values (or None for all)")

  def __eq__(self, other):
    return isinstance(other, MapSpec) and (self.variables, self.levels, self.events) == (other.variables, other.levels, other.events)

  def __hash__(self):
    return hash((self.variables, self.levels, self.events))

  def channels(self, template) -> np.ndarray:
    """The selected channels [C'] int32, ascending, in the channel order of `datasets.channel_layout(template)`."""
    template = datasets.as_dataset(template)
    layout = {name: (off, n) for name, off, n in datasets.channel_layout(template)}
    for name in self.variables or ():
      if name not in layout:
        raise ValueError(f"{name!r} is not a target variable")
    level_idx = None
    if self.levels is not None:
      if "level" not in template.coords:
        raise ValueError("levels given, but the template has no 'level' coordinate")
      coord = np.asarray(template.coords["level"], dtype=np.float64).reshape(-1)
      level_idx = []
      for v in self.levels:
        at = np.flatnonzero(coord == v)
        if at.size != 1:
          raise ValueError(f"level {v:g} is not one of the template's levels {coord.tolist()}")
        level_idx.append(int(at[0]))
    out = []
    for name in sorted(layout):
      if self.variables is not None and name not in self.variables:
        continue
      off, n = layout[name]
      var = template[name]
      stack = [d for d in var.dims if d not in datasets.PRESERVED]
      idx = np.arange(n).reshape([var.sizes[d] for d in stack])
      if level_idx is not None and "level" in stack:
        idx = np.take(idx, level_idx, axis=stack.index("level"))
      out.extend(int(off + i) for i in idx.reshape(-1))
    if not out:
      raise ValueError("the map spec selects no channel")
    return np.array(sorted(out), dtype=np.int32)


def _map_channels(channels, n: int) -> Tuple[int, ...]:
  ch = tuple(range(n)) if channels is None else tuple(int(c) for c in np.asarray(channels).reshape(-1))
  if len(ch) != n:
    raise ValueError(f"channels must name the {n} channels of the planes, got {len(ch)}")
  return ch


def _map_field(values, counted, template, channels, name: Optional[str]):
  """[G, B, C'] -> a Dataset on the template's grid: the selected channels of the template's variables, NaN elsewhere and
  where the point never counted; `name`: a prefix of the variable names (None: as in the template)."""
  template = datasets.as_dataset(template)
  sizes = template.sizes
  n_lat, n_lon = int(sizes["lat"]), int(sizes["lon"])
  total = sum(n for _, _, n in datasets.channel_layout(template))
  v = np.where(counted, values, np.nan)
  G, B = v.shape[:2]
  if G != n_lat * n_lon:
    raise ValueError(f"the planes have {G} nodes, the template {n_lat} x {n_lon}")
  full = np.full((G, B, total), np.nan)
  full[:, :, list(channels)] = v
  stacked = np.transpose(full.reshape(n_lat, n_lon, B, total), (2, 0, 1, 3))
  like = datasets.Dataset({k: datasets.Variable(var.dims, np.broadcast_to(np.zeros(()), tuple(B if d == "batch" else n for d, n in
                                                                                     zip(var.dims, np.shape(var.data)))))
                           for k, var in template.items()}, template.coords)
  ds = datasets.stacked_to_dataset(stacked, like)
  if name is None:
    return ds
  return datasets.Dataset({f"{name}_{k}": var for k, var in ds.items()}, ds.coords)


class MapRegionScores(EnsembleScores):
  """`ScoreMaps.region`: the column sums of `EnsembleScores` formed from map planes.  Of the rank histogram the planes hold
  the two end bins alone; the bins between them are zero here, and `valid_points` comes from the N0 plane."""
  _listed = tuple(x for x in EnsembleScores._listed if x != "rank_histogram") + ("outlier_low", "outlier_high")

  def __init__(self, sums, rank_histogram, n_members: int, points=None):
    super().__init__(sums, rank_histogram, n_members)
    self.points = self.rank_histogram.sum(axis=-1) if points is None else np.asarray(points, dtype=np.uint64)

  @property
  def valid_points(self) -> np.ndarray:
    return self.points

  @property
  def outlier_low(self) -> np.ndarray:
    return self.rank_histogram[..., 0] / self.points.astype(np.float64)

  @property
  def outlier_high(self) -> np.ndarray:
    return self.rank_histogram[..., -1] / self.points.astype(np.float64)


class ScoreMaps:
  """The raw planes of `gc_ens_map_download` for one slot: `sums` [6, G, B, C'] float64 (P0 .. P5: the per-date e, e^2, s2, ae, d
  and c^2 of a point, added date after date), `counts` [3, G, B, C'] uint32 (N0 dates counted, N1 dates with the truth below
  every member, N2 above every member), with the member count M, the `channels` [C'] the planes cover and `dates`, the
  calls that were added.  Every score is [G, B, C'] float64, NaN where the point never counted.  The planes add over dates
  (`merge`); scores do not."""

  def __init__(self, sums, counts, n_members: int, channels=None, dates: int = 0):
    self.sums = np.asarray(sums, dtype=np.float64)
    self.counts = np.asarray(counts, dtype=np.uint32)
    self.n_members = int(n_members)
    if self.n_members < 2:
      raise ValueError("n_members must be >= 2")
    if self.sums.ndim != 4 or self.sums.shape[0] != 6:
      raise ValueError(f"sums must be [6, G, batch, channels], got {self.sums.shape}")
    if self.counts.shape != (3,) + self.sums.shape[1:]:
      raise ValueError(f"counts must be {(3,) + self.sums.shape[1:]}, got {self.counts.shape}")
    self.channels = _map_channels(channels, self.sums.shape[-1])
    self.dates = int(dates)

  # -- the planes
  def _p(self, k: int) -> np.ndarray:
    return self.sums[k]

  @property
  def valid_dates(self) -> np.ndarray:
    """N0: the dates on which the point counted."""
    return self.counts[0]

  @property
  def _n(self) -> np.ndarray:
    n = self.counts[0].astype(np.float64)
    return np.where(n > 0.0, n, np.nan)

  @property
  def bias(self) -> np.ndarray:
    return self._p(0) / self._n

  @property
  def rmse(self) -> np.ndarray:
    """Of the ensemble mean."""
    return np.sqrt(self._p(1) / self._n)

  @property
  def spread(self) -> np.ndarray:
    return np.sqrt(self._p(2) / self._n)

  @property
  def spread_skill_ratio(self) -> np.ndarray:
    """sqrt((M+1)/M) spread / rmse: 1 for a calibrated ensemble of any size."""
    m = float(self.n_members)
    with np.errstate(divide="ignore", invalid="ignore"):
      return np.sqrt((m + 1.0) / m) * self.spread / self.rmse

  @property
  def crps(self) -> np.ndarray:
    """The fair CRPS."""
    return (self._p(3) - 0.5 * self._p(4)) / self._n

  @property
  def crps_ensemble(self) -> np.ndarray:
    """The CRPS of the M-member empirical distribution (pair term normalised by M^2)."""
    m = float(self.n_members)
    return (self._p(3) - 0.5 * (m - 1.0) / m * self._p(4)) / self._n

  @property
  def crps_stderr(self) -> np.ndarray:
    """The standard error of `crps` over the dates: sqrt((P5 / N0 - crps^2) / (N0 - 1)); NaN with fewer than two dates."""
    n = self._n
    crps = self.crps
    with np.errstate(divide="ignore", invalid="ignore"):
      var = (self._p(5) / n - crps * crps) / np.where(n > 1.0, n - 1.0, np.nan)
    return np.sqrt(np.maximum(var, 0.0))

  @property
  def outlier_low(self) -> np.ndarray:
    """The frequency of the truth below every member (1 / (M + 1) for a calibrated ensemble)."""
    return self.counts[1] / self._n

  @property
  def outlier_high(self) -> np.ndarray:
    return self.counts[2] / self._n

  # -- algebra
  def scaled(self, channel_scale) -> "ScoreMaps":
    """The planes of a x + b in place of x (members and truth alike), a = channel_scale [C'], any b: P0 scales with a, P3 and
    P4 with |a|, P1, P2 and P5 with a^2; for a < 0 the two outlier counts change places."""
    a = np.asarray(channel_scale, dtype=np.float64).reshape(-1)
    if a.shape != (self.sums.shape[-1],):
      raise ValueError(f"channel_scale must have shape ({self.sums.shape[-1]},)")
    if np.any(a == 0.0) or not np.all(np.isfinite(a)):
      raise ValueError("channel_scale must be finite and non-zero")
    f = np.stack([a, a * a, a * a, np.abs(a), np.abs(a), a * a])
    counts = self.counts.copy()
    neg = a < 0.0
    counts[1][..., neg], counts[2][..., neg] = self.counts[2][..., neg], self.counts[1][..., neg]
    return ScoreMaps(self.sums * f[:, None, None, :], counts, self.n_members, self.channels, self.dates)

  @staticmethod
  def merge(parts: Sequence["ScoreMaps"]) -> "ScoreMaps":
    """The planes over the dates of all parts: a left fold of plane additions, in the order of `parts` -- what the device
    holds after the same dates were accumulated in that order."""
    parts = list(parts)
    if not parts:
      raise ValueError("merge: nothing to merge")
    first = parts[0]
    sums, counts, dates = first.sums.copy(), first.counts.copy(), first.dates
    for p in parts[1:]:
      if p.n_members != first.n_members or p.channels != first.channels or p.sums.shape != first.sums.shape:
        raise ValueError("merge: the score maps differ in members, channels or shape")
      sums = sums + p.sums
      counts = counts + p.counts
      dates += p.dates
    return ScoreMaps(sums, counts, first.n_members, first.channels, dates)

  def region(self, weights) -> MapRegionScores:
    """The column sums of `EnsembleScores` over the nodes: S0 = sum_g w N0, S1 .. S5 = sum_g w P0 .. P4, per (batch, channel);
    `weights` [G] (a mask, or node weights times a mask).  Any region chosen after the fact is such a weighted sum of planes."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape != (self.sums.shape[1],):
      raise ValueError(f"weights must have shape ({self.sums.shape[1]},)")
    planes = np.concatenate([self.counts[:1].astype(np.float64), self.sums[:5]])
    sums = np.moveaxis(np.tensordot(w, planes, axes=([0], [1])), 0, -1)          # [B, C', 6]
    inside = w != 0.0
    hist = np.zeros(sums.shape[:2] + (self.n_members + 1,), np.uint64)
    hist[..., 0] = self.counts[1][inside].sum(axis=0, dtype=np.uint64)
    hist[..., -1] = self.counts[2][inside].sum(axis=0, dtype=np.uint64)
    return MapRegionScores(sums, hist, self.n_members, self.counts[0][inside].sum(axis=0, dtype=np.uint64))

  def to_dataset(self, template, name: str = "crps"):
    """The score `name` (a property of this class) as a Dataset on the lat / lon of `template`: the variables of the template,
    NaN at the points that never counted and in the channels the maps do not cover."""
    if name.startswith("_") or not isinstance(getattr(type(self), name, None), property):
      raise ValueError(f"{name!r} is not a score of {type(self).__name__}")
    return _map_field(getattr(self, name), self.counts[0] > 0, template, self.channels, None)


class EventMaps:
  """The event planes of `gc_ens_map_download` for one slot: `events` [T, 5, G, B, C'] uint32 (E0 dates counted, E1 sum k,
  E2 sum k^2, E3 sum k o, E4 sum o; k members in the event, o the truth in it), with M, the `directions` [T] of the events,
  the `channels` and the `dates` added.  Scores are [T, G, B, C'] float64, NaN where the point never counted."""

  def __init__(self, events, n_members: int, directions=None, channels=None, dates: int = 0):
    self.events = np.asarray(events, dtype=np.uint32)
    self.n_members = int(n_members)
    if self.n_members < 2:
      raise ValueError("n_members must be >= 2")
    if self.events.ndim != 5 or self.events.shape[1] != 5:
      raise ValueError(f"events must be [T, 5, G, batch, channels], got {self.events.shape}")
    self.directions = None if directions is None else tuple(int(np.sign(d)) for d in directions)
    if self.directions is not None and len(self.directions) != self.events.shape[0]:
      raise ValueError(f"directions must be {self.events.shape[0]} signs")
    self.channels = _map_channels(channels, self.events.shape[-1])
    self.dates = int(dates)

  @staticmethod
  def _brier(e, m: float) -> np.ndarray:
    """(E2 / M^2 - 2 E3 / M + E4) / E0 from planes (or weighted sums of planes) in float64: the numerator as the integer
    E2 - 2 M E3 + M^2 E4, so nothing cancels in rounded numbers."""
    e0 = np.where(e[:, 0] > 0.0, e[:, 0], np.nan)
    return (e[:, 2] - 2.0 * m * e[:, 3] + m * m * e[:, 4]) / (m * m * e0)

  @property
  def valid_dates(self) -> np.ndarray:
    return self.events[:, 0]

  @property
  def brier(self) -> np.ndarray:
    return self._brier(self.events.astype(np.float64), float(self.n_members))

  @property
  def base_rate(self) -> np.ndarray:
    e = self.events.astype(np.float64)
    return e[:, 4] / np.where(e[:, 0] > 0.0, e[:, 0], np.nan)

  @property
  def forecast_probability(self) -> np.ndarray:
    e = self.events.astype(np.float64)
    return e[:, 1] / (float(self.n_members) * np.where(e[:, 0] > 0.0, e[:, 0], np.nan))

  @staticmethod
  def merge(parts: Sequence["EventMaps"]) -> "EventMaps":
    parts = list(parts)
    if not parts:
      raise ValueError("merge: nothing to merge")
    first = parts[0]
    events, dates = first.events.copy(), first.dates
    for p in parts[1:]:
      if (p.n_members != first.n_members or p.channels != first.channels or p.events.shape != first.events.shape
          or p.directions != first.directions):
        raise ValueError("merge: the event maps differ in members, channels, directions or shape")
      events = events + p.events
      dates += p.dates
    return EventMaps(events, first.n_members, first.directions, first.channels, dates)

  def region(self, weights) -> Dict[str, np.ndarray]:
    """{"brier", "base_rate", "forecast_probability", "valid_weight"}: [T, B, C'] over the nodes with `weights` [G] -- with the
    integer weights of `quantize_node_weights` the sums are exact below 2^53, as the tables of `EventScores` are."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape != (self.events.shape[2],):
      raise ValueError(f"weights must have shape ({self.events.shape[2]},)")
    e = np.tensordot(self.events.astype(np.float64), w, axes=([2], [0]))             # [T, 5, B, C']
    e0 = np.where(e[:, 0] > 0.0, e[:, 0], np.nan)
    return {"brier": self._brier(e, float(self.n_members)), "base_rate": e[:, 4] / e0,
            "forecast_probability": e[:, 1] / (float(self.n_members) * e0), "valid_weight": e[:, 0]}

  def to_dataset(self, template, name: str = "brier", threshold: int = 0):
    if name.startswith("_") or not isinstance(getattr(type(self), name, None), property):
      raise ValueError(f"{name!r} is not a score of {type(self).__name__}")
    return _map_field(getattr(self, name)[threshold], self.events[threshold, 0] > 0, template, self.channels, None)


# ---------------------------------------------------------------------------------------------
# the scorers of a member store, each declared once
# ---------------------------------------------------------------------------------------------
class Scorer(NamedTuple):
  """One row of `SCORERS`: everything `ScoredStore`, the rollout's results and its per-lead loop know about a scorer."""
  name: str                                   # the series on a result; with `score`, the `ScoredStore` keyword that switches it on
  word: Optional[str]                         # what an error message calls it (None: the scores themselves, never checked alone)
  settings: Tuple[str, ...] = ()              # the companion keywords and attributes of `ScoredStore`
  set: Optional[Callable] = None              # set(store): hands the settings to `store.handle`; they survive every score
  score: Optional[Callable] = None            # score(store, truth) -> the score object (None: not scored through `_score`)
  scaled: bool = True                         # the scores have a `scaled(scale)` twin: the raw series is `<name>_normalized`
  optional: bool = True                       # absent from `vars(result)` unless the run asked for it
  carried_by: Tuple[str, ...] = ("ensemble", "derived", "window")   # the results (`_SeriesResult._carried_as`) that hold it
  from_spec: Optional[Callable] = None        # from_spec(spec, template, pack) -> {setting: value} for a spec given per store

  @property
  def series(self) -> Tuple[str, ...]:
    return (self.name, self.name + "_normalized") if self.scaled else (self.name,)


def _fractions_plan(store):
  """The windows of the store's EventSpec (None without `scales_km`): made by `EventSpec.packed` for the store's own grid."""
  spec = store.events
  if getattr(spec, "scales_km", None) is None:
    return None
  if spec.fractions_plan is None:
    raise ValueError("an EventSpec with scales_km needs its windows: call packed(template) (or windows) for the store's grid")
  return spec.fractions_plan


def _set_events(store):
  store.handle.ens_event_set(store.thresholds, store.events.directions, store.weight_q[0])
  plan = _fractions_plan(store)
  if plan is not None:
    store.handle.ens_fss_set(*plan)


def _score_events(store, truth):
  weighted, counts, invalid = store.handle.ens_event_score(truth)
  scores = EventScores(weighted, counts, store.n_members, store.events.directions, store.weight_q[1], invalid)
  if _fractions_plan(store) is not None:
    scores.fractions = FractionsScores(store.handle.ens_fss_score(), scores.weighted.sum(axis=(-1, -2)), store.n_members,
                                       store.events.directions, store.events.scales_km, store.weight_q[1])
  return scores


def _score_order(store, truth):
  bins, extra, pinball, counts, _ = store.handle.ens_order_score(truth)
  return OrderScores(bins, extra, pinball, counts, store.n_members, store.order)


def _score_energy(store, truth):
  d2, s0, invalid = store.handle.ens_energy_score(truth)
  return EnergyScores.from_sums(d2, s0, store.n_members, store.energy.get("names"), invalid)


def _score_variogram(store, truth):
  sums, counts = store.handle.ens_variogram_score(truth)
  return VariogramScores(sums, counts, store.n_members, store.variogram["offsets"], store.variogram["p"])


def _score_tails(store, truth):
  sums, counts, invalid = store.handle.ens_tail_score(truth)
  return TailScores(sums, counts, store.n_members, store.tails.directions, invalid)


def _score_regions(store, truth):
  sums, hist, invalid = store.handle.ens_region_score(truth)
  return RegionScores(store.regions.names, sums, hist, store.n_members, invalid)


# In the order in which a store is configured and a lead time is scored, which is the order of the series on a result.  The
# scores, the spectra (the main handle only) and the climatology (a second handle: `ScoredStore.score_climatology`) are rows for
# what a row can say of them.  The rows up to the climatology predate the `optional` rule: their series are always set.
SCORERS = [
    Scorer("scores", None, optional=False),
    Scorer("spectra", "spectra", optional=False, carried_by=("ensemble",)),
    Scorer("events", "events", ("thresholds", "weight_q"), scaled=False, optional=False, score=_score_events,
           set=_set_events),                                                   # (the fractions of the events ride on this row)
    Scorer("order", "order statistics", optional=False, score=_score_order, set=lambda s: s.handle.ens_order_set(s.order)),
    Scorer("climatology", "climatology scores", optional=False, carried_by=("ensemble", "derived")),
    Scorer("energy", "energy scores", scaled=False, score=_score_energy,         # (in the store's own units: no `scaled`)
           set=lambda s: s.handle.ens_energy_set(s.energy["n_groups"], s.energy["group"], s.energy["scale"])),
    Scorer("variogram", "variogram scores", score=_score_variogram,
           set=lambda s: s.handle.ens_variogram_set(*(s.variogram[k] for k in ("n_lat", "n_lon", "offsets", "p")))),
    Scorer("tails", "tail scores", ("tail_thresholds",), score=_score_tails,
           set=lambda s: s.handle.ens_tail_set(s.tail_thresholds, s.tails.directions),
           from_spec=lambda spec, template, pack: {"tail_thresholds": pack(spec, template)}),
    Scorer("regions", "region scores", ("region_bits",), score=_score_regions,
           set=lambda s: s.handle.ens_region_set(s.region_bits, s.regions.n_regions),
           from_spec=lambda spec, template, pack: {"region_bits": spec.node_bits(template)}),
]


def _set_efi(store):
  store._efi_set_for = None                     # (the ranks need K: the next `score_efi` hands them over)  pylint: disable=protected-access


def _score_efi(store, truth):
  return store.score_efi(truth)


# The extreme forecast index, scored next to the climatology row (it reads the same second handle, after that row has
# filled it).  It stands beside the table, not in it: the series of the table's rows are a recorded public surface
# (tests/test_scorer_table.py) that a new name would change, so the results carry `efi` as they carry `features` -- an
# attribute that exists only on the result of a run that asked for it.
EFI_SCORER = Scorer("efi", "extreme forecast index", set=_set_efi, score=_score_efi, scaled=False,
                    carried_by=("ensemble", "derived"))


def _set_maps(store):
  """Makes (and zeroes) the accumulators of the store's handle.  A store with `maps_resident` keeps what the handle holds
  when it was made for the same channels, slots and thresholds -- the sums of earlier runs -- and refuses another plan."""
  T = store.events.n_thresholds if store.maps.events else 0
  key = (None if store.map_channels is None else tuple(int(c) for c in store.map_channels), store.map_slots, T)
  held = getattr(store.handle, "_resident_map_plan", None)
  if store.maps_resident and held is not None:
    if held != key:
      raise ValueError(f"maps_resident: the handle holds sums of another plan or horizon (channels, slots, thresholds {held}, now "
                       f"{key}): download them and call reset_maps(), or run without maps_resident")
    return
  store.handle.ens_map_set(store.map_channels, store.map_slots, T)
  store.handle._resident_map_plan = key if store.maps_resident else None   # pylint: disable=protected-access


# The score maps (gc_ens_map_*): per-point accumulators over dates.  Beside the table for the reason the index is: the
# table's series are a recorded surface.  `set` makes (and zeroes) the accumulators; a store adds a date with
# `accumulate_maps`, so the row has no `score` of the per-lead kind.
MAP_SCORER = Scorer("maps", "score maps", ("map_channels", "map_slots"), set=_set_maps, scaled=True)


def scorer(name: str) -> Scorer:
  return next(row for row in SCORERS + [EFI_SCORER, MAP_SCORER] if row.name == name)


# ---------------------------------------------------------------------------------------------
# a member store that gets scored
# ---------------------------------------------------------------------------------------------
class ScoredStore:
  """The member store of one handle and everything that is scored from it: the M members it holds, the node weights
  (None: `ens_score` is not used on it), optionally the events counted on it -- an `EventSpec`, its packed `thresholds`
  in the members' units and `weight_q` = `quantize_node_weights(...)` -- and optionally the `plan` (`DerivedSpec.plan`) that
  fills it from the store of a `source` handle (`ens_derive`), or instead the `feature_plan` (`FeatureSpec.plan`) that fills
  it with the strike fields of the centres found in the source's store (`ens_feature`; `centres()` has the lists), or instead the
  `band_plan` (`BandSpec.plan`) that fills it with the band-limited fields of the source's store (`ens_band`; the handle holds the
  analysis tables already: `spectra.ensure_tables`), and optionally `order`: the probabilities of the quantile
  fields `score_order` leaves on the device next to its `OrderScores`, optionally `energy` and `variogram`: the plans
  (`EnergySpec.plan`, `VariogramSpec.plan`) of `score_energy` and `score_variogram`, and optionally `climatology`: a second handle of the
  same graph, batch and c_out (`Denoiser.climatology_handle`) whose member store takes the K climatological samples
  `score_climatology` scores the members against -- on a derived view together with `climatology_source`, the handle whose
  store holds the samples the view's plan is applied to, and optionally `tails`: an `EventSpec` read as tails (direction
  > 0: the upper tail) with its packed `tail_thresholds` in the members' units, for `score_tails`, and optionally `regions`: a
  `RegionSpec` with `region_bits` = `regions.node_bits(template)`, for `score_regions`.  `EnsembleSampler` and `EnsembleRollout`
  use one for the main store and one per derived view.

  `set_per_score`: the plan and the thresholds are not set once by `setup` but by every `score` -- two stores that share
  a handle, or thresholds that change from call to call (assign `thresholds` before the call)."""

  def __init__(self, handle, n_members: int, node_weight=None, *, plan=None, source=None, set_per_score: bool = False,
               climatology=None, climatology_source=None, feature_plan=None, band_plan=None, efi=None, maps=None,
               map_channels=None, map_slots: int = 1, maps_resident: bool = False, **scorers):
    """`scorers`: per row of `SCORERS` with a `score`, its name (what switches it on) and its settings, None by default.
    `efi`: an `EfiSpec` for `score_efi` (it needs the `climatology` handle, and `weight_q` where it has events).
    `maps`: a `MapSpec` for `accumulate_maps` / `download_maps` / `reset_maps`, with `map_channels` = `maps.channels(template)`
    (None: every channel of the store) and `map_slots` (1..128) the slots the accumulators get; `maps_resident`: `configure`
    keeps the sums the handle already holds for the same plan (`forget_maps` ends that)."""
    for row in (r for r in SCORERS if r.score is not None):
      for key in (row.name,) + row.settings:
        setattr(self, key, scorers.pop(key, None))
    if scorers:
      raise TypeError(f"ScoredStore() got an unexpected keyword argument {next(iter(scorers))!r}")
    if self.regions is not None and self.region_bits is None:
      raise ValueError("regions need their node bits (RegionSpec.node_bits)")
    if climatology_source is not None and (climatology is None or (plan is None and band_plan is None)):
      raise ValueError("a climatology source goes with a climatology handle and a derive plan (or a band plan)")
    if self.events is not None and self.weight_q is None:
      raise ValueError("events need the quantised node weights (quantize_node_weights)")
    if efi is not None:
      if not isinstance(efi, EfiSpec):
        raise TypeError("efi must be an EfiSpec")
      if climatology is None:
        raise ValueError("the extreme forecast index needs a climatology handle")
      if efi.n_events and self.weight_q is None:
        raise ValueError("the events of an EfiSpec need the quantised node weights (quantize_node_weights)")
    self.efi, self._efi_set_for = efi, None      # (K the events and bins were last handed over for)
    if maps is not None:
      if not isinstance(maps, MapSpec):
        raise TypeError("maps must be a MapSpec")
      if set_per_score:
        raise ValueError("maps: a store that shares its handle with another (set_per_score) cannot keep score maps -- two "
                         "views must not add into one accumulator")
      if maps.events and self.events is None:
        raise ValueError("maps: event planes (MapSpec(events=True)) need the store's EventSpec (events=...)")
      if not 1 <= int(map_slots) <= 128:
        raise ValueError("map_slots must be in 1..128")
      if map_channels is None and (maps.variables is not None or maps.levels is not None):
        raise ValueError("maps: a MapSpec that selects variables or levels needs map_channels = maps.channels(template)")
    self.maps = maps
    self.map_channels = None if map_channels is None else np.asarray(map_channels, dtype=np.int32).reshape(-1)
    self.map_slots, self.maps_resident = int(map_slots), bool(maps_resident)
    if plan is not None and feature_plan is not None:
      raise ValueError("a store is filled by a derive plan or by a feature plan, not both")
    if band_plan is not None and (plan is not None or feature_plan is not None):
      raise ValueError("a store is filled by one of a derive plan, a feature plan and a band plan, not two")
    if (plan is None and feature_plan is None and band_plan is None) != (source is None):
      raise ValueError("a derive plan (or a feature plan, or a band plan) and its source handle go together")
    self.handle, self.n_members, self.node_weight = handle, int(n_members), node_weight
    self.plan, self.source, self.set_per_score = plan, source, bool(set_per_score)
    self.feature_plan, self.band_plan = feature_plan, band_plan
    if self.order is not None:
      self.order = tuple(float(p) for p in np.asarray(self.order, dtype=np.float64).reshape(-1))
    self.climatology, self.climatology_source = climatology, climatology_source
    self._clim_reserved = 0                      # K of the store this object reserved on the climatology handle
    self._clim_plan_set = False                  # the plan has been handed to the climatology handle (a derived view)

  def reserve(self) -> None:
    self.handle.ens_reserve(self.n_members)
    if self.node_weight is not None:
      self.handle.ens_set_node_weight(self.node_weight)

  def _set_plan(self) -> None:
    if self.plan is not None:
      self.handle.ens_derive_set(**self.plan)
    if self.feature_plan is not None:
      self.handle.ens_feature_set(**self.feature_plan)
    if self.band_plan is not None:
      self.handle.ens_band_set(**self.band_plan)

  def configure(self) -> None:
    """The plan, then every scorer that is switched on, in the order of `SCORERS` -- the thresholds, the probabilities, the
    multivariate plans, the tails and the regions: all survive `ens_reserve` and every score."""
    self._set_plan()
    for row in SCORERS + [EFI_SCORER, MAP_SCORER]:
      if row.set is not None and getattr(self, row.name) is not None:
        row.set(self)

  def setup(self) -> None:
    self.reserve()
    if not self.set_per_score:
      self.configure()

  def _score(self, row: Scorer, truth=None):
    """The scores of one row of `SCORERS` (None where the store does not have it switched on)."""
    if getattr(self, row.name) is None:
      return None
    if self.set_per_score:
      row.set(self)
    return row.score(self, truth)

  def score_events(self, truth=None) -> Optional["EventScores"]:
    """The event tables of the store (None without an EventSpec); `truth` None: the truth already on the device."""
    return self._score(scorer("events"), truth)

  def score_order(self, truth=None) -> Optional["OrderScores"]:
    """The order statistics of the store (None without `order`); `truth` None: the truth already on the device.  On a
    derived view (a store with a plan) the DERIVED members are scored: call it after `score`, which fills the view, and
    leave `truth` None."""
    return self._score(scorer("order"), truth)

  def score_energy(self, truth=None) -> Optional["EnergyScores"]:
    """The energy score of the store over the groups of `energy` (None without it), in the store's own units; `truth` None:
    the truth already on the device.  On a derived view the DERIVED members are scored: call it after `score`."""
    return self._score(scorer("energy"), truth)

  def score_variogram(self, truth=None) -> Optional["VariogramScores"]:
    """The raw variogram sums of the store at the offsets of `variogram` (None without it), in the store's own units;
    `truth` None: the truth already on the device.  On a derived view call it after `score`."""
    return self._score(scorer("variogram"), truth)

  def score_tails(self, truth=None) -> Optional["TailScores"]:
    """The raw threshold-weighted CRPS sums of the store at the thresholds of `tails` (None without it), in the store's own
    units; `truth` None: the truth already on the device.  On a derived view call it after `score`."""
    return self._score(scorer("tails"), truth)

  def score_regions(self, truth=None) -> Optional["RegionScores"]:
    """The raw sums of `score` per region of `regions` (None without it), from one pass over the nodes of all regions, in the
    store's own units; `truth` None: the truth already on the device.  On a derived view call it after `score`."""
    return self._score(scorer("regions"), truth)

  def _reserve_climatology(self, K: int) -> None:
    if K != self._clim_reserved:
      self.climatology.ens_reserve(K)
      self._clim_reserved = K

  def load_climatology(self, fields) -> int:
    """The K (2..64) samples [G, B, c_out], in the members' units, into the climatology handle's store (reserved again only
    when K changes) -> K."""
    K = len(fields)
    self._reserve_climatology(K)
    for j, f in enumerate(fields):
      self.climatology.ens_push_host(j, f)
    return K

  def score_climatology(self, fields=None, truth=None, *, n_samples: Optional[int] = None,
                        source_truth=None) -> Optional["ClimatologyScores"]:
    """The members against a climatology (None without a climatology handle).  `fields`: the K (2..64) samples
    [G, B, c_out] in the members' units, pushed into the climatology handle's store with `ens_push_host` (its store is
    reserved again only when K changes); None: the samples already there.  `truth` None: the truth already on the device.
    On a derived view with a `climatology_source` the samples are instead made by `ens_derive` -- the view's plan applied
    to the `n_samples` samples in the source's store, with `source_truth` [G, B, c_src] (the truth in the source's units:
    the climatology handle has none of its own) -- and the DERIVED members are scored: call it after `score`."""
    if self.climatology is None:
      return None
    if self.climatology_source is not None:
      K = int(n_samples)
      self._reserve_climatology(K)
      band = self.band_plan is not None            # (the climatology handle of a band view holds the analysis tables already)
      if self.set_per_score or not self._clim_plan_set:
        if band:
          self.climatology.ens_band_set(**self.band_plan)
        else:
          self.climatology.ens_derive_set(**self.plan)
        self._clim_plan_set = True
      (self.climatology.ens_band if band else self.climatology.ens_derive)(self.climatology_source, source_truth)
    elif fields is not None:
      K = self.load_climatology(fields)
    else:
      K = self._clim_reserved
    sums, counts, invalid = self.handle.ens_clim_score(self.climatology, truth)
    return ClimatologyScores(sums, counts, self.n_members, K, invalid)

  def score_efi(self, truth=None, *, n_samples: Optional[int] = None) -> Optional["EfiScores"]:
    """The extreme forecast index of the members against the samples in the climatology handle's store, verified against
    the truth (None without an `EfiSpec`): call it after `score_climatology`, which fills that store.  `n_samples`: K of a
    store somebody else filled; `truth` None: the truth already on the device.  Both fields stay on the device
    (`efi_fields`)."""
    if self.efi is None:
      return None
    K = self._clim_reserved if n_samples is None else int(n_samples)
    ranks = self.efi.ranks_for(K)
    if self.set_per_score or self._efi_set_for != K:
      self.handle.ens_efi_set(ranks, self.efi.directions, self.efi.bins, None if self.weight_q is None else self.weight_q[0])
      self._efi_set_for = K
    sums, weighted, counts, invalid = self.handle.ens_efi_score(self.climatology, efi_table(K), truth)
    return EfiScores(sums, weighted, counts, self.n_members, K, ranks, self.efi.directions,
                     1.0 if self.weight_q is None else self.weight_q[1], invalid)

  def efi_field_without_truth(self) -> np.ndarray:
    """The EFI field [G, B, c_out] of the members against the samples in the climatology handle's store, downloaded: no truth,
    no weights, no events (`gc_ens_efi_fields`) -- what a real forecast, one without an analysis, can ask."""
    self.handle.ens_efi_fields(self.climatology, efi_table(self._clim_reserved))
    return self.handle.ens_efi_field(0)

  def efi_fields(self, *, observed: bool = True) -> Tuple[np.ndarray, ...]:
    """The EFI field [G, B, c_out] of the last `score_efi`, downloaded, and with `observed` the observed index too."""
    return tuple(self.handle.ens_efi_field(i) for i in range(2 if observed else 1))

  def _need_maps(self, who: str) -> None:
    if self.maps is None:
      raise ValueError(f"{who}: the store has no MapSpec (maps=...)")

  def accumulate_maps(self, slot: int, truth=None) -> None:
    """Adds the date in the store into the planes of `slot` (`gc_ens_map_accumulate`), and with `MapSpec(events=True)` the
    codes of the store's last event score into its event planes: call it after `score`, which fills a derived view and
    counts the events.  `truth` None: the truth already on the device."""
    self._need_maps("accumulate_maps")
    self.handle.ens_map_accumulate(slot, truth)
    if self.maps.events:
      self.handle.ens_map_accumulate_events(slot)

  def download_maps(self, slot: int):
    """-> `ScoreMaps` of `slot`, raw (in the members' units); with `MapSpec(events=True)` -> (`ScoreMaps`, `EventMaps`)."""
    self._need_maps("download_maps")
    sums, counts, events, dates = self.handle.ens_map_download(slot, self.maps.events)
    C = sums.shape[-1]
    channels = tuple(range(C)) if self.map_channels is None else tuple(int(c) for c in self.map_channels)
    maps = ScoreMaps(sums, counts, self.n_members, channels, int(dates[0]))
    if not self.maps.events:
      return maps
    return maps, EventMaps(events, self.n_members, self.events.directions, channels, int(dates[1]))

  def reset_maps(self, slot: Optional[int] = None) -> None:
    """Zeroes the planes of `slot` (None: of every slot)."""
    self._need_maps("reset_maps")
    self.handle.ens_map_reset(-1 if slot is None else int(slot))

  def forget_maps(self) -> None:
    """Zeroes every slot and lets the next `configure` make accumulators for another plan (the end of `maps_resident`)."""
    self.reset_maps()
    self.handle._resident_map_plan = None          # pylint: disable=protected-access

  def centres(self) -> Dict[str, list]:
    """The centres the last `score` found on a store with a `feature_plan` (`ens_feature_centres`), as `unpack_centres`
    gives them: {detector: [B][M + 1] entries}, field M the truth; with a `FeaturePlan` in physical units."""
    if self.feature_plan is None:
      raise ValueError("centres: the store has no feature plan")
    return unpack_centres(*self.handle.ens_feature_centres(), self.feature_plan)

  def quantile_fields(self) -> List[np.ndarray]:
    """The Q quantile fields [G, B, c_out] of the last `score_order`, downloaded."""
    return [self.handle.ens_order_quantile(q) for q in range(len(self.order or ()))]

  def score(self, truth=None, want_fields: bool = False) -> Tuple[EnsembleScores, Optional["EventScores"]]:
    """-> (raw `EnsembleScores`, `EventScores` or None).  `truth` [G, B, c_out] in the members' units, None: the truth
    already on the device; with a plan (or a feature plan, or a band plan) the store is first filled from the source's (members and truth,
    device to device) and `truth` [G, B, c_src] is the SOURCE's."""
    if self.plan is not None:
      if self.set_per_score:
        self._set_plan()
      self.handle.ens_derive(self.source, truth)
      truth = None
    if self.feature_plan is not None:
      if self.set_per_score:
        self._set_plan()
      self.handle.ens_feature(self.source, truth)
      truth = None
    if self.band_plan is not None:
      if self.set_per_score:
        self._set_plan()
      self.handle.ens_band(self.source, truth)
      truth = None
    sums, hist = self.handle.ens_score(truth, want_fields=want_fields)
    return EnsembleScores(sums, hist, self.n_members), self.score_events(None)
