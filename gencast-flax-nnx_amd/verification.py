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
"""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

from . import datasets, losses


class EnsembleScores:
  """Raw sums [B, c_out, 6] float64, rank histogram [B, c_out, M + 1] uint64 and the member count M."""

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
  def merge(parts: Sequence["EnsembleScores"]) -> "EnsembleScores":
    """Scores over the union of what the parts covered (other nodes, other dates): raw sums and counts add."""
    parts = list(parts)
    if not parts:
      raise ValueError("merge: nothing to merge")
    first = parts[0]
    for p in parts[1:]:
      if p.n_members != first.n_members or p.sums.shape != first.sums.shape:
        raise ValueError("merge: the parts differ in members or shape")
    sums = first.sums.copy()
    hist = first.rank_histogram.copy()
    for p in parts[1:]:
      sums += p.sums
      hist += p.rank_histogram
    return EnsembleScores(sums, hist, first.n_members)

  def per_variable(self, template) -> Dict[str, Dict[str, np.ndarray]]:
    """{score: {variable: [batch, channels of the variable]}} in the channel order of `datasets.channel_layout`
    (for a variable with levels and one time step: (batch, level))."""
    layout = datasets.channel_layout(datasets.as_dataset(template))
    if sum(n for _, _, n in layout) != self.sums.shape[1]:
      raise ValueError(f"template has {sum(n for _, _, n in layout)} channels, the scores {self.sums.shape[1]}")
    out: Dict[str, Dict[str, np.ndarray]] = {}
    for score in ("rmse", "spread", "spread_skill_ratio", "crps", "crps_ensemble", "bias", "valid_weight"):
      values = getattr(self, score)
      out[score] = {name: values[:, off:off + n] for name, off, n in layout}
    out["rank_histogram"] = {name: self.rank_histogram[:, off:off + n] for name, off, n in layout}
    return out

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
