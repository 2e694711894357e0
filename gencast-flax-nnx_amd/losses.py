"""Latitude- and pressure-level-weighted MSE on this package's `Dataset` (host side, NumPy only).

Mirrors common/losses.py:58-187: `weighted_mse_per_level`, `sum_per_variable_losses`,
`normalized_level_weights`, `normalized_latitude_weights` (same cases, same `ValueError`s), and adds
`loss_plan`: the same weighting as four flat arrays in the channel order of `datasets.channel_layout`,
which is what the device-side evaluation takes (`gc_loss_set_weights`, include/gencast_hip.h):

  per variable v   l_v[b] = sum over grid nodes i and the channels c of v of
                            node_weight[i] * channel_weight[c] * (prediction - target)[i, b, c] ** 2
  loss[b]          = sum_v group_weight[v] * l_v[b]

with node_weight = unit-mean latitude weight / number of grid nodes and channel_weight = level weight /
channels of the variable, so l_v is the reference's mean over (lat, lon, level, time).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Mapping, Optional, Tuple

import numpy as np

from . import datasets
from .datasets import Dataset, Variable

# gencast/gencast.py:259-278: every variable not named weighs 1.0
DEFAULT_PER_VARIABLE_WEIGHTS: Dict[str, float] = {
    "2m_temperature": 1.0,
    "10m_u_component_of_wind": 0.1,
    "10m_v_component_of_wind": 0.1,
    "mean_sea_level_pressure": 0.1,
}


def _coord(data, name: str) -> np.ndarray:
  coords = getattr(data, "coords", None)
  if coords is None:
    return np.asarray(data, dtype=np.float64)
  if name not in coords:
    raise ValueError(f"no {name!r} coordinate")
  return np.asarray(getattr(coords[name], "values", coords[name]), dtype=np.float64)


def _uniform_delta(vector: np.ndarray) -> float:
  diff = np.diff(vector)
  if not np.all(np.isclose(diff[0], diff)):
    raise ValueError(f"Vector {diff} is not uniformly spaced.")
  return float(diff[0])


def normalized_level_weights(data) -> np.ndarray:
  """Weights proportional to pressure: level / mean(level) (losses.py:99-102).  `data`: anything with a
  `coords['level']`, or the level values themselves."""
  level = _coord(data, "level")
  return level / level.mean()


def normalized_latitude_weights(data) -> np.ndarray:
  """Unit-mean weights proportional to grid-cell area (losses.py:105-187), for equispaced latitudes that
  either stop half a spacing short of the poles (weight cos(lat)) or include them (cos(lat) * sin(d/2), and
  sin(d/4)^2 for the two pole rows).  `data`: anything with a `coords['lat']`, or the latitudes in degrees."""
  lat = _coord(data, "lat")
  delta = abs(_uniform_delta(lat))
  if np.any(np.isclose(np.abs(lat), 90.0)):
    if not np.isclose(lat.max(), 90.0) or not np.isclose(lat.min(), -90.0):
      raise ValueError(f"Latitude vector {lat} does not start/end at +- 90 degrees.")
    weights = np.cos(np.deg2rad(lat)) * np.sin(np.deg2rad(delta / 2))
    weights[[0, -1]] = np.sin(np.deg2rad(delta / 4)) ** 2
  else:
    if not np.isclose(lat.max(), 90.0 - delta / 2) or not np.isclose(lat.min(), -90.0 + delta / 2):
      raise ValueError(f"Latitude vector {lat} does not start/end at +- (90 - delta_latitude/2) degrees.")
    weights = np.cos(np.deg2rad(lat))
  return weights / weights.mean()


def _along(weights: np.ndarray, var: Variable, dim: str) -> np.ndarray:
  if weights.shape != (var.sizes[dim],):
    raise ValueError(f"{dim!r} coordinate has {weights.shape[0]} values, the variable {var.sizes[dim]}")
  shape = [1] * len(var.dims)
  shape[var.dims.index(dim)] = -1
  return weights.reshape(shape)


def sum_per_variable_losses(per_variable_losses: Mapping[str, Variable], weights: Mapping[str, float]):
  """Weighted sum of per-variable losses (losses.py:79-96) -> (total, per_variable_losses)."""
  if not set(weights.keys()).issubset(set(per_variable_losses.keys())):
    raise ValueError("Passing a weight that does not correspond to any variable "
                     f"{set(weights.keys()) - set(per_variable_losses.keys())}")
  total = None
  for name, loss in per_variable_losses.items():
    term = np.asarray(getattr(loss, "data", loss)) * weights.get(name, 1)
    total = term if total is None else total + term
  return Variable(("batch",), np.asarray(total)), per_variable_losses


def weighted_mse_per_level(predictions, targets, per_variable_weights: Mapping[str, float]):
  """losses.py:58-76 -> (loss, diagnostics): `loss` a Variable with dims ('batch',), `diagnostics` a Dataset of the
  unweighted per-variable means, each ('batch',).  Evaluated in float64."""
  predictions, targets = datasets.as_dataset(predictions), datasets.as_dataset(targets)
  if set(predictions.keys()) != set(targets.keys()):
    raise ValueError("predictions and targets must hold the same variables")
  per_var: Dict[str, Variable] = {}
  for name in targets.keys():
    t, p = targets[name], predictions[name]
    if p.dims != t.dims:
      raise ValueError(f"{name}: prediction dims {p.dims} differ from target dims {t.dims}")
    if "batch" not in t.dims:
      raise ValueError(f"{name}: no 'batch' dimension")
    se = (np.asarray(p.data, dtype=np.float64) - np.asarray(t.data, dtype=np.float64)) ** 2
    if "lat" in t.dims:
      se = se * _along(normalized_latitude_weights(targets), t, "lat")
    if "level" in t.dims:
      se = se * _along(normalized_level_weights(targets), t, "level")
    axes = tuple(i for i, d in enumerate(t.dims) if d != "batch")
    per_var[name] = Variable(("batch",), se.mean(axis=axes))
  total, _ = sum_per_variable_losses(per_var, per_variable_weights)
  return total, Dataset(per_var)


@dataclasses.dataclass
class LossPlan:
  """`weighted_mse_per_level` as flat arrays over [grid node, batch, channel] (node = lat_i * n_lon + lon_j)."""
  node_weight: np.ndarray       # [G]      float32, sums to 1
  channel_weight: np.ndarray    # [c_out]  float32, sums to 1 inside every group
  channel_group: np.ndarray     # [c_out]  int32
  group_weight: np.ndarray      # [groups] float32
  names: Tuple[str, ...]        # group -> variable name (sorted)

  def evaluate(self, squared_error: np.ndarray):
    """Host evaluation in float64: `squared_error` [G, B, c_out] -> (loss [B], per_group [B, groups])."""
    se = np.asarray(squared_error, dtype=np.float64)
    cols = np.einsum("i,ibc->bc", self.node_weight.astype(np.float64), se) * self.channel_weight.astype(np.float64)
    per_group = np.zeros((se.shape[1], len(self.names)))
    for c, g in enumerate(self.channel_group):
      per_group[:, g] += cols[:, c]
    return per_group @ self.group_weight.astype(np.float64), per_group


def loss_plan(targets, per_variable_weights: Optional[Mapping[str, float]] = None, *, dtype=np.float32) -> LossPlan:
  """The flat form of `weighted_mse_per_level(., targets, per_variable_weights)` for targets stacked the way the
  denoiser stacks them (sorted names; every dim other than batch / lat / lon folded into channels in the
  variable's own order).  One group per variable.  `per_variable_weights=None`: the reference's table."""
  targets = datasets.as_dataset(targets)
  weights = DEFAULT_PER_VARIABLE_WEIGHTS if per_variable_weights is None else per_variable_weights
  names = tuple(sorted(targets.keys()))
  if per_variable_weights is not None and not set(weights.keys()).issubset(names):
    raise ValueError(f"Passing a weight that does not correspond to any variable {set(weights.keys()) - set(names)}")
  sizes = targets.sizes
  if "lat" not in sizes or "lon" not in sizes:
    raise ValueError("targets must have 'lat' and 'lon' dimensions")
  node = np.repeat(normalized_latitude_weights(targets), sizes["lon"]) / (sizes["lat"] * sizes["lon"])
  chan_w, chan_g = [], []
  for g, (name, _, n) in enumerate(datasets.channel_layout(targets)):
    var = targets[name]
    if not all(d in var.dims for d in datasets.PRESERVED):
      raise ValueError(f"{name}: target variables need batch, lat and lon dimensions, found {var.dims}")
    stack = [d for d in var.dims if d not in datasets.PRESERVED]
    w = np.ones([var.sizes[d] for d in stack])
    if "level" in stack:
      w = w * _along(normalized_level_weights(targets), Variable(tuple(stack), w), "level")
    chan_w.append(w.reshape(-1) / n)
    chan_g.append(np.full(n, g, dtype=np.int32))
  return LossPlan(node.astype(dtype), np.concatenate(chan_w).astype(dtype), np.concatenate(chan_g),
                  np.asarray([weights.get(name, 1.0) for name in names], dtype=dtype), names)
