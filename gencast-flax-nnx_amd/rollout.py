"""Autoregressive rollout around `GenCast.full_sampling`.

Three layers, each mirroring the reference at the array level:

* `normalize` / `unnormalize` / `InputsAndResiduals` -- common/normalization.py:31-238:
  inputs and forcings are normalised with per-variable (per-level) `scales`/`locations`;
  target variables that are also inputs are predicted as residuals to the last input frame,
  normalised with `residual_scales`; everything else with the plain statistics.
* `compose_next_frame` / `autoregressive_rollout` -- training/train_helpers.py:485-622
  (forecast-time branch): the context drops its oldest frame and gets a new one made of the
  predicted target variables, this step's forcings, and the input-only variables carried from
  the last context frame.
* `DeviceRollout` -- the same loop with the conditioning kept in HBM: in NORMALISED space the
  whole update (un-normalise, add last input, re-normalise, roll the time axis) is one affine
  per conditioning channel, which `gc_rollout_advance` applies on the device
  (include/gencast_hip.h).  Per step only the 4 progress forcings go up and the sample comes
  down; Python never re-packs the 11-MB conditioning.
"""
from __future__ import annotations

import time as _time
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np

from . import config as cfg
from . import datasets, spectra as _spectra, verification
from .datasets import Dataset, Variable
from .denoiser import Denoiser


# ---------------------------------------------------------------------------------------------
# small Dataset helpers (xarray's isel / concat on the time axis)
# ---------------------------------------------------------------------------------------------
def isel_time(ds: Dataset, sl) -> Dataset:
  """`ds.isel(time=sl)`: variables without a time axis pass through; an int drops the axis."""
  out: Dict[str, Variable] = {}
  for k, v in ds.items():
    if "time" not in v.dims:
      out[k] = v
      continue
    ax = v.dims.index("time")
    idx = [slice(None)] * len(v.dims)
    idx[ax] = sl
    data = v.data[tuple(idx)]
    dims = v.dims if isinstance(sl, slice) else tuple(d for d in v.dims if d != "time")
    out[k] = Variable(dims, data)
  coords = dict(ds.coords)
  if "time" in coords and coords["time"].ndim == 1:
    if isinstance(sl, slice):
      coords["time"] = coords["time"][sl]
    else:
      coords.pop("time")
  return Dataset(out, coords)


def concat_time(parts: Sequence[Dataset]) -> Dataset:
  """`xr.concat(parts, dim="time")` for datasets with the same variables."""
  first = parts[0]
  out: Dict[str, Variable] = {}
  for k, v in first.items():
    if "time" not in v.dims:
      out[k] = v
      continue
    ax = v.dims.index("time")
    out[k] = Variable(v.dims, np.concatenate([p[k].data for p in parts], axis=ax))
  coords = dict(first.coords)
  if all("time" in p.coords for p in parts):
    coords["time"] = np.concatenate([np.atleast_1d(p.coords["time"]) for p in parts])
  return Dataset(out, coords)


def _stat_like(stat: Variable, like: Variable) -> np.ndarray:
  """Broadcasts a statistic (dims a subset of `like`'s, e.g. () or ('level',)) to `like`."""
  shape = [1] * len(like.dims)
  for d, n in zip(stat.dims, np.shape(stat.data)):
    if d not in like.dims:
      raise ValueError(f"statistic dimension {d!r} is not a dimension of the variable {like.dims}")
    shape[like.dims.index(d)] = n
  order = sorted(range(len(stat.dims)), key=lambda i: like.dims.index(stat.dims[i]))
  data = np.transpose(np.asarray(stat.data), order) if stat.dims else np.asarray(stat.data)
  return data.reshape(shape).astype(like.data.dtype)


def normalize(values: Dataset, scales: Dataset, locations: Optional[Dataset]) -> Dataset:
  """common/normalization.py:31-50: (x - location) / scale, per variable, where statistics exist."""
  out = {}
  for name, v in values.items():
    data = v.data
    if locations is not None and name in locations:
      data = data - _stat_like(locations[name], v)
    if name in scales:
      data = data / _stat_like(scales[name], v)
    out[name] = Variable(v.dims, data)
  return Dataset(out, values.coords)


def unnormalize(values: Dataset, scales: Dataset, locations: Optional[Dataset]) -> Dataset:
  """common/normalization.py:53-71: x * scale + location."""
  out = {}
  for name, v in values.items():
    data = v.data
    if name in scales:
      data = data * _stat_like(scales[name], v)
    if locations is not None and name in locations:
      data = data + _stat_like(locations[name], v)
    out[name] = Variable(v.dims, data)
  return Dataset(out, values.coords)


class InputsAndResiduals:
  """common/normalization.py:74-238 (sampling side): normalised inputs, normalised residual targets."""

  def __init__(self, predictor, stddev_by_level: Dataset, mean_by_level: Dataset,
               diffs_stddev_by_level: Dataset):
    self.predictor = predictor
    self._scales = stddev_by_level
    self._locations = mean_by_level
    self._residual_scales = diffs_stddev_by_level
    self._residual_locations = None

  def _unnormalize_prediction_and_add_input(self, inputs: Dataset, name: str, pred: Variable) -> Variable:
    if pred.sizes.get("time") != 1:
      raise ValueError("normalization.InputsAndResiduals only supports predicting a single timestep.")
    one = Dataset({name: pred})
    if name in inputs:                                   # residual prediction (:110-118)
      out = unnormalize(one, self._residual_scales, self._residual_locations)[name]
      last = isel_time(Dataset({name: inputs[name]}), -1)[name]
      return Variable(out.dims, out.data + _broadcast_last(last, out))
    return unnormalize(one, self._scales, self._locations)[name]

  def _subtract_input_and_normalize_target(self, inputs: Dataset, name: str, target: Variable) -> Variable:
    if target.sizes.get("time") != 1:
      raise ValueError("normalization.InputsAndResiduals only supports wrapping predictors"
                       "that predict a single timestep.")
    if name in inputs:
      last = isel_time(Dataset({name: inputs[name]}), -1)[name]
      resid = Variable(target.dims, target.data - _broadcast_last(last, target))
      return normalize(Dataset({name: resid}), self._residual_scales, self._residual_locations)[name]
    return normalize(Dataset({name: target}), self._scales, self._locations)[name]

  def _wrap(self, fn_name, inputs, targets_template, forcings, **kwargs):
    given = (targets_template, inputs, forcings)            # xarray in -> xarray out (datasets.like_inputs)
    inputs = datasets.as_dataset(inputs)
    forcings = datasets.as_dataset(forcings)
    template = datasets.as_dataset(targets_template)
    norm_inputs = normalize(inputs, self._scales, self._locations)
    norm_forcings = normalize(forcings, self._scales, self._locations)
    norm_template = Dataset({k: self._subtract_input_and_normalize_target(inputs, k, v)
                             for k, v in template.items()}, template.coords)
    norm_pred = datasets.as_dataset(getattr(self.predictor, fn_name)(norm_inputs, norm_template, forcings=norm_forcings, **kwargs))
    return datasets.like_inputs(Dataset({k: self._unnormalize_prediction_and_add_input(inputs, k, v)
                                         for k, v in norm_pred.items()}, norm_pred.coords), *given)

  def full_sampling(self, inputs, targets_template, forcings, **kwargs):
    """common/normalization.py:200-238."""
    return self._wrap("full_sampling", inputs, targets_template, forcings, **kwargs)

  def _normalized_loss_args(self, inputs, targets, forcings):
    inputs, targets, forcings = (datasets.as_dataset(x) for x in (inputs, targets, forcings))
    norm_targets = Dataset({k: self._subtract_input_and_normalize_target(inputs, k, v) for k, v in targets.items()},
                           targets.coords)
    return (inputs, normalize(inputs, self._scales, self._locations), norm_targets,
            normalize(forcings, self._scales, self._locations))

  def denoising_loss(self, inputs, targets, forcings=None, **kwargs):
    """common/normalization.py:163-176 on the forward-only objective: the loss of the wrapped predictor on normalised
    inputs and forcings and residual-normalised targets."""
    _, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    return datasets.loss_like_inputs(*self.predictor.denoising_loss(ni, nt, forcings=nf, **kwargs), targets, inputs, forcings)

  def denoising_loss_and_predictions(self, inputs, targets, forcings=None, **kwargs):
    """common/normalization.py:178-197: the same loss, with the predictions un-normalised (residuals added back)."""
    given = (targets, inputs, forcings)
    raw, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    loss, norm_pred = self.predictor.denoising_loss_and_predictions(ni, nt, forcings=nf, **kwargs)
    norm_pred = datasets.as_dataset(norm_pred)
    preds = Dataset({k: self._unnormalize_prediction_and_add_input(raw, k, v) for k, v in norm_pred.items()}, norm_pred.coords)
    return datasets.loss_like_inputs(*loss, *given), datasets.like_inputs(preds, *given)

  def _target_scale(self, raw_inputs: Dataset, targets) -> np.ndarray:
    """Per target channel, the a of the member-to-physical map x -> a x + b: the residual scale of a variable that is also
    an input, else its plain scale."""
    tds = datasets.as_dataset(targets)
    return np.concatenate([_per_channel_stat(self._residual_scales if name in raw_inputs else self._scales, name, tds[name], 1.0)
                           for name, _, _ in datasets.channel_layout(tds)])


  def ensemble_scores(self, inputs, targets, forcings=None, **kwargs):
    """`ensemble_scores` of the wrapped predictor on normalised inputs and forcings and residual-normalised targets,
    returned in physical units: the member-to-physical map is x -> a x + b per channel (a: the residual scale of a
    variable that is also an input, else its plain scale; b cancels in every score), so the raw sums are rescaled
    (`EnsembleScores.scaled`), nothing is recomputed.  With `fields=True` the mean is un-normalised like a
    prediction (last input frame added back for residual variables) and the variance is multiplied by a^2."""
    given = (targets, inputs, forcings)
    raw, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    scale = self._target_scale(raw, targets)
    out = self.predictor.ensemble_scores(ni, nt, forcings=nf, **kwargs)
    if not isinstance(out, tuple):
      return out.scaled(scale)
    scores, mean, var = out[0], datasets.as_dataset(out[1]), datasets.as_dataset(out[2])
    mean = Dataset({k: self._unnormalize_prediction_and_add_input(raw, k, v) for k, v in mean.items()}, mean.coords)
    squared = {True: self._residual_scales.map(np.square), False: self._scales.map(np.square)}
    var = Dataset({k: unnormalize(Dataset({k: v}), squared[k in raw], None)[k] for k, v in var.items()}, var.coords)
    return scores.scaled(scale), datasets.like_inputs(mean, *given), datasets.like_inputs(var, *given)


  def ensemble_order(self, inputs, targets, forcings=None, **kwargs):
    """`ensemble_order` of the wrapped predictor on normalised inputs and forcings and residual-normalised targets, in
    physical units: the bin and pinball sums are rescaled as `ensemble_scores` rescales its sums (`OrderScores.scaled`).
    With `quantile_fields=True` every field is un-normalised like a prediction (last input frame added back for residual
    variables).  That is valid because the member-to-physical map x -> a x + b(point) has a > 0 and a b that is the same
    for all members of a point: it is monotone, so it keeps the order of the members, and affine, so it commutes with the
    linear interpolation between two of them -- the quantile of the mapped members is the mapped quantile."""
    given = (targets, inputs, forcings)
    raw, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    scale = self._target_scale(raw, targets)
    out = self.predictor.ensemble_order(ni, nt, forcings=nf, **kwargs)
    if not isinstance(out, tuple):
      return out.scaled(scale)
    fields = []
    for f in out[1]:
      f = datasets.as_dataset(f)
      fields.append(datasets.like_inputs(Dataset({k: self._unnormalize_prediction_and_add_input(raw, k, v)
                                                  for k, v in f.items()}, f.coords), *given))
    return out[0].scaled(scale), fields

  def ensemble_multivariate(self, inputs, targets, forcings=None, **kwargs):
    """`ensemble_multivariate` of the wrapped predictor on normalised inputs and forcings and residual-normalised targets.
    The variogram sums are scaled back to physical units (`VariogramScores.scaled`: the location drops out of every
    difference).  The energy score STAYS in normalised residual units: a norm over several variables has a meaning only
    where they are comparable, and there is no single factor that would take it back."""
    raw, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    scale = self._target_scale(raw, targets)
    en, vg = self.predictor.ensemble_multivariate(ni, nt, forcings=nf, **kwargs)
    return en, None if vg is None else vg.scaled(scale)

  def ensemble_climatology(self, inputs, targets, forcings=None, *, climatology, **kwargs):
    """`ensemble_climatology` of the wrapped predictor on normalised inputs and forcings and residual-normalised targets.
    Every climatological sample (physical units) goes through the SAME map as the targets
    (`_subtract_input_and_normalize_target`: for a residual variable the last input frame is subtracted, per batch member),
    so members, samples and truth differ from their physical values by one affine map x -> a x + b(point) per channel; the
    raw sums are scaled back (`ClimatologyScores.scaled`: b drops out of every term), nothing is recomputed."""
    raw, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    scale = self._target_scale(raw, targets)
    nclim = []
    for c in climatology:
      c = datasets.as_dataset(c)
      nclim.append(Dataset({k: self._subtract_input_and_normalize_target(raw, k, v) for k, v in c.items()}, c.coords))
    return self.predictor.ensemble_climatology(ni, nt, forcings=nf, climatology=nclim, **kwargs).scaled(scale)

  def ensemble_efi(self, inputs, targets, forcings=None, *, climatology, **kwargs):
    """`ensemble_efi` of the wrapped predictor on normalised inputs and forcings and residual-normalised targets, passed
    through as it is: every sample goes through the SAME map as the targets (as in `ensemble_climatology`), that map is
    increasing per point, and ranks -- hence the index, its fields and its tables -- do not change under it.  With
    `targets=None` the first sample stands in where the shape of the targets is needed."""
    climatology = [datasets.as_dataset(c) for c in climatology]
    raw, ni, nt, nf = self._normalized_loss_args(inputs, climatology[0] if targets is None else targets, forcings)
    nclim = [Dataset({k: self._subtract_input_and_normalize_target(raw, k, v) for k, v in c.items()}, c.coords)
             for c in climatology]
    return self.predictor.ensemble_efi(ni, None if targets is None else nt, forcings=nf, climatology=nclim, **kwargs)

  def ensemble_events(self, inputs, targets, forcings=None, *, spec, **kwargs):
    """`ensemble_events` of the wrapped predictor on normalised inputs and forcings and residual-normalised targets.
    The thresholds of `spec` (physical units) go through the SAME map as the targets
    (`_subtract_input_and_normalize_target`: for a residual variable the last input frame is subtracted, per batch
    member -- which is why thresholds are full fields).  Scales are positive, so no direction flips; the tables are
    integers and carry no unit."""
    raw, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    nspec = spec.mapped(datasets.as_dataset(targets), lambda name, v: self._subtract_input_and_normalize_target(raw, name, v))
    return self.predictor.ensemble_events(ni, nt, forcings=nf, spec=nspec, **kwargs)

  def ensemble_tails(self, inputs, targets, forcings=None, *, spec, **kwargs):
    """`ensemble_tails` of the wrapped predictor on normalised inputs and forcings and residual-normalised targets.  The
    thresholds of `spec` (physical units) go through the SAME map as the targets, exactly as in `ensemble_events`; the map
    x -> a x + b(point) has a > 0, so clamping commutes with it and no tail flips, and the sums are scaled back to physical
    units (`TailScores.scaled`: b drops out of every difference)."""
    raw, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    scale = self._target_scale(raw, targets)
    nspec = spec.mapped(datasets.as_dataset(targets), lambda name, v: self._subtract_input_and_normalize_target(raw, name, v))
    return self.predictor.ensemble_tails(ni, nt, forcings=nf, spec=nspec, **kwargs).scaled(scale)

  def ensemble_maps(self, inputs, targets, forcings=None, *, spec, events=None, **kwargs):
    """`ensemble_maps` of the wrapped predictor on normalised inputs and forcings and residual-normalised targets, returned in
    physical units: the planes are rescaled per selected channel (`ScoreMaps.scaled`: b drops out of every term), nothing is
    recomputed.  The thresholds of `events` (physical units) go through the SAME map as the targets, as in `ensemble_events`;
    the event planes are integers and carry no unit."""
    raw, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    scale = self._target_scale(raw, targets)[spec.channels(targets)]
    nev = None if events is None else events.mapped(datasets.as_dataset(targets),
                                                     lambda name, v: self._subtract_input_and_normalize_target(raw, name, v))
    out = self.predictor.ensemble_maps(ni, nt, forcings=nf, spec=spec, events=nev, **kwargs)
    if not isinstance(out, tuple):
      return out.scaled(scale)
    return out[0].scaled(scale), out[1]

  def ensemble_regions(self, inputs, targets, forcings=None, **kwargs):
    """`ensemble_regions` of the wrapped predictor on normalised inputs and forcings and residual-normalised targets, returned
    in physical units: every region's raw sums are rescaled as in `ensemble_scores` (`RegionScores.scaled`)."""
    raw, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    scale = self._target_scale(raw, targets)
    return self.predictor.ensemble_regions(ni, nt, forcings=nf, **kwargs).scaled(scale)

  def ensemble_rollout(self, inputs, targets, forcings, horizon, num_members, **kwargs):
    """`ensemble_rollout` of the wrapped predictor with this wrapper as its normalisation (`EnsembleRollout(norm=self)`):
    the inputs go in RAW -- the device rollout normalises them itself and folds the residual arithmetic into its
    per-channel context update -- and scores, spectra and fields come back in physical units."""
    return self.predictor.ensemble_rollout(inputs, targets, forcings, horizon, num_members, norm=self, **kwargs)

  def ensemble_features(self, inputs, targets, forcings=None, *, num_members, spec, **kwargs):
    """The features of `spec` (`verification.FeatureSpec`, thresholds and depths in physical units) in the members and in
    `targets`: `verification.FeatureScores`.  A single-step sample is a normalised RESIDUAL here, in which a pressure
    minimum is no minimum, so the detector runs on the member STATES of a one-step `ensemble_rollout` under this
    normalisation (`EnsembleRollout.run(features=...)`): the members hold (x - l) / s of the field itself, a monotone map per
    channel, and thresholds and depths take it."""
    res = self.ensemble_rollout(inputs, targets, forcings, 1, num_members, features={"features": spec}, **kwargs)
    part = res.features["features"]
    members, of_truth = verification.split_centres(part.centres[0])
    return verification.FeatureScores(part.scores[0], part.events[0], members, of_truth, part.strike_probability[0], part.template)

  def ensemble_spectra(self, inputs, targets, forcings=None, **kwargs):
    """`ensemble_spectra` of the wrapped predictor on normalised inputs and forcings and residual-normalised targets,
    in physical units: every power is multiplied by a^2 per channel (`EnsembleSpectra.scaled`; a: the residual scale of
    a variable that is also an input, else its plain scale).  This is the spectrum of the predicted INCREMENT without
    its location offset (for a residual variable the last input frame, else the mean): adding a field back is not a
    rescaling of sums.  The error and spread spectra do not depend on that offset.  With `scores=True` the scores are
    rescaled as `ensemble_scores` does."""
    raw, ni, nt, nf = self._normalized_loss_args(inputs, targets, forcings)
    scale = self._target_scale(raw, targets)
    out = self.predictor.ensemble_spectra(ni, nt, forcings=nf, **kwargs)
    if not isinstance(out, tuple):
      return out.scaled(scale)
    return tuple(o.scaled(scale) for o in out)


def _broadcast_last(last: Variable, like: Variable) -> np.ndarray:
  """The last input frame (no time axis) broadcast against a time=1 variable."""
  shape = [1] * len(like.dims)
  for d, n in zip(last.dims, np.shape(last.data)):
    shape[like.dims.index(d)] = n
  order = sorted(range(len(last.dims)), key=lambda i: like.dims.index(last.dims[i]))
  return np.transpose(last.data, order).reshape(shape)


# ---------------------------------------------------------------------------------------------
# host-composed autoregressive rollout (training/train_helpers.py:485-622)
# ---------------------------------------------------------------------------------------------
def compose_next_frame(target_like: Dataset, forcings_like: Dataset, prev_context: Dataset,
                       task: cfg.TaskConfig = cfg.TASK) -> Dataset:
  """One full input frame (time=1): predicted targets + this step's forcings + carried input-only vars."""
  target_vars, forcing_vars = set(task.target_variables), set(task.forcing_variables)
  input_only = set(task.input_variables) - target_vars - forcing_vars
  dv: Dict[str, Variable] = {}
  for v in target_vars:
    if v in target_like:
      dv[v] = target_like[v]
  for v in forcing_vars:
    if v in forcings_like:
      dv[v] = forcings_like[v]
  for v in input_only:
    if v in prev_context:
      var = prev_context[v]
      if "time" in var.dims:
        ax = var.dims.index("time")
        dv[v] = Variable(var.dims, np.take(var.data, [-1], axis=ax))
      else:
        dv[v] = var
  coords = dict(prev_context.coords)
  coords.update(target_like.coords)
  return Dataset(dv, coords)


def autoregressive_rollout(model, inputs: Dataset, targets: Dataset, forcings: Dataset, horizon: int, *,
                           context_steps: int = 2, task: cfg.TaskConfig = cfg.TASK,
                           init_noise: Optional[Sequence[np.ndarray]] = None):
  """Forecast-time AR rollout.  Returns (mse vs `targets`, predictions [time=horizon], targets[:horizon]).

  `targets` supplies the per-step templates (`* 0`) and the MSE reference exactly as the reference
  does (train_helpers.py:596-640); `init_noise[k]` optionally fixes step k's initial noise.
  """
  given = (targets, inputs, forcings)
  inputs, targets, forcings = (datasets.as_dataset(x) for x in (inputs, targets, forcings))
  if inputs.sizes.get("time", 0) < context_steps:
    raise ValueError(f"inputs carry {inputs.sizes.get('time', 0)} time steps (need at least {context_steps})")
  context = isel_time(inputs, slice(-context_steps, None))
  preds: List[Dataset] = []
  for k in range(horizon):
    template = isel_time(targets, slice(k, k + 1)).map(np.zeros_like)
    forc_k = isel_time(forcings, slice(k, k + 1))
    kw = {} if init_noise is None else {"init_noise": init_noise[k]}
    pred = datasets.as_dataset(model.full_sampling(inputs=context, targets_template=template, forcings=forc_k, **kw))
    preds.append(pred)
    tail = isel_time(context, slice(1, None))
    frame = compose_next_frame(pred, forc_k, context, task)
    context = concat_time([tail, Dataset({n: frame[n] for n in tail.keys()}, frame.coords)])
  rollout = concat_time(preds)
  future = isel_time(targets, slice(0, horizon))
  se, cnt = 0.0, 0
  for name, v in rollout.items():
    d = v.data.astype(np.float64) - future[name].data.astype(np.float64)
    se += float((d * d).sum())
    cnt += d.size
  future_x = isel_time(datasets.as_dataset(given[0]), slice(0, horizon))
  if datasets.is_xarray(given[0]):                          # predictions on the targets' time axis, like the harness's xr.concat
    return se / max(cnt, 1), datasets.to_xarray(rollout, given[0].isel(time=slice(0, horizon))), given[0].isel(time=slice(0, horizon))
  return se / max(cnt, 1), datasets.like_inputs(rollout, None, *given[1:]), future_x


# ---------------------------------------------------------------------------------------------
# device-resident rollout
# ---------------------------------------------------------------------------------------------
def _time_blocks(ds: Dataset):
  """For every variable in stacking order: (name, first_channel, n_time, channels_per_time)."""
  out = []
  for name, off, n in datasets.channel_layout(ds):
    v = ds[name]
    rest = [d for d in v.dims if d not in datasets.PRESERVED]
    if "time" in rest:
      if rest[0] != "time":
        raise ValueError(f"{name}: the time axis must come before {rest[1:]} for the device rollout")
      nt = v.sizes["time"]
    else:
      nt = 1
    out.append((name, off, nt, n // nt))
  return out


def _per_channel_stat(stat: Optional[Dataset], name: str, var: Variable, default: float) -> np.ndarray:
  """Statistic of one time slice of `var`, flattened in channel order (level-major remainder)."""
  rest = [d for d in var.dims if d not in datasets.PRESERVED and d != "time"]
  n = int(np.prod([var.sizes[d] for d in rest])) if rest else 1
  if stat is None or name not in stat:
    return np.full(n, default, np.float64)
  s = stat[name]
  shape = [var.sizes[d] for d in rest]
  full = np.ones(shape, np.float64)
  view = [1] * len(rest)
  for d, m in zip(s.dims, np.shape(s.data)):
    view[rest.index(d)] = m
  order = sorted(range(len(s.dims)), key=lambda i: rest.index(s.dims[i]))
  data = np.transpose(np.asarray(s.data, np.float64), order) if s.dims else np.asarray(s.data, np.float64)
  return (full * data.reshape(view)).reshape(-1)


def build_rollout_plan(inputs: Dataset, forcings: Dataset, template: Dataset, task: cfg.TaskConfig,
                       norm: Optional[InputsAndResiduals]):
  """Plan arrays for `gc_rollout_plan` + the order of the forcing columns `advance` expects.

  In normalised space, with s/l the input statistics and rs/rl the residual ones (normalization.py:100-121):
    x_new = pred * rs + rl + x_last,  xn = (x - l) / s   =>   xn_new = xn_last + (rs / s) * pred + rl / s.
  Without a normalisation wrapper the prediction is the new frame itself (a = 1, no carry).
  """
  n_inputs = sum(n for _, _, n in datasets.channel_layout(inputs))
  merged = forcings.assign(datasets.zeros_like(template))
  c_in = n_inputs + sum(n for _, _, n in datasets.channel_layout(merged))
  kind = np.zeros(c_in, np.int32)
  src = np.zeros(c_in, np.int32)
  sidx = np.zeros(c_in, np.int32)
  a = np.zeros(c_in, np.float32)
  b = np.zeros(c_in, np.float32)
  tgt_off = {name: off for name, off, _ in datasets.channel_layout(template)}
  forc_off = {name: n_inputs + off for name, off, _ in datasets.channel_layout(merged)}
  target_vars, forcing_vars = set(task.target_variables), set(task.forcing_variables)

  for name, off, nt, per in _time_blocks(inputs):
    if nt < 2:
      continue                                            # no time axis (or one frame): carried unchanged
    for t in range(nt - 1):                               # older slots take the next-newer slot's values
      c = off + t * per + np.arange(per)
      kind[c] = 1
      src[c] = c + per
    last = off + (nt - 1) * per + np.arange(per)
    if name in target_vars and name in template:
      var = inputs[name]
      if norm is not None:
        s = _per_channel_stat(norm._scales, name, var, 1.0)
        rs = _per_channel_stat(norm._residual_scales, name, var, 1.0)
        rl = _per_channel_stat(norm._residual_locations, name, var, 0.0)
        kind[last] = 2
        src[last] = last
        a[last] = (rs / s).astype(np.float32)
        b[last] = (rl / s).astype(np.float32)
      else:
        kind[last] = 4
        a[last] = 1.0
      sidx[last] = tgt_off[name] + np.arange(per)
    elif name in forcing_vars and name in forcings:
      kind[last] = 1                                      # this step's forcing becomes the newest input frame
      src[last] = forc_off[name] + np.arange(per)
    # input-only variables: newest slot keeps its value (carried forward)

  forcing_cols = []                                       # (name, channel offset in the NEXT forcings array)
  nf = 0
  for name, off, n in datasets.channel_layout(merged):
    c = n_inputs + off + np.arange(n)
    if name in forcings and name not in template:
      kind[c] = 3
      sidx[c] = nf + np.arange(n)
      forcing_cols.append((name, nf, n))
      nf += n
    # noisy-target slots are rewritten by the sampler at every denoiser call: left as they are
  return dict(kind=kind, src=src, sidx=sidx, a=a, b=b, n_forcing=nf), forcing_cols


def _on_time_axis(parts: Sequence[Dataset], given, horizon: int):
  """`parts` joined on the targets' time axis, like the harness's xr.concat; `given` = (targets, inputs, forcings) as passed."""
  out = concat_time(parts)
  if datasets.is_xarray(given[0]):
    return datasets.to_xarray(out, given[0].isel(time=slice(0, horizon)))
  return datasets.like_inputs(out, None, *given[1:])


class DeviceRollout:
  """AR rollout with the conditioning resident in HBM (one `gc_rollout_advance` per step)."""

  def __init__(self, model, norm: Optional[InputsAndResiduals] = None, task: cfg.TaskConfig = cfg.TASK,
               device_noise: bool = False):
    """`device_noise`: draw every step's initial state on the GPU (`gc_noise_draw`) instead of synthesising
    it on the host and uploading 3.4 MB per step."""
    self.model = model                                    # a GenCast (its sampler drives the native handle)
    self.norm = norm
    self.task = task
    self.device_noise = device_noise
    self.last_step_ms: List[float] = []

  def _forcing_rows(self, forc_k: Dataset, forcing_cols, sizes, grid_shape) -> np.ndarray:
    if self.norm is not None:
      forc_k = normalize(forc_k, self.norm._scales, self.norm._locations)
    cols = []
    for name, _, _ in forcing_cols:
      cols.append(datasets.variable_to_stacked(forc_k[name], sizes))
    st = np.concatenate(cols, axis=-1)                    # (batch, lat, lon, nf)
    a = np.transpose(st, (1, 2, 0, 3))
    return np.ascontiguousarray(a.reshape((grid_shape[0] * grid_shape[1],) + a.shape[2:]), np.float32)

  def run(self, inputs: Dataset, targets: Dataset, forcings: Dataset, horizon: int, *,
          context_steps: int = 2, init_noise: Optional[Sequence[np.ndarray]] = None, rngs=0):
    """Returns the predictions (physical units, time = horizon) like `autoregressive_rollout`."""
    given = (targets, inputs, forcings)
    inputs, targets, forcings = (datasets.as_dataset(x) for x in (inputs, targets, forcings))
    context = isel_time(inputs, slice(-context_steps, None))
    template0 = isel_time(targets, slice(0, 1)).map(np.zeros_like)
    forc0 = isel_time(forcings, slice(0, 1))
    sampler = self.model._sampler
    den: Denoiser = self.model.denoiser
    if self.norm is not None:
      n_in = normalize(context, self.norm._scales, self.norm._locations)
      n_fo = normalize(forc0, self.norm._scales, self.norm._locations)
    else:
      n_in, n_fo = context, forc0
    cond, grid_shape, slots = den.init_for(n_in, template0, n_fo)
    native = den.native
    native.set_noisy_slots(slots)
    plan, forcing_cols = build_rollout_plan(context, forc0, template0, self.task, self.norm)
    native.rollout_plan(**plan)
    native.upload_cond(cond)
    sizes = dict(forc0.sizes)
    sizes.update(context.sizes)
    gen = rngs if isinstance(rngs, np.random.Generator) else np.random.default_rng(rngs)
    sigmas = np.asarray(sampler.noise_levels, np.float32)
    shape = (cond.shape[0], cond.shape[1], den.dims.c_out)
    last_phys = {k: isel_time(Dataset({k: context[k]}), -1)[k] for k in template0.keys() if k in context}
    preds: List[Dataset] = []
    self.last_step_ms = []

    def finish(k, out):
      """Host post-processing of step k's sample: unpack, un-normalise, add the last physical frame."""
      template = isel_time(targets, slice(k, k + 1)).map(np.zeros_like)
      norm_pred = Denoiser.unpack_outputs(out, grid_shape, template)
      if self.norm is not None:
        dv = {}
        for name, v in norm_pred.items():
          one = Dataset({name: v})
          if name in last_phys:
            u = unnormalize(one, self.norm._residual_scales, self.norm._residual_locations)[name]
            dv[name] = Variable(u.dims, u.data + _broadcast_last(last_phys[name], u))
          else:
            dv[name] = unnormalize(one, self.norm._scales, self.norm._locations)[name]
        pred = Dataset(dv, norm_pred.coords)
      else:
        pred = norm_pred
      for name in last_phys:
        last_phys[name] = isel_time(Dataset({name: pred[name]}), -1)[name]
      preds.append(pred)

    on_device = self.device_noise and init_noise is None
    churn = getattr(sampler, "_stochastic_churn", False)
    if on_device or churn:
      sampler.ensure_device_noise(native, template0)
      native.noise_seed(sampler.seed_from(gen), 0)
    native.set_churn(sampler._per_step_churn_rates if churn else None,
                     getattr(sampler, "_noise_level_inflation_factor", 1.0))

    def draw(k):
      if on_device:
        return None
      return np.asarray(init_noise[k], np.float32) if init_noise is not None else \
          sampler.draw_noise(gen, shape, template0)

    noise = draw(0)
    pending = None                                        # step whose snapshot waits to be downloaded and finished
    for k in range(horizon):
      t0 = _time.perf_counter()
      if on_device:
        native.noise_draw()
      else:
        native.upload_noise(noise)
      native.sample_resident(sigmas, skip_dead_call=True, want_stats=False)   # asynchronous
      # while the GPU samples step k: download step k-1's snapshot (side stream), finish it on the host, draw the next noise
      if pending is not None:
        finish(pending, native.download_stash())
      if k + 1 < horizon:
        noise = draw(k + 1)
        frows = (self._forcing_rows(isel_time(forcings, slice(k + 1, k + 2)), forcing_cols, sizes, grid_shape)
                 if plan["n_forcing"] else None)
      native.stash_sample()                               # waits for sample k (and its domain check); device-side snapshot
      if k + 1 < horizon:
        native.rollout_advance(frows)                     # the gap to the next sample holds no host copy any more
      pending = k
      self.last_step_ms.append(1e3 * (_time.perf_counter() - t0))
    finish(pending, native.download_stash())
    return _on_time_axis(preds, given, horizon)


# ---------------------------------------------------------------------------------------------
# ensemble rollout: every member's context resident on the device, scored at every lead time
# ---------------------------------------------------------------------------------------------
def state_channels(plan, c_out: int) -> np.ndarray:
  """`state_src` [c_out] int32 for `gc_ens_push_state`: the conditioning channel that holds target channel j after
  `gc_rollout_advance`, i.e. the channel c the plan fills from the sample (`kind[c]` 2 or 4) with `sidx[c] == j` --
  the newest input frame of a variable that is both predicted and fed back.  -1: the target channel has no input
  channel (its state is the sample itself).  Two conditioning channels claiming one j raise ValueError."""
  kind, sidx = np.asarray(plan["kind"]), np.asarray(plan["sidx"])
  out = np.full(int(c_out), -1, np.int32)
  for c in np.flatnonzero((kind == 2) | (kind == 4)):
    j = int(sidx[c])
    if not 0 <= j < c_out:
      raise ValueError(f"plan: sample index {j} of channel {c} is outside [0, {c_out})")
    if out[j] >= 0:
      raise ValueError(f"plan: conditioning channels {out[j]} and {c} both take target channel {j}")
    out[j] = c
  return out


class _MemberNoise:
  """The noise of one ensemble member over a whole rollout: ONE generator, seeded by (base_seed, member) only and
  consumed in step order exactly as `DeviceRollout.run(..., rngs=member_seed(base_seed, member))` consumes its own --
  the Philox key first (once, when anything is drawn on the device), then one host field per step unless the initial
  states are drawn on the device or given."""

  def __init__(self, sampler, base_seed: int, member: int, *, needs_key: bool, host_fields: bool):
    from .ensemble import member_seed  # pylint: disable=import-outside-toplevel
    self._sampler = sampler
    self._gen = np.random.default_rng(member_seed(base_seed, member))
    self.key = sampler.seed_from(self._gen) if needs_key else None
    self.stream = 0                                       # Philox stream of the member's next device field
    self._host_fields = host_fields

  def host_field(self, shape, template) -> Optional[np.ndarray]:
    if not self._host_fields:
      return None
    return np.asarray(self._sampler.draw_noise(self._gen, shape, template), np.float32)


class _SeriesResult:
  """What the three results share: the series of the rows of `verification.SCORERS` that name the result's kind
  (`_carried_as`), each a list with one entry per lead time or None, and their merge.  A result that was not given a series of
  an `optional` row keeps no instance attribute for it (it reads as None), so `vars(result)` of a run that does not use the
  scorer is what it was before the scorer existed (tests/golden/rollout_call_sequence.json records it)."""
  _carried_as = "none"
  _kind = "results"                                       # (as the merge's error messages name the two operands)

  @classmethod
  def _rows(cls) -> List[verification.Scorer]:
    return [row for row in verification.SCORERS if cls._carried_as in row.carried_by]

  @classmethod
  def _carries(cls) -> List[str]:
    return [name for row in cls._rows() for name in row.series]

  @classmethod
  def _carries_efi(cls) -> bool:
    return cls._carried_as in verification.EFI_SCORER.carried_by

  def __getattr__(self, name):
    if any(row.optional and name in row.series for row in self._rows()):
      return None
    if name in ("efi", "efi_fields") and self._carries_efi():    # of `run(efi=...)`: absent from `vars(result)` unless asked for
      return None
    if name in ("maps", "maps_normalized", "event_maps"):        # of `run(maps=...)`: likewise
      return None
    raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

  def _set_efi(self, efi, efi_fields) -> None:
    """`efi`: one `verification.EfiScores` per lead time; `efi_fields`: per lead time (EFI, observed index) [G, B, c]."""
    word = verification.EFI_SCORER.word
    if efi is not None:
      self.efi = list(efi)
      if len(self.efi) != len(self.scores):
        raise ValueError(f"scores and the {word} must cover the same lead times")
    if efi_fields is not None:
      self.efi_fields = efi_fields

  def _merged_efi(self, other) -> Optional[list]:
    """The index tables and sums of both results added entry by entry (None: neither has them); the fields belong to one date."""
    if (self.efi is None) != (other.efi is None):
      raise ValueError(f"merge: only one of the two {self._kind} carries the {verification.EFI_SCORER.word}")
    return None if self.efi is None else [type(x).merge([x, y]) for x, y in zip(self.efi, other.efi)]

  _MAP_SERIES = ("maps", "maps_normalized", "event_maps")

  def _set_maps(self, maps, maps_normalized, event_maps) -> None:
    """Of `run(maps=...)`, per slot (a lead time; on a window result a window): `maps[k]` (`verification.ScoreMaps` in physical
    units), `maps_normalized[k]` (as the device holds them), `event_maps[k]` (`verification.EventMaps`, with
    `MapSpec(events=True)`).  Absent from `vars(result)` unless asked for (`verification.MAP_SCORER`: beside the table)."""
    for name, given in zip(self._MAP_SERIES, (maps, maps_normalized, event_maps)):
      if given is not None:
        setattr(self, name, list(given))

  def _merged_maps(self, other) -> Dict[str, Optional[list]]:
    """The planes of both results added slot by slot (`ScoreMaps.merge`, `EventMaps.merge`: a left fold, self first)."""
    out = {}
    for name in self._MAP_SERIES:
      a, b = getattr(self, name), getattr(other, name)
      if (a is None) != (b is None):
        raise ValueError(f"merge: only one of the two {self._kind} carries {verification.MAP_SCORER.word}")
      out[name] = None if a is None else [type(x).merge([x, y]) for x, y in zip(a, b)]
    return out

  def _set_series(self, named, series) -> None:
    """Copies the series into lists (the scores first) and checks that the others cover the lead times of the scores.
    `named`: the constructor's own parameters by name; `series`: its other keywords, each a series the result carries."""
    unknown = [name for name in series if name not in self._carries()]
    if unknown:
      raise TypeError(f"{type(self).__name__}() got an unexpected keyword argument {unknown[0]!r}")
    for row in self._rows():
      for name in row.series:
        given = series.get(name, named.get(name))
        if given is None and row.optional:
          continue                                        # (it reads as None)
        setattr(self, name, None if given is None else list(given))
        if name == row.name and row.word is not None and given is not None and len(getattr(self, name)) != len(self.scores):
          raise ValueError(f"scores and {row.word} must cover the same lead times")

  def _merged_series(self, other) -> Dict[str, Optional[list]]:
    """{attribute: the series of both results merged entry by entry (raw sums add), None where either has none}."""
    for row in self._rows():
      if row.word is not None and (getattr(self, row.name) is None) != (getattr(other, row.name) is None):
        raise ValueError(f"merge: only one of the two {self._kind} carries {row.word}")
    both = lambda a, b: None if a is None or b is None else [type(x).merge([x, y]) for x, y in zip(a, b)]
    return {name: both(getattr(self, name), getattr(other, name)) for name in self._carries()}


def _merge_named(a, b, word: str, names: str):
  """The merge of two {name: result} parts of an `EnsembleRolloutResult` (None: the result has no such part)."""
  if (a is None) != (b is None):
    raise ValueError(f"merge: only one of the two results carries {word}")
  if a is not None and sorted(a) != sorted(b):
    raise ValueError(f"merge: the {names} names differ ({sorted(a)} and {sorted(b)})")
  return None if a is None else {k: v.merge(b[k]) for k, v in a.items()}


class DerivedRolloutResult(_SeriesResult):
  """The part of an `EnsembleRolloutResult` that belongs to one entry of `EnsembleRollout.run(derived=...)`: per lead time
  `scores[k]` (`verification.EnsembleScores` in the units of the derived variables: `scores_normalized[k].scaled(scale_d)`
  with `DerivedSpec.channel_stats`), `scores_normalized[k]` (as the device returned them), `events[k]`
  (`verification.EventScores`, or None without an EventSpec) and `members[k]` (`[M]` arrays [G, B, c_d] in the members' own
  units, or None); `template`: the Dataset of the derived variables (`DerivedSpec.template`) for `per_variable`.  With
  `run(order=...)` also `order[k]` / `order_normalized[k]` (`verification.OrderScores`, as `scores`) and, when asked for,
  `quantiles[k]` (`[Q]` arrays [G, B, c_d] in the members' own units).  With `run(climatology=...)` also `climatology[k]` /
  `climatology_normalized[k]` (`verification.ClimatologyScores`, as `scores`): the derived members against the derived
  climatological samples.  With `run(energy=...)` / `run(variogram=...)` also `energy[k]` (`verification.EnergyScores` over the
  groups whose variables are all derived variables of this entry, in the members' own units; None where no group is) and
  `variogram[k]` / `variogram_normalized[k]` (`verification.VariogramScores`, as `scores`).  With `run(tails={name: spec})`
  also `tails[k]` / `tails_normalized[k]` (`verification.TailScores`, as `scores`).  With `run(regions={name: spec})` also
  `regions[k]` / `regions_normalized[k]` (`verification.RegionScores`, as `scores`)."""

  _carried_as, _kind = "derived", "derived results"

  def __init__(self, scores, scores_normalized, events=None, members=None, template=None, *, quantiles=None, efi=None,
               efi_fields=None, maps=None, maps_normalized=None, event_maps=None, **series):
    self._set_series(locals(), series)
    self._set_efi(efi, efi_fields)
    self._set_maps(maps, maps_normalized, event_maps)
    self.members, self.template, self.quantiles = members, template, quantiles

  def merge(self, other: "DerivedRolloutResult") -> "DerivedRolloutResult":
    return DerivedRolloutResult(template=self.template, efi=self._merged_efi(other), **self._merged_maps(other),
                                **self._merged_series(other))


class FeatureRolloutResult(_SeriesResult):
  """The part of an `EnsembleRolloutResult` that belongs to one entry of `EnsembleRollout.run(features=...)`: per lead time
  `scores[k]` / `scores_normalized[k]` (`verification.EnsembleScores` of the 0 / 1 strike fields: the same numbers, a strike
  field has no unit), `events[k]` (`verification.EventScores` at threshold 0.5: Brier score, reliability curve, ROC area and
  economic value of the strike probability), `centres[k]` ({detector: [B][M + 1] entries} as `verification.unpack_centres`
  gives them, field M the truth, in physical units), `strike_probability[k]` (a Dataset, one variable per detector: the
  ensemble mean of the strike fields) and `members[k]` (`[M]` arrays [G, B, D], the strike fields, or None); `template`: the
  Dataset of the detectors (`FeatureSpec.template`) for `per_variable`.  `order`, `tails` and `regions` as on a
  `DerivedRolloutResult`."""

  _carried_as, _kind = "derived", "feature results"

  def __init__(self, scores, scores_normalized, events=None, centres=None, strike_probability=None, members=None, template=None,
               *, quantiles=None, **series):
    self._set_series(locals(), series)
    self.centres, self.strike_probability = centres, strike_probability
    self.members, self.template, self.quantiles = members, template, quantiles

  def merge(self, other: "FeatureRolloutResult") -> "FeatureRolloutResult":
    """Raw sums and tables add; centres, probability maps and members belong to one date and are dropped."""
    return FeatureRolloutResult(template=self.template, **self._merged_series(other))


class WindowRolloutResult(_SeriesResult):
  """The part of an `EnsembleRolloutResult` that belongs to one entry of `EnsembleRollout.run(windows=...)`.  `leads`: the
  lead times that end a window (`WindowSpec.leads`), `steps`: the window length; per window i, ending at `leads[i]`,
  `scores[i]` (`verification.EnsembleScores` in physical units: `scores_normalized[i].scaled(scale)` with
  `WindowSpec.channel_stats`), `scores_normalized[i]` (as the device returned them), `events[i]` (`verification.EventScores`,
  or None without an EventSpec), `order[i]` / `order_normalized[i]` (`verification.OrderScores`, or None without
  `run(order=...)`) and `members[i]` (`[M]` arrays [G, B, c] of the windowed members in the members' own units, or None);
  `template`: the Dataset of the source's variables for `per_variable`.  With `run(energy=...)` / `run(variogram=...)` also
  `energy[i]` (`verification.EnergyScores` of the windowed fields, in the members' own units; None where no group names
  variables of the source) and `variogram[i]` / `variogram_normalized[i]` (`verification.VariogramScores`, as `scores`).  With
  `run(tails={name: spec})` also `tails[i]` / `tails_normalized[i]` (`verification.TailScores`, as `scores`).  With
  `run(regions={name: spec})` also `regions[i]` / `regions_normalized[i]` (`verification.RegionScores`, as `scores`)."""

  _carried_as, _kind = "window", "window results"

  def __init__(self, leads, steps: int, scores, scores_normalized, events=None, order=None, members=None, template=None,
               *, maps=None, maps_normalized=None, event_maps=None, **series):
    self.leads, self.steps = [int(k) for k in leads], int(steps)
    self._set_series(locals(), series)
    self._set_maps(maps, maps_normalized, event_maps)
    if len(self.scores) != len(self.leads) or len(self.scores_normalized) != len(self.leads):
      raise ValueError("a window result needs one score per window lead time")
    self.members, self.template = members, template

  def merge(self, other: "WindowRolloutResult") -> "WindowRolloutResult":
    """The result over the union of the start dates, window by window: raw sums add; members belong to one date."""
    if self.leads != other.leads or self.steps != other.steps:
      raise ValueError(f"merge: the windows differ (steps {self.steps} and {other.steps}, leads {self.leads} and {other.leads})")
    return WindowRolloutResult(self.leads, self.steps, template=self.template, **self._merged_maps(other),
                               **self._merged_series(other))


class EnsembleRolloutResult(_SeriesResult):
  """What `EnsembleRollout.run` returns.  `scores`: one `verification.EnsembleScores` per lead time; `spectra`: one
  `spectra.EnsembleSpectra` per lead time, or None; `mean` / `variance`: the ensemble mean and variance fields on the
  targets' time axis (physical units), or None; `members`: `[horizon][M]` arrays [G, B, c_out] in the members' own
  units (normalised with the input statistics under a normalisation wrapper), or None; `n_members`.
  `scores_normalized` / `spectra_normalized`: the same lists as the device returned them, in the members' units
  (`scores[k]` is `scores_normalized[k].scaled(s)`).  `events`: one `verification.EventScores` per lead time, or None
  (integer tables: no unit, nothing to rescale).  `derived`: {name: `DerivedRolloutResult`} for the entries of
  `run(derived=...)`, or None.  `order` / `order_normalized`: one `verification.OrderScores` per lead time (as `scores` /
  `scores_normalized`), or None; `quantiles`: `[horizon][Q]` arrays [G, B, c_out] in the members' own units (as `members`),
  or None.  `climatology` / `climatology_normalized`: one `verification.ClimatologyScores` per lead time (as `scores` /
  `scores_normalized`) -- anomaly correlation and CRPS skill score against the samples of `run(climatology=...)` -- or None.
  `windows`: {name: `WindowRolloutResult`} for the entries of `run(windows=...)`, or None.  `energy`: one
  `verification.EnergyScores` per lead time -- the energy score of the groups of `run(energy=...)`, in the members' own units
  (normalised under a normalisation wrapper: what makes a norm over several variables meaningful) -- or None; `variogram` /
  `variogram_normalized`: one `verification.VariogramScores` per lead time (as `scores` / `scores_normalized`), or None.
  `tails` / `tails_normalized`: one `verification.TailScores` per lead time (as `scores` / `scores_normalized`) -- the
  threshold-weighted CRPS at the thresholds of `run(tails=...)` -- or None.  `regions` / `regions_normalized`: one
  `verification.RegionScores` per lead time (as `scores` / `scores_normalized`) -- the scores of every region of
  `run(regions=...)`, `regions[k][name]` an `EnsembleScores` -- or None."""

  _carried_as = "ensemble"

  def __init__(self, scores, spectra=None, mean=None, variance=None, members=None, n_members: Optional[int] = None, *,
               derived=None, quantiles=None, windows=None, features=None, efi=None, efi_fields=None, maps=None,
               maps_normalized=None, event_maps=None, **series):
    self._set_series(locals(), series)
    self._set_efi(efi, efi_fields)
    self._set_maps(maps, maps_normalized, event_maps)
    self.derived = None if derived is None else dict(derived)
    self.windows = None if windows is None else dict(windows)
    if features is not None:                              # (as an optional series: absent from `vars(result)` unless asked for)
      self.features = dict(features)
    self.mean, self.variance, self.members, self.quantiles = mean, variance, members, quantiles
    self.n_members = int(n_members if n_members is not None else self.scores[0].n_members)

  @property
  def horizon(self) -> int:
    return len(self.scores)

  def __getattr__(self, name):
    if name == "features":                                # {name: `FeatureRolloutResult`} of `run(features=...)`, else None
      return None
    return super().__getattr__(name)

  def merge(self, other: "EnsembleRolloutResult") -> "EnsembleRolloutResult":
    """The result over the union of the start dates, lead time by lead time (`EnsembleScores.merge`,
    `EnsembleSpectra.merge`, `OrderScores.merge`, `ClimatologyScores.merge`, `VariogramScores.merge`, `TailScores.merge`,
    `RegionScores.merge`: raw sums add; `EnergyScores.merge`: the forecasts of both).  Fields, members and quantile fields belong to one date and are dropped."""
    if other.horizon != self.horizon:
      raise ValueError(f"merge: horizons differ ({self.horizon} and {other.horizon})")
    if other.n_members != self.n_members:
      raise ValueError(f"merge: member counts differ ({self.n_members} and {other.n_members})")
    series = self._merged_series(other)
    return EnsembleRolloutResult(n_members=self.n_members, **series, efi=self._merged_efi(other), **self._merged_maps(other),
                                 derived=_merge_named(self.derived, other.derived, "derived scores", "derived"),
                                 windows=_merge_named(self.windows, other.windows, "windows", "window"),
                                 features=_merge_named(self.features, other.features, "features", "feature"))


class _StoreSeries:
  """One scored store of an `EnsembleRollout.run` -- the main store, the view of a `derived` entry or the store of a window --
  as a `verification.ScoredStore`, the scale and the template of its channels, and what the lead times have yielded so far:
  every series the store and the `keep_*` flags call for is a list, the others are None."""

  def __init__(self, store, scale, template, *, keep_members: bool = False, keep_quantiles: bool = False,
               keep_efi: bool = False):
    self.store, self.scale, self.template = store, scale, template
    # the extreme forecast index of a store with an `EfiSpec` (`verification.EFI_SCORER`: beside the table) and its two fields
    self.efi = [] if getattr(store, "efi", None) is not None else None
    self.efi_fields = [] if self.efi is not None and keep_efi else None
    # {series, by the name a result has it under: its list} of the scores and of every row the store has switched on
    self.lists = {name: [] for row in verification.SCORERS
                  if row.name == "scores" or getattr(store, row.name, None) is not None for name in row.series}
    self.quantiles = [] if store.order is not None and keep_quantiles else None
    self.members = [] if keep_members else None
    # the score maps of a store with a `MapSpec`: the slot the next scored lead (or window) is added into, and what
    # `collect_maps` downloads at the end of a run that does not keep them resident
    self.map_slot, self.map_series = 0, {}
    # a store with a feature plan: per lead time the centres and the strike-probability map
    self.centres, self.probabilities = ([], []) if getattr(store, "feature_plan", None) is not None else (None, None)

  def __getattr__(self, name):
    """`series.tails`, `series.raw_tails`, `series.raw`, `series.clim`, ...: a list of `lists` by its short name (None: the
    store does not have the scorer switched on)."""
    short = {"raw": "raw_scores", "clim": "climatology", "raw_clim": "raw_climatology"}.get(name, name)
    key = short[4:] + "_normalized" if short.startswith("raw_") else short
    if name != "lists" and any(key in row.series for row in verification.SCORERS):
      return self.lists.get(key)
    raise AttributeError(name)

  def score_lead(self, truth=None, *, want_fields: bool = False, after_score=None, clim_fields=None, n_samples=None,
                 source_truth=None) -> None:
    """Scores the store as it stands and appends to every series: the scores (the events ride with them), then, after
    `after_score()`, every other row of `verification.SCORERS` the store has switched on -- the order statistics and their
    quantile fields, the climatology scores, the energy and variogram scores, the tail scores, the region scores -- then the
    members, in that order on the device.  `truth`, `want_fields`: as `ScoredStore.score`; `after_score()`: what the caller
    downloads between the scores and the rest; `clim_fields`, or `n_samples` and `source_truth`: as
    `ScoredStore.score_climatology`."""
    lists = self.lists
    raw, ev = self.store.score(truth, want_fields=want_fields)   # (the events: on the truth already on the device)
    lists["scores_normalized"].append(raw)
    lists["scores"].append(raw.scaled(self.scale))
    if ev is not None:
      lists["events"].append(ev)
    if after_score is not None:
      after_score()
    for row in verification.SCORERS:
      if row.name in ("scores", "events") or row.name not in lists:
        continue
      if row.name == "climatology":
        raw = self.store.score_climatology(clim_fields, None, n_samples=n_samples, source_truth=source_truth)
      else:
        raw = self.store._score(row, None)                  # (the truth is on the device already)  pylint: disable=protected-access
      if row.scaled:
        lists[row.name + "_normalized"].append(raw)
        raw = raw.scaled(self.scale)
      lists[row.name].append(raw)                           # (without `scaled`: in the store's own units)
      if row.name == "order" and self.quantiles is not None:
        self.quantiles.append(self.store.quantile_fields())
    if self.efi is not None:                                # (behind the climatology row, which has filled the second handle)
      self.efi.append(verification.EFI_SCORER.score(self.store, None))
      if self.efi_fields is not None:
        self.efi_fields.append(self.store.efi_fields())
    if getattr(self.store, "maps", None) is not None:       # (the events ran with the scores: their codes are on the device)
      self.store.accumulate_maps(self.map_slot)
      self.map_slot += 1
    if self.members is not None:
      self.members.append([self.store.handle.ens_download_member(m) for m in range(self.store.n_members)])

  def collect_maps(self) -> Dict[str, Optional[list]]:
    """Downloads every slot of the store's accumulators: {"maps": physical units, "maps_normalized": as the device holds them,
    "event_maps": with `MapSpec(events=True)`, else None}; kept as `map_series` for the results."""
    store = self.store
    got = [store.download_maps(slot) for slot in range(store.map_slots)]
    raw = [g[0] if store.maps.events else g for g in got]
    scale = np.asarray(self.scale, np.float64)[list(raw[0].channels)]
    self.map_series = {"maps": [r.scaled(scale) for r in raw], "maps_normalized": raw,
                       "event_maps": [g[1] for g in got] if store.maps.events else None}
    return self.map_series

  def carried(self, result) -> Dict[str, list]:
    """The series of the store that a result of class `result` carries, as the keywords of its constructor."""
    return {name: series for name, series in self.lists.items() if name in result._carries()}  # pylint: disable=protected-access

  def feature_result(self) -> FeatureRolloutResult:
    return FeatureRolloutResult(centres=self.centres, strike_probability=self.probabilities, members=self.members,
                                template=self.template, quantiles=self.quantiles, **self.carried(FeatureRolloutResult))

  def derived_result(self) -> DerivedRolloutResult:
    return DerivedRolloutResult(members=self.members, template=self.template, quantiles=self.quantiles, efi=self.efi,
                                efi_fields=self.efi_fields, **self.map_series, **self.carried(DerivedRolloutResult))


class _WindowEntry:
  """One entry of `EnsembleRollout.run(windows=...)`: its window handle's store as a `_StoreSeries` (the ring lives on that
  handle) and the handle its pushes come from."""

  def __init__(self, spec, series: _StoreSeries, source, horizon: int):
    self.spec, self.series, self.source = spec, series, source
    self.leads = spec.leads(horizon)

  def start(self) -> None:
    """Before the first lead time: the store, what is scored on it, the plan, and an empty ring."""
    self.series.store.setup()
    self.series.store.handle.ens_window_set(**self.spec.plan())
    self.series.store.handle.ens_window_reset()

  def push(self) -> None:
    """The source's members and truth as they stand (the truth of the lead is on the device already) into the ring."""
    self.series.store.handle.ens_window_push(self.source, None)

  def finish_lead(self, k: int) -> None:
    """At a lead time that ends a window: the window into the store, scored there like any other store."""
    if k in self.leads:
      self.series.store.handle.ens_window_emit()
      self.series.score_lead()

  def result(self) -> WindowRolloutResult:
    s = self.series
    return WindowRolloutResult(self.leads, self.spec.steps, members=s.members, template=s.template, **s.map_series,
                               **s.carried(WindowRolloutResult))


class _EnsembleRun:
  """The state of one `EnsembleRollout.run`: what `_setup` made (handles, plan, noise sources, the main store `main`, the
  derived `views` and the `windows`) and the fields and spectra `_score_lead` appends next to the main store's series."""

  def __init__(self):
    self.means, self.variances = [], []
    self.thresholds = None                                # per EventSpec, in the members' units
    self.views: Dict[str, _StoreSeries] = {}
    self.features: Dict[str, _StoreSeries] = {}
    self.windows: Dict[str, _WindowEntry] = {}


def _to_members_units(x: np.ndarray, scale, loc, normalized: bool) -> np.ndarray:
  """[..., c] physical values in the members' units: (x - l) / s in float64, rounded once; without a norm one plain cast."""
  return ((x.astype(np.float64) - loc) / scale).astype(np.float32) if normalized else x.astype(np.float32)


def _members_units(ds, shape, scale, loc, normalized: bool) -> np.ndarray:
  """A Dataset as [G, B, c] in the members' units (`_to_members_units`)."""
  ds = datasets.as_dataset(ds)
  x = np.transpose(datasets.dataset_to_stacked(ds, ds.sizes), (1, 2, 0, 3)).reshape(shape)
  return _to_members_units(x, scale, loc, normalized)


def _spec_entries(entries) -> Dict[str, tuple]:
  """The entries of `derived=` / `windows=` as {name: (spec, EventSpec or None)}."""
  return {name: tuple(entry) if isinstance(entry, (tuple, list)) else (entry, None) for name, entry in (entries or {}).items()}


def _per_store(arg: str, given, known) -> Optional[dict]:
  """An argument of `run` that is a spec for the main store, or {None: spec, name: spec, ...}, as that mapping (None stays
  None); a name that is not among `known`, the entries of `derived` and `windows`, is a ValueError."""
  if given is None:
    return None
  given = dict(given) if isinstance(given, Mapping) else {None: given}
  if set(given) - known - {None}:
    raise ValueError(f"{arg}: {sorted(set(given) - known - {None})} name no entry of `derived` or `windows` ({sorted(known)})")
  return given


class EnsembleRollout:
  """M members rolled out `horizon` steps with every member's conditioning resident in HBM, scored at every lead time
  on the device.  What is scored is each member's STATE -- the channels of its advanced context
  (`state_channels`) -- not its sample: under `InputsAndResiduals` a sample is a residual relative to that member's own
  previous frame and is not comparable between members from the second step on.

  Member m is exactly `DeviceRollout(model, norm).run(..., rngs=member_seed(base_seed, m))`, bit for bit, however many
  lanes (`concurrent_members`, `Denoiser.member_lanes`) are used and however the members fall into groups: its context
  travels with it through the context store (`gc_ctx_save` / `gc_ctx_load`), its noise through `_MemberNoise` and, for
  fields drawn on the device, the library's own stream counter ("noise_stream")."""

  def __init__(self, model, norm: Optional[InputsAndResiduals] = None, task: cfg.TaskConfig = cfg.TASK, *,
               base_seed: int = 0, concurrent_members: int = 1, device_noise: bool = False,
               rank: int = 0, world_size: int = 1):
    if concurrent_members < 1:
      raise ValueError("concurrent_members must be >= 1")
    self.model = model                                    # a GenCast (its sampler drives the native handles)
    self.norm = norm
    self.task = task
    self.base_seed = int(base_seed)
    self.concurrent_members = int(concurrent_members)
    self.device_noise = bool(device_noise)
    self.rank, self.world_size = int(rank), int(world_size)
    self.last_lead_ms: List[float] = []

  def member_noise(self, member: int, *, given: bool = False) -> _MemberNoise:
    """The noise source of one member; `given`: the initial states come from `init_noise`."""
    sampler = self.model._sampler  # pylint: disable=protected-access
    on_device = self.device_noise and not given
    churn = bool(getattr(sampler, "_stochastic_churn", False))
    return _MemberNoise(sampler, self.base_seed, member, needs_key=on_device or churn,
                        host_fields=not on_device and not given)

  @staticmethod
  def next_forcings(forcings: Dataset, k: int, horizon: int) -> Dataset:
    """The forcing frame `gc_rollout_advance` takes after step k: frame k + 1.  After the LAST step the frame `horizon`
    is used when `forcings` carries one; else frame `horizon - 1` is used again -- no sample ever reads those channels
    (the rollout ends there) and no state channel is a forcing channel, so the scores cannot depend on them."""
    del horizon                                           # (frame k + 1 can only be missing after the last step)
    t = k + 1 if k + 1 < forcings.sizes.get("time", 0) else k
    return isel_time(forcings, slice(t, t + 1))

  def _stat(self, stat, template: Dataset, default: float) -> np.ndarray:
    return np.concatenate([_per_channel_stat(stat, name, template[name], default)
                           for name, _, _ in datasets.channel_layout(template)])

  def run(self, inputs, targets, forcings, horizon: int, num_members: int, *, context_steps: int = 2,
          init_noise=None, spectra: bool = False, lmax: Optional[int] = None, fields: bool = False,
          keep_members: bool = False, events=None, derived=None, order=None,
          keep_quantiles: bool = False, climatology=None, windows=None, energy=None,
          variogram=None, tails=None, regions=None, features=None, efi=None,
          keep_efi: bool = False, maps=None, maps_resident: bool = False) -> EnsembleRolloutResult:
    """Rolls `num_members` (2..64) members out `horizon` steps and scores them against `targets[k]` at every lead time
    k.  `init_noise[m][k]`: a given initial state [G, B, c_out] for member m, step k.  `spectra` / `lmax`: also the
    spherical-harmonic spectra per lead time (`targets` must then be finite).  `fields`: also the ensemble mean and
    variance as Datasets on the targets' time axis.  `keep_members`: also every member state, downloaded.
    `events`: a `verification.EventSpec` (thresholds in the physical units of `targets`), or a sequence of `horizon` of
    them with equal directions (a climatology that moves with the lead time): also the event tables per lead time,
    `EnsembleRolloutResult.events`, counted right after the scores on the truth already on the device.  The thresholds
    take the map of the truth, (thr - l) / s in float64, rounded once; s > 0, so no direction flips.
    `derived`: {name: `verification.DerivedSpec`, or (DerivedSpec, EventSpec)}: per lead time, after the scores, the member
    states and the truth go through `gc_ens_derive` into the store of a view handle (`Denoiser.view_handle`) -- wind speed
    in physical units from the normalised components, fields pooled over a neighbourhood -- and are scored there with the
    same node weights: `EnsembleRolloutResult.derived[name]`.  The thresholds of such an EventSpec are keyed by the derived
    names, in physical units, and take the map of `DerivedSpec.channel_stats`.  With `keep_members` the derived members
    are downloaded too.  A `verification.BandSpec` goes wherever a DerivedSpec goes: the states and the truth are then
    analysed, weighted per total wavenumber and synthesised back (`gc_ens_band`) into a handle of the
    entry's own (`Denoiser.band_handle`) that holds the analysis tables of its band limit -- the scores of the planetary
    waves, of the synoptic scales, of what is left without them; the members stay in the normalised units of their source
    channel (`BandSpec.channel_stats`).
    `order`: probabilities (at most 8; an empty sequence: none): per lead time, after the scores, the member states are
    sorted point by point on the device (`gc_ens_order_score`, on the truth already there): `EnsembleRolloutResult.order`
    (`verification.OrderScores`: the reliability / potential split of the ensemble CRPS, pinball loss and coverage of the
    quantiles), and the same for every `derived` entry on its derived members.  `keep_quantiles`: also the quantile
    fields, downloaded, in the members' units (`EnsembleRolloutResult.quantiles`).  Without `order` nothing changes.
    `climatology`: a sequence of `horizon` entries, or a callable of the lead time k, giving the K (2..64) climatological
    samples of lead k -- Datasets shaped like `targets[k]` in physical units, past states for that calendar date; a plain
    climatological mean is given twice.  Per lead time, after the scores, they take the map of the truth, go into the store
    of a second handle (`Denoiser.climatology_handle`) and the member states are scored against them
    (`gc_ens_clim_score`, on the truth already there): `EnsembleRolloutResult.climatology` (`verification.ClimatologyScores`:
    anomaly correlation of the ensemble mean, CRPS skill score).  For every `derived` entry the samples go through the
    entry's plan as the members do (`gc_ens_derive` from the climatology handle into a climatology view) and the derived
    members are scored against them.  A NaN in a sample is a point the device skips.  Without `climatology` nothing changes.
    `windows`: {name: `verification.WindowSpec`, or (WindowSpec, EventSpec)}: per lead time, after the scores, the member
    states and the truth of the entry's source -- the main store, or the view of a `derived` entry -- are copied into a ring
    on a window handle (`Denoiser.window_handle`, one per entry); at the lead times that end a window (`WindowSpec.leads`)
    the last `steps` of them become one field per member and for the truth (`gc_ens_window_emit`: an accumulation, a mean,
    a change, the extreme over time) and are scored there with the same node weights, with `order` where given:
    `EnsembleRolloutResult.windows[name]` (`WindowRolloutResult`).  The thresholds of such an EventSpec are keyed by the
    source's variable names, in physical units, and take the map of `WindowSpec.channel_stats`.  With `keep_members` the
    windowed members are downloaded too.  `climatology` does not reach the windows: skill of a windowed field needs the
    window of every climatological sample, which is not built.  Without `windows` nothing changes.
    `energy`: a `verification.EnergySpec` (groups of variables, e.g. the two components of the 10 m wind, or every level of
    the geopotential): per lead time, after the scores, the energy score of every group over the member states
    (`gc_ens_energy_score`, on the truth already there): `EnsembleRolloutResult.energy` (`verification.EnergyScores`), in the
    members' own units -- normalised under a normalisation wrapper, which is what makes a norm over several variables
    meaningful.  A store is scored over the groups whose variables it all has: the main store and the windows on it by the
    names of `targets`, a `derived` entry and the windows on it by its derived names; a group that fits no store is an
    error.  `variogram`: a `verification.VariogramSpec` (grid offsets, an order p): per lead time the variogram score of
    every channel at every offset (`gc_ens_variogram_score`): `EnsembleRolloutResult.variogram` in physical units
    (`VariogramScores.scaled`), `variogram_normalized` as the device returned it, and the same for every `derived` entry
    and every window.  Without them nothing changes.
    `tails`: a `verification.EventSpec` read as tails (direction > 0: the upper tail, weight 1{z >= threshold}; < 0: the lower
    tail) for the main store, or a mapping {None: spec, name: spec, ...} whose other keys name entries of `derived` /
    `windows` (an unknown key is a ValueError), with thresholds keyed by that store's variable names in physical units.  Per
    lead time, after the variogram, the members of every point are sorted once and the threshold-weighted CRPS sums of all
    thresholds are formed (`gc_ens_tail_score`, on the truth already there): `EnsembleRolloutResult.tails`
    (`verification.TailScores` in physical units, `TailScores.scaled`), `tails_normalized` as the device returned them, and
    the same on the results of the named entries.  The thresholds reach the members' units by the path of the thresholds of
    `events`.  Without `tails` nothing changes.
    `regions`: a `verification.RegionSpec` (named masks over the grid nodes, overlapping or not) for the main store, or a
    mapping {None: spec, name: spec, ...} whose other keys name entries of `derived` / `windows` (an unknown key is a
    ValueError; every store lives on the same grid nodes).  Per lead time, after the tails, ONE pass over the nodes that belong
    to any region forms the sums of `scores` for every region (`gc_ens_region_score`, on the truth already there):
    `EnsembleRolloutResult.regions` (`verification.RegionScores` in physical units, `regions[k][name]` an `EnsembleScores`),
    `regions_normalized` as the device returned them, and the same on the results of the named entries.  Without `regions`
    nothing changes.
    `features`: {name: `verification.FeatureSpec`}: per lead time, after the derived entries, the member states and the truth
    go through `gc_ens_feature` into the store of a handle of the entry's own (`Denoiser.feature_handle`) -- the centres of
    every detector (cyclone centres: a local extremum with a threshold and a closed-contour depth test, in physical units)
    as lists, and as 0 / 1 strike fields, which are scored there like a `derived` entry with the same node weights and with
    the event `strike > 0.5`: `EnsembleRolloutResult.features[name]` (`FeatureRolloutResult`: `scores[k]`, `events[k]`,
    `centres[k]`, `strike_probability[k]`).  `order`, and `tails` / `regions` under the entry's name, reach it; `energy`,
    `variogram` and `climatology` do not.  A window may name it as its source: `WindowSpec("max", L, source=name)` is a strike
    within L steps, the track-probability map.  `verification.link_tracks` links the centres of a member over the lead times.
    Without `features` nothing changes.
    `efi`: a `verification.EfiSpec`, together with `climatology` (without it a ValueError): per lead time, behind the
    climatology scores, the member states are ranked point by point in the K samples already in the second handle's store
    (`gc_ens_efi_score`, on the truth already there): `EnsembleRolloutResult.efi` (`verification.EfiScores`: mean index, its
    correlation with the observed index, the ROC of the index against the climatological events of the spec), and the same
    for every `derived` entry -- a band view included -- on its derived members and derived samples.  The index has no
    unit, so there is no normalised twin.  `keep_efi`: also the two fields, downloaded: `efi_fields[k]` = (EFI, observed
    index), [G, B, c] each.  It does not reach the windows (`climatology` does not) nor the `features`.  Without `efi` nothing
    changes.
    `maps`: a `verification.MapSpec` for the main store, or a mapping {None: spec, name: spec, ...} whose other keys name
    entries of `derived` / `windows`: per lead time (per window, on a window entry), behind everything else that is scored, the
    date is added into the store's score maps on the device (`gc_ens_map_accumulate`; slot = lead index, or the index of the
    window) -- per grid point the planes of bias, RMSE, spread, CRPS and the outlier counts, with `MapSpec(events=True)` also
    the event planes of the store's EventSpec.  By default a run zeroes its slots, adds its one date and downloads them at the
    end: `EnsembleRolloutResult.maps[k]` (`verification.ScoreMaps` in physical units), `maps_normalized[k]`, `event_maps[k]`,
    and the same on the results of the named entries; `merge` adds them over start dates.  With `maps_resident` a run neither
    zeroes nor downloads: the sums stay in HBM over any number of runs with the same plan and horizon (another plan or horizon
    is a ValueError), `download_maps()` fetches them once and `reset_maps()` clears them.  A store that shares its handle with
    another (two `derived` entries of equal width, one EventSpec per lead time) cannot keep maps.  Without `maps` nothing changes.

    Units: scores and spectra are returned in the units of `targets` through `EnsembleScores.scaled(s)` /
    `EnsembleSpectra.scaled(s)`, s the input scale per channel; the location offset l cancels in every score and in the
    error and spread spectra.  `truth_power`, `member_power` and `mean_power` are those of (x - l) s / s = x - l: a
    constant offset moves l = 0 only, through a cross term the sums do not hold, so at l = 0 they
    are the power of the field minus its climatological location, at l > 0 the field's own.  Fields are un-normalised
    with s and l.  A NaN in `targets` is a point the device skips (`ens_invalid_points`).

    After the last step the context is advanced once more to form the state; see `next_forcings` for the forcing frame
    that update takes."""
    if self.world_size > 1:
      raise ValueError("EnsembleRollout needs all members on one rank (world_size == 1): bring the other "
                       "ranks' members over and push them with NativeDenoiser.ens_push_host")
    for name, (wspec, _) in _spec_entries(windows).items():
      if wspec.source is not None and wspec.source not in (derived or {}) and wspec.source not in (features or {}):
        raise ValueError(f"window {name!r}: its source {wspec.source!r} names no entry of `derived` ({sorted(derived or {})})"
                         + (f" or `features` ({sorted(features)})" if features else ""))
    if set(derived or {}) & set(features or {}):
      raise ValueError(f"derived and features share the names {sorted(set(derived or {}) & set(features or {}))}")
    given = (targets, inputs, forcings)
    inputs, targets, forcings = (datasets.as_dataset(x) for x in (inputs, targets, forcings))
    M = int(num_members)
    if horizon < 1 or targets.sizes.get("time", 0) < horizon:
      raise ValueError(f"targets carry {targets.sizes.get('time', 0)} time steps (need horizon = {horizon})")
    if energy is not None:                                # every group must fit a store: the main one or a derived view
      template0 = isel_time(targets, slice(0, 1)).map(np.zeros_like)
      fitted = set()
      for template in [template0] + [dspec.template(template0) for dspec, _ in _spec_entries(derived).values()]:
        part = energy.restricted(template)
        fitted.update(() if part is None else part.names)
      if set(energy.names) - fitted:
        raise ValueError(f"energy: the groups {sorted(set(energy.names) - fitted)} name variables that no scored store has all of")
    if init_noise is not None and (len(init_noise) != M or any(len(z) < horizon for z in init_noise)):
      raise ValueError("init_noise must be [num_members][horizon] fields")
    known = set(derived or {}) | set(windows or {}) | set(features or {})
    per_store = {arg: _per_store(arg, spec, known) for arg, spec in (("tails", tails), ("regions", regions))}
    map_specs = _per_store("maps", maps, set(derived or {}) | set(windows or {}))
    if maps_resident and map_specs is None:
      raise ValueError("maps_resident goes with maps=...")
    run = self._setup(inputs, targets, forcings, horizon, M, context_steps=context_steps, init_noise=init_noise,
                      spectra=spectra, lmax=lmax, fields=fields, keep_members=keep_members, events=events, derived=derived,
                      order=order, keep_quantiles=keep_quantiles, climatology=climatology, windows=windows, energy=energy,
                      variogram=variogram, per_store=per_store, features=features, efi=efi, keep_efi=keep_efi,
                      map_specs=map_specs, maps_resident=maps_resident)
    self.last_lead_ms = []
    for k in range(horizon):
      t0 = _time.perf_counter()
      self._sample_lead(run, k, forcings, horizon)
      self._score_lead(run, k, targets)
      self.last_lead_ms.append(1e3 * (_time.perf_counter() - t0))
    main = run.main
    if map_specs is not None:
      self._map_run = run                                  # (what `download_maps` / `reset_maps` reach)
      if not maps_resident:
        for series in self._map_stores(run).values():
          series.collect_maps()
    return EnsembleRolloutResult(mean=_on_time_axis(run.means, given, horizon) if fields else None,
                                 variance=_on_time_axis(run.variances, given, horizon) if fields else None,
                                 members=main.members, n_members=M, quantiles=main.quantiles,
                                 derived=None if derived is None else {k: v.derived_result() for k, v in run.views.items()},
                                 windows=None if windows is None else {k: v.result() for k, v in run.windows.items()},
                                 features=None if features is None else {k: v.feature_result() for k, v in run.features.items()},
                                 spectra=run.spectra, spectra_normalized=run.raw_spectra, efi=main.efi,
                                 efi_fields=main.efi_fields, **main.map_series, **main.carried(EnsembleRolloutResult))

  @staticmethod
  def _map_stores(run: "_EnsembleRun") -> Dict[Optional[str], "_StoreSeries"]:
    """{store name (None: the main store): its series} of the stores of a run that keep score maps."""
    named = [(None, run.main)] + list(run.views.items()) + [(name, w.series) for name, w in run.windows.items()]
    return {name: series for name, series in named if getattr(series.store, "maps", None) is not None}

  def download_maps(self) -> Dict[Optional[str], Dict[str, Optional[list]]]:
    """The score maps the last `run(maps=...)` left on the device -- with `maps_resident` the sums over every run since they
    were last cleared -- as {store name (None: the main store): {"maps": [slots] `ScoreMaps` in physical units,
    "maps_normalized": as the device holds them, "event_maps": `EventMaps` or None}}: per store the series the result of a
    run without `maps_resident` carries."""
    run = getattr(self, "_map_run", None)
    if run is None:
      raise ValueError("download_maps: no run with maps=... has been made")
    return {name: dict(series.collect_maps()) for name, series in self._map_stores(run).items()}

  def reset_maps(self) -> None:
    """Zeroes the score maps of every store of the last `run(maps=...)`; the next run may bring another plan or horizon."""
    run = getattr(self, "_map_run", None)
    if run is None:
      raise ValueError("reset_maps: no run with maps=... has been made")
    for series in self._map_stores(run).values():
      series.store.forget_maps()

  def _setup(self, inputs, targets, forcings, horizon, M, *, context_steps, init_noise, spectra, lmax, fields, keep_members,
             events, derived, order, keep_quantiles, climatology, windows, energy, variogram, per_store,
             features=None, efi=None, keep_efi=False, map_specs=None, maps_resident=False) -> "_EnsembleRun":
    """Everything `run` does before the first sample: lanes, context store, the main store and the derived views.  The
    keywords are `run`'s own; `per_store`: {argument given per store ("tails", "regions"): {store name: spec} or None}."""
    run = _EnsembleRun()
    context = isel_time(inputs, slice(-context_steps, None))
    template0 = isel_time(targets, slice(0, 1)).map(np.zeros_like)
    forc0 = isel_time(forcings, slice(0, 1))
    sampler = self.model._sampler  # pylint: disable=protected-access
    den: Denoiser = self.model.denoiser
    norm = self.norm
    if norm is not None:
      n_in = normalize(context, norm._scales, norm._locations)
      n_fo = normalize(forc0, norm._scales, norm._locations)
    else:
      n_in, n_fo = context, forc0
    cond, run.grid_shape, slots = den.init_for(n_in, template0, n_fo)
    native = den.native
    run.plan, run.forcing_cols = build_rollout_plan(context, forc0, template0, self.task, norm)
    run.state_src = state_channels(run.plan, den.dims.c_out)
    lanes = [native]
    n_lanes = min(self.concurrent_members, M)
    if n_lanes > 1:
      lanes += list(den.member_lanes(n_lanes - 1))
    for lane in lanes:
      lane.set_noisy_slots(slots)
      lane.rollout_plan(**run.plan)
    native.upload_cond(cond)
    native.ctx_reserve(M)
    for m in range(M):                                    # every member starts from the initial conditioning
      native.ctx_save(m)
    scale = self._stat(None if norm is None else norm._scales, template0, 1.0)
    loc = self._stat(None if norm is None else norm._locations, template0, 0.0)

    def packed(spec, template, s, l):
      """The thresholds [T, G, B, c] in the members' units: the map of the truth."""
      return _to_members_units(spec.packed(template), s, l, norm is not None)

    entries, wentries = _spec_entries(derived), _spec_entries(windows)
    # the multivariate plans: the offsets are the grid's, the same for every store; the groups go by a store's variable names
    vplan = None if variogram is None else variogram.plan(template0)

    def eplan(template):
      part = None if energy is None else energy.restricted(template)
      return None if part is None else part.plan(template)

    def per_store_args(name, template, s, l):
      """The `ScoredStore` keywords of the store `name` (None: the main store) for what is given per store: the spec and the
      settings its row makes of it (`Scorer.from_spec`; thresholds come in the members' units)."""
      out = {}
      for arg, specs in per_store.items():
        spec = (specs or {}).get(name)
        if spec is not None:
          out.update({arg: spec}, **verification.scorer(arg).from_spec(spec, template, lambda sp, t: packed(sp, t, s, l)))
      return out

    def map_args(name, template, slots):
      """The `ScoredStore` keywords of the score maps of the store `name`: one slot per scored lead time (or window)."""
      spec = (map_specs or {}).get(name)
      if spec is None:
        return {}
      if not 1 <= slots <= 128:
        raise ValueError(f"maps: {slots} slots (lead times or windows) -- the accumulators hold 1..128")
      return dict(maps=spec, map_channels=spec.channels(template), map_slots=slots, maps_resident=maps_resident)

    weights = verification.node_weights(template0)        # the same nodes everywhere: quantised once, too
    wq = None
    if efi is not None and climatology is None:
      raise ValueError("efi: the extreme forecast index ranks the members in the samples of `climatology`, which was not given")
    if (events is not None or features or any(dev is not None for _, dev in entries.values())
        or any(wev is not None for _, wev in wentries.values()) or (efi is not None and efi.n_events)):
      wq = verification.quantize_node_weights(weights)
    specs = None
    if events is not None:
      specs = list(events) if isinstance(events, (list, tuple)) else [events]
      if len(specs) not in (1, horizon) or any(s.directions != specs[0].directions for s in specs):
        raise ValueError(f"events must be one EventSpec or {horizon} of them with equal directions")
      if any(s.scales_km != specs[0].scales_km for s in specs):
        raise ValueError("the EventSpecs of the lead times must have equal scales_km")
      run.thresholds = [packed(s, template0, scale, loc) for s in specs]
    if climatology is not None and not callable(climatology) and len(climatology) < horizon:
      raise ValueError(f"climatology must give the samples of {horizon} lead times, got {len(climatology)}")
    run.climatology = climatology
    clim_handle = None if climatology is None else den.climatology_handle(den.dims.c_out)
    # one spec: uploaded once, it survives the store and every lead time; else the one of the lead, before it is scored
    main = verification.ScoredStore(native, M, weights, events=None if specs is None else specs[0],
                                    thresholds=None if specs is None else run.thresholds[0], weight_q=wq,
                                    set_per_score=specs is not None and len(specs) > 1, order=order, climatology=clim_handle,
                                    energy=eplan(template0), variogram=vplan, efi=efi, **map_args(None, template0, horizon),
                                    **per_store_args(None, template0, scale, loc))
    run.main = _StoreSeries(main, scale, template0, keep_members=keep_members, keep_quantiles=keep_quantiles, keep_efi=keep_efi)
    main.reserve()
    if spectra:
      _spectra.ensure_tables(native, template0, lmax)

    run.given_noise = init_noise is not None
    run.init_noise = init_noise
    run.noise = [self.member_noise(m, given=run.given_noise) for m in range(M)]
    churn = bool(getattr(sampler, "_stochastic_churn", False))
    run.on_device = self.device_noise and not run.given_noise
    if run.on_device or churn:
      sampler.ensure_device_noise(native, template0)
      key = (len(template0.coords["lat"]), len(template0.coords["lon"]))
      for lane in lanes[1:]:                              # (the sampler remembers lane 0 only)
        if getattr(lane, "_noise_tables_key", None) != key:
          lane.noise_set_tables(*key, *sampler._noise_gen.device_tables())  # pylint: disable=protected-access
          lane._noise_tables_key = key  # pylint: disable=protected-access
    for lane in lanes:
      lane.set_churn(sampler._per_step_churn_rates if churn else None,  # pylint: disable=protected-access
                     getattr(sampler, "_noise_level_inflation_factor", 1.0))

    run.M, run.lanes, run.native, run.template0 = M, lanes, native, template0
    run.sigmas = np.asarray(sampler.noise_levels, np.float32)
    run.shape = (cond.shape[0], cond.shape[1], den.dims.c_out)
    run.sizes = dict(forc0.sizes)
    run.sizes.update(context.sizes)
    run.rows_of = DeviceRollout(self.model, norm, self.task)._forcing_rows  # pylint: disable=protected-access
    run.scale, run.loc, run.normalized = scale, loc, norm is not None
    run.want_fields, run.want_spectra = bool(fields), bool(spectra)
    run.spectra, run.raw_spectra = ([], []) if spectra else (None, None)
    if not main.set_per_score:
      main.configure()

    for name, (dspec, dev) in entries.items():
      dplan = dspec.plan(template0, scale, loc)
      dtemplate = dspec.template(template0)
      dscale, dloc = dspec.channel_stats(template0, scale, loc)
      if isinstance(dspec, verification.BandSpec):
        # a band view: a handle of its own (and a climatology view of its own) with the analysis tables of its band limit
        width, how = len(dplan["band"]), "band_plan"
        handle = den.band_handle(width, name)
        clim_view = None if clim_handle is None else den.climatology_handle(width, view=True, key="band:" + name)
        for h in (handle, clim_view):
          if h is not None:
            _spectra.ensure_tables(h, template0, dplan["response"].shape[1])
      else:
        width, how = len(dplan["op"]), "plan"
        handle = den.view_handle(width)
        clim_view = None if clim_handle is None else den.climatology_handle(width, view=True)
      store = verification.ScoredStore(handle, M, weights, events=dev,
                                       thresholds=None if dev is None else packed(dev, dtemplate, dscale, dloc), weight_q=wq,
                                       source=native, order=order, energy=eplan(dtemplate), variogram=vplan,
                                       climatology=clim_view, climatology_source=clim_handle, efi=efi, **{how: dplan},
                                       **map_args(name, dtemplate, horizon), **per_store_args(name, dtemplate, dscale, dloc))
      run.views[name] = _StoreSeries(store, dscale, dtemplate, keep_members=keep_members, keep_quantiles=keep_quantiles,
                                     keep_efi=keep_efi)
    for store in (v.store for v in run.views.values()):
      # entries of equal width share a handle: their plan and thresholds are then set again at every lead time
      store.set_per_score = sum(1 for v in run.views.values() if v.store.handle is store.handle) > 1
      if store.set_per_score and store.maps is not None:
        raise ValueError("maps: a derived entry that shares its handle with another of equal width cannot keep score maps -- "
                         "two views must not add into one accumulator")
      store.setup()

    for name, fspec in (features or {}).items():
      # a handle of its own per entry (it keeps the lists of its last call); the strike fields are 0 / 1: scale 1, location 0
      fplan, ftemplate, fev = fspec.plan(template0, scale, loc), fspec.template(template0), fspec.event_spec()
      fscale, floc = fspec.channel_stats(template0, scale, loc)
      store = verification.ScoredStore(den.feature_handle(len(fplan["channel"]), name), M, weights, events=fev,
                                       thresholds=fev.packed(ftemplate), weight_q=wq, feature_plan=fplan, source=native,
                                       order=order, **per_store_args(name, ftemplate, fscale, floc))
      run.features[name] = _StoreSeries(store, fscale, ftemplate, keep_members=keep_members, keep_quantiles=keep_quantiles)
      store.setup()

    for name, (wspec, wev) in wentries.items():
      # the source's channels, their statistics and their names; the window maps the statistics once more
      if wspec.source is None:
        source, stemplate, sscale, sloc = native, template0, scale, loc
      elif wspec.source in run.features:
        fspec = features[wspec.source]
        source, stemplate = run.features[wspec.source].store.handle, fspec.template(template0)
        sscale, sloc = fspec.channel_stats(template0, scale, loc)
      else:
        dspec = entries[wspec.source][0]
        source, stemplate = run.views[wspec.source].store.handle, dspec.template(template0)
        sscale, sloc = dspec.channel_stats(template0, scale, loc)
      wscale, wloc = wspec.channel_stats(sscale, sloc)
      store = verification.ScoredStore(den.window_handle(len(wscale), name), M, weights, events=wev,
                                       thresholds=None if wev is None else packed(wev, stemplate, wscale, wloc), weight_q=wq,
                                       order=order, energy=eplan(stemplate), variogram=vplan,
                                       **map_args(name, stemplate, len(wspec.leads(horizon))),
                                       **per_store_args(name, stemplate, wscale, wloc))
      run.windows[name] = _WindowEntry(wspec, _StoreSeries(store, wscale, stemplate, keep_members=keep_members), source, horizon)
      run.windows[name].start()
    return run

  @staticmethod
  def _sample_lead(run: "_EnsembleRun", k: int, forcings, horizon: int) -> None:
    """The member loop of lead time k: every member sampled from its own context, advanced, and its state pushed."""
    native, lanes, M, noise = run.native, run.lanes, run.M, run.noise
    frows = (run.rows_of(EnsembleRollout.next_forcings(forcings, k, horizon), run.forcing_cols, run.sizes, run.grid_shape)
             if run.plan["n_forcing"] else None)
    for g0 in range(0, M, len(lanes)):
      group = list(zip(lanes, range(g0, min(M, g0 + len(lanes)))))
      for lane, m in group:                               # enqueue only: every lane's sample is in flight after this
        native.ctx_load(m, dst=lane)
        if noise[m].key is not None:
          lane.noise_seed(noise[m].key, noise[m].stream)
        if run.on_device:
          lane.noise_draw()
        else:
          z = np.asarray(run.init_noise[m][k], np.float32) if run.given_noise else \
              noise[m].host_field(run.shape, run.template0)
          lane.upload_noise(z)
        lane.sample_resident(run.sigmas, skip_dead_call=True, want_stats=False)
        if noise[m].key is not None:
          noise[m].stream = lane.counter("noise_stream")   # churn fields drew too: the library is the one that knows
      for lane, m in group:
        lane.rollout_advance(frows)                       # resolves the lane's domain check, then advances ITS context
        native.ctx_save(m, src=lane)
        native.ens_push_state(m, run.state_src, src=lane)

  @staticmethod
  def _score_lead(run: "_EnsembleRun", k: int, targets) -> None:
    """Lead time k scored on the device: the main store against `targets[k]`, then every derived view, then the windows that
    end here (`_StoreSeries.score_lead` each)."""
    native, scale, loc = run.native, run.scale, run.loc
    tk = isel_time(targets, slice(k, k + 1))
    truth = _members_units(tk, run.shape, scale, loc, run.normalized)
    if run.main.store.set_per_score:
      run.main.store.thresholds = run.thresholds[k]

    def fields_and_spectra():
      if run.want_fields:
        mean, var = native.ens_download_fields()
        mean = (mean.astype(np.float64) * scale + loc).astype(np.float32)
        var = (var.astype(np.float64) * scale * scale).astype(np.float32)
        tmpl = tk.map(np.zeros_like)
        run.means.append(Denoiser.unpack_outputs(mean, run.grid_shape, tmpl))
        run.variances.append(Denoiser.unpack_outputs(var, run.grid_shape, tmpl))
      if run.want_spectra:
        run.raw_spectra.append(_spectra.EnsembleSpectra(native.ens_spectrum(None), run.M))   # the truth is on the device already
        run.spectra.append(run.raw_spectra[-1].scaled(scale))

    samples = None
    if "climatology" in run.main.lists:
      samples = list(run.climatology(k) if callable(run.climatology) else run.climatology[k])
      if not 2 <= len(samples) <= 64:
        raise ValueError(f"climatology of lead time {k}: 2..64 Datasets shaped like the targets, got {len(samples)}")
      samples = [_members_units(c, run.shape, scale, loc, run.normalized) for c in samples]
    run.main.score_lead(truth, want_fields=run.want_fields, after_score=fields_and_spectra, clim_fields=samples)
    for w in run.windows.values():
      if w.spec.source is None:
        w.push()
    for vname, v in run.views.items():
      # members and truth, device to device; the climatology: the samples in the main climatology handle's store, through the
      # view's plan -- that handle has no truth of its own
      v.score_lead(None, n_samples=None if samples is None else len(samples), source_truth=truth)
      for w in run.windows.values():                      # (two views may share a handle: the view's fields are there NOW)
        if w.spec.source == vname:
          w.push()
    for fname, f in run.features.items():
      # members and truth, device to device; then the lists of centres and the ensemble mean of the strike fields

      def centres_and_probability(f=f):
        f.centres.append(f.store.centres())
        mean = f.store.handle.ens_download_fields()[0]
        f.probabilities.append(Denoiser.unpack_outputs(mean, run.grid_shape, f.template))

      f.score_lead(None, want_fields=True, after_score=centres_and_probability)
      for w in run.windows.values():
        if w.spec.source == fname:
          w.push()
    for w in run.windows.values():
      w.finish_lead(k)
