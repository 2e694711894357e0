"""`NaNCleaner`: predictor wrapper that fills NaNs of one variable before the wrapped predictor sees
them and (optionally) puts them back into the predictions.

Mirrors gencast/nan_cleaning.py:27-156 (`__call__`, `full_sampling`; `loss` is training-only, its forward-only
value is `denoising_loss` / `denoising_loss_and_predictions`, :87-126).  With
this repo's TASK the cleaned variable (`sea_surface_temperature`, training/train_helpers.py:170-178)
is absent, so the wrapper is a pass-through at run time -- it exists so that the reference's model
stack `NaNCleaner(InputsAndResiduals(GenCast))` can be assembled unchanged.  It also keeps NaNs
(land points of SST) away from the f16x3 domain guard, which would otherwise re-run every call in f32.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import datasets
from .datasets import Dataset, Variable


class NaNCleaner:

  def __init__(self, predictor, var_to_clean: str, fill_value, reintroduce_nans: bool = False):
    self.predictor = predictor
    fv = datasets.as_dataset(fill_value)[var_to_clean]
    self._fill_value = fv
    self._var_to_clean = var_to_clean
    self._reintroduce_nans = reintroduce_nans

  def _clean(self, dataset: Dataset) -> Dataset:
    """nan_cleaning.py:52-58: `data_array.fillna(fill_value)` with xarray broadcasting by dim name."""
    var = dataset[self._var_to_clean]
    fill = np.asarray(self._fill_value.data, dtype=var.data.dtype)
    shape = [1] * len(var.dims)
    for d, n in zip(self._fill_value.dims, fill.shape):
      if d not in var.dims:
        raise ValueError(f"fill value dimension {d!r} is not a dimension of {self._var_to_clean!r}")
      shape[var.dims.index(d)] = n
    order = sorted(range(len(self._fill_value.dims)), key=lambda i: var.dims.index(self._fill_value.dims[i]))
    fill = np.transpose(fill, order).reshape(shape) if fill.ndim else fill
    data = np.where(np.isnan(var.data), fill, var.data)
    return dataset.assign(Dataset({self._var_to_clean: Variable(var.dims, data)}))

  def _maybe_reintroduce_nans(self, stale_inputs: Dataset, predictions: Dataset) -> Dataset:
    """nan_cleaning.py:60-69: NaN where ANY input frame was NaN."""
    if self._var_to_clean in predictions.keys() and self._var_to_clean in stale_inputs.keys():
      src = stale_inputs[self._var_to_clean]
      mask = np.isnan(src.data)
      dims = list(src.dims)
      if "time" in dims:
        mask = mask.any(axis=dims.index("time"))
        dims.remove("time")
      pred = predictions[self._var_to_clean]
      shape = [1] * len(pred.dims)
      for d, n in zip(dims, mask.shape):
        shape[pred.dims.index(d)] = n
      order = sorted(range(len(dims)), key=lambda i: pred.dims.index(dims[i]))
      m = np.transpose(mask, order).reshape(shape)
      predictions = predictions.assign(Dataset(
          {self._var_to_clean: Variable(pred.dims, np.where(m, np.nan, pred.data).astype(pred.data.dtype))}))
    return predictions

  def _wrap(self, fn, inputs, targets_template, forcings, **kwargs):
    given = (targets_template, inputs, forcings)            # xarray in -> xarray out (datasets.like_inputs)
    inputs = datasets.as_dataset(inputs)
    forcings = None if forcings is None else datasets.as_dataset(forcings)
    original = inputs if self._reintroduce_nans else None
    if self._var_to_clean in inputs.keys():
      inputs = self._clean(inputs)
    if forcings is not None and self._var_to_clean in forcings.keys():
      forcings = self._clean(forcings)
    preds = datasets.as_dataset(fn(inputs, targets_template, forcings, **kwargs))
    if self._reintroduce_nans:
      preds = self._maybe_reintroduce_nans(original, preds)
    return datasets.like_inputs(preds, *given)

  def __call__(self, inputs, targets_template, forcings=None, **kwargs):
    return self._wrap(self.predictor, inputs, targets_template, forcings, **kwargs)

  def full_sampling(self, inputs, targets_template, forcings: Optional[Dataset] = None, **kwargs):
    return self._wrap(self.predictor.full_sampling, inputs, targets_template, forcings, **kwargs)

  def _cleaned(self, inputs, targets, forcings, clean_targets: bool):
    """Inputs and forcings as Datasets with the variable cleaned; the targets as a Dataset, cleaned only when asked."""
    inputs, targets = datasets.as_dataset(inputs), datasets.as_dataset(targets)
    forcings = None if forcings is None else datasets.as_dataset(forcings)
    if self._var_to_clean in inputs.keys():
      inputs = self._clean(inputs)
    if clean_targets and self._var_to_clean in targets.keys():
      targets = self._clean(targets)
    if forcings is not None and self._var_to_clean in forcings.keys():
      forcings = self._clean(forcings)
    return inputs, targets, forcings

  def _clean_all(self, inputs, targets, forcings):
    return self._cleaned(inputs, targets, forcings, True)

  def denoising_loss(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """nan_cleaning.py:87-102 on the forward-only objective: inputs, targets and forcings are cleaned."""
    out = self.predictor.denoising_loss(*self._clean_all(inputs, targets, forcings), **kwargs)
    return datasets.loss_like_inputs(*out, targets, inputs, forcings)

  def denoising_loss_and_predictions(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """nan_cleaning.py:104-126: as above; NaNs go back into the predictions when `reintroduce_nans`."""
    given = (targets, inputs, forcings)
    original = datasets.as_dataset(inputs)
    loss, preds = self.predictor.denoising_loss_and_predictions(*self._clean_all(inputs, targets, forcings), **kwargs)
    preds = datasets.as_dataset(preds)
    if self._reintroduce_nans:
      preds = self._maybe_reintroduce_nans(original, preds)
    return datasets.loss_like_inputs(*loss, *given), datasets.like_inputs(preds, *given)

  def ensemble_scores(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned; the targets pass through unchanged: their NaNs (land points of the cleaned
    variable) are the points the device skips, so the scores are over the valid points only."""
    given = (targets, inputs, forcings)
    out = self.predictor.ensemble_scores(*self._cleaned(inputs, targets, forcings, False), **kwargs)
    if not isinstance(out, tuple):
      return out
    return (out[0],) + tuple(datasets.like_inputs(datasets.as_dataset(f), *given) for f in out[1:])

  def ensemble_order(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned; the targets pass through unchanged, as in `ensemble_scores`: their NaNs are
    points the device does not count.  The quantile fields need no truth and are finite there."""
    given = (targets, inputs, forcings)
    out = self.predictor.ensemble_order(*self._cleaned(inputs, targets, forcings, False), **kwargs)
    if not isinstance(out, tuple):
      return out
    return out[0], [datasets.like_inputs(datasets.as_dataset(f), *given) for f in out[1]]

  def ensemble_multivariate(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned; the targets pass through unchanged, as in `ensemble_scores`: their NaNs are
    points the device skips (`EnergyScores.invalid`) and ends of pairs it does not count."""
    return self.predictor.ensemble_multivariate(*self._cleaned(inputs, targets, forcings, False), **kwargs)

  def ensemble_climatology(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned; the targets and the climatology pass through unchanged: their NaNs are points
    the device does not count (`ClimatologyScores.invalid`)."""
    return self.predictor.ensemble_climatology(*self._cleaned(inputs, targets, forcings, False), **kwargs)

  def ensemble_efi(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned; the targets (None: a forecast without an analysis) and the climatology pass through
    unchanged: their NaNs are points the device does not count (`EfiScores.invalid`) and NaNs of both index fields."""
    inputs, _, forcings = self._cleaned(inputs, inputs if targets is None else targets, forcings, False)
    return self.predictor.ensemble_efi(inputs, targets, forcings, **kwargs)

  def ensemble_events(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned; the targets pass through unchanged, as in `ensemble_scores`: their NaNs are
    points the device does not count (`EventScores.invalid`)."""
    return self.predictor.ensemble_events(*self._cleaned(inputs, targets, forcings, False), **kwargs)

  def ensemble_tails(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned; the targets pass through unchanged, as in `ensemble_scores`: their NaNs are
    points the device does not count (`TailScores.invalid`)."""
    return self.predictor.ensemble_tails(*self._cleaned(inputs, targets, forcings, False), **kwargs)

  def ensemble_maps(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned; the targets pass through unchanged, as in `ensemble_scores`: their NaNs are
    points that add nothing to any plane (`ScoreMaps.valid_dates` is 0 there)."""
    return self.predictor.ensemble_maps(*self._cleaned(inputs, targets, forcings, False), **kwargs)

  def ensemble_regions(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned; the targets pass through unchanged, as in `ensemble_scores`: their NaNs are
    points the device does not count (`RegionScores.invalid`, per region)."""
    return self.predictor.ensemble_regions(*self._cleaned(inputs, targets, forcings, False), **kwargs)

  def ensemble_features(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned; the targets pass through unchanged, as in `ensemble_scores`: a NaN of the detection
    variable is a node that is no centre, is skipped as a neighbour, and is NaN in the strike field (a point the scorers do
    not count)."""
    given = (targets, inputs, forcings)
    out = self.predictor.ensemble_features(*self._cleaned(inputs, targets, forcings, False), **kwargs)
    if out.strike_probability is not None:
      out.strike_probability = datasets.like_inputs(datasets.as_dataset(out.strike_probability), *given)
    return out

  def ensemble_spectra(self, inputs, targets, forcings: Optional[Dataset] = None, **kwargs):
    """Inputs and forcings are cleaned, and so are the targets: a transform cannot skip points, so the spectrum of the
    cleaned variable is that of the field with its NaNs (land points) replaced by the fill value, truth and members
    alike."""
    return self.predictor.ensemble_spectra(*self._clean_all(inputs, targets, forcings), **kwargs)

  def ensemble_rollout(self, inputs, targets, forcings, horizon, num_members, **kwargs):
    """Inputs and forcings are cleaned.  The targets pass through unchanged (their NaNs are the points the device
    skips) unless `spectra=True`: a transform cannot skip points, so they are then cleaned too, as `ensemble_spectra`
    does, and the scores of the same call are over the filled field."""
    given = (targets, inputs, forcings)
    cleaned = self._cleaned(inputs, targets, datasets.as_dataset(forcings), bool(kwargs.get("spectra")))
    out = self.predictor.ensemble_rollout(*cleaned, horizon, num_members, **kwargs)
    if out.mean is not None and any(datasets.is_xarray(g) for g in given):   # xarray in -> xarray out
      like = given[0].isel(time=slice(0, horizon)) if datasets.is_xarray(given[0]) else None
      out.mean, out.variance = (datasets.to_xarray(datasets.as_dataset(f), like) for f in (out.mean, out.variance))
    return out

  def loss(self, *args, **kwargs):
    raise NotImplementedError("training (loss) is outside the sampling hot path; the forward-only value of the "
                              "objective is denoising_loss / denoising_loss_and_predictions")

  loss_and_predictions = loss
