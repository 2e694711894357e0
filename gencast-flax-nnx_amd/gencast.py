"""`GenCast`: the Predictor-like wrapper the rollout / evaluation harness calls.

Mirrors gencast/gencast.py:119-185,282-294: constructor signature
(task_config, denoiser_architecture_config, sampler_config, noise_config,
noise_encoder_config), `num_outputs` inference (:158-169), the sampler singleton
(:182-185), `__call__` and `full_sampling(inputs, targets_template, forcings)`.

Known reference defect NOT copied: `GenCast.__call__` forwards `forcings`
positionally into the denoiser's `noise_levels` slot (gencast.py:282-287 vs
denoiser.py:172-178).  Here `__call__` takes `noise_levels` explicitly.
`loss` / `loss_and_predictions` (gencast.py:221-280) keep raising NotImplementedError: training is out of scope.
The diffusion objective itself is available forward-only as `denoising_loss` /
`denoising_loss_and_predictions` (a harness that only evaluates may alias them: INTEGRATION.md).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, Optional

import numpy as np

from . import config as cfg
from . import datasets, losses
from .datasets import Dataset, Variable
from .denoiser import Denoiser
from .sampler import Sampler, rho_inverse_cdf


def _generator(rngs) -> np.random.Generator:
  """A numpy Generator from whatever `rngs` is, the way `Sampler` consumes it: a Generator is used (and advanced) as
  it is, an int seeds a fresh one, an object with `.noise()` seeds one from the key it hands out."""
  if rngs is None:
    raise ValueError("Must pass rngs (a numpy Generator, an int seed, or an object with .noise())")
  if isinstance(rngs, np.random.Generator):
    return rngs
  if isinstance(rngs, (int, np.integer)):
    return np.random.default_rng(int(rngs))
  if hasattr(rngs, "noise"):
    return np.random.default_rng(datasets.key_words(rngs.noise()).tolist())
  raise TypeError(f"unsupported rngs: {type(rngs)}")


def _base_seed(rngs) -> int:
  """The base seed of an ensemble: an int as it is, anything else through `Sampler.seed_from`."""
  return int(rngs if isinstance(rngs, (int, np.integer)) else Sampler.seed_from(rngs))


class GenCast:

  def __init__(self,
               task_config: cfg.TaskConfig,
               denoiser_architecture_config: cfg.DenoiserArchitectureConfig,
               sampler_config: Optional[cfg.SamplerConfig] = None,
               noise_config: Optional[cfg.NoiseConfig] = None,
               noise_encoder_config: Optional[cfg.NoiseEncoderConfig] = None,
               gpu_mesh=None,
               rngs=0,
               *,
               params: Optional[Dict[str, np.ndarray]] = None,
               device_id: int = 0,
               graph=None,
               options: Optional[Dict[str, str]] = None):
    """Positional order as gencast/gencast.py:145-154 (`..., noise_encoder_config, gpu_mesh, rngs`).  `gpu_mesh`
    (the reference's jax device mesh) is accepted and ignored: one GenCast drives one GPU, ensemble members are
    spread over GPUs by `EnsembleSampler` / `launch.py`.  `rngs`: an int seed, a numpy Generator, or an
    nnx.Rngs-like object whose `.noise()` returns key words (kept as it is: the sampler draws its keys from it)."""
    del gpu_mesh
    self.task_config = task_config
    if isinstance(rngs, np.random.Generator) or hasattr(rngs, "noise"):
      self.rngs = rngs
    else:
      self.rngs = np.random.default_rng(rngs)
    denoiser_architecture_config = dataclasses.replace(
        denoiser_architecture_config, node_output_size=cfg.num_outputs(task_config))
    self.denoiser = Denoiser(noise_encoder_config, denoiser_architecture_config, params,
                             device_id=device_id, graph=graph, options=options)
    self._sampler_config = sampler_config or cfg.SamplerConfig()
    self._noise_config = noise_config
    self._sampler = Sampler(self.denoiser, **dataclasses.asdict(self._sampler_config))

  def __call__(self, inputs, targets_template, noise_levels, forcings=None, **kwargs):
    """One raw denoiser evaluation (`targets_template` plays the noisy targets)."""
    return self.denoiser(inputs, targets_template, noise_levels, forcings, **kwargs)

  def full_sampling(self, inputs, targets_template, forcings=None, **kwargs):
    """gencast/gencast.py:289-294."""
    return self._sampler(inputs, targets_template, forcings, rngs=self.rngs, **kwargs)

  def as_predictor_fn(self):
    """`PredictorFn(rng, inputs, targets_template, forcings)` (common/rollout.py:29-38): the functional form
    `chunked_prediction_generator` calls (:345-349).  `rng`: a numpy Generator, an int seed, or an object
    with `.noise()` returning key words (the reference passes a jax PRNG key / nnx.Rngs stream)."""
    def predictor_fn(rng, inputs, targets_template, forcings, **optional_kwargs):
      return self._sampler(inputs, targets_template, forcings, rngs=rng, **optional_kwargs)
    return predictor_fn

  def _ensemble_sampler(self, rngs, concurrent_members):
    """The `EnsembleSampler` of the `ensemble_*` methods: all members on this rank, `rngs` as the base seed."""
    from .ensemble import EnsembleSampler  # pylint: disable=import-outside-toplevel
    return EnsembleSampler(self._sampler, base_seed=_base_seed(rngs), concurrent_members=concurrent_members)

  def ensemble_scores(self, inputs, targets, forcings=None, *, num_members, rngs=0, concurrent_members=1, fields=False):
    """Samples `num_members` (2..64) members for (inputs, forcings) and scores them against `targets` on the GPU:
    `verification.EnsembleScores` (CRPS, RMSE of the ensemble mean, spread, rank histogram, per batch member and
    channel, latitude-weighted), with `fields=True` also the ensemble mean and variance as Datasets.  No member
    leaves the device.  `rngs`: the base seed of the members' noise streams (`ensemble.member_seed`), so member m
    is the member m of `EnsembleSampler(base_seed=rngs)`; `concurrent_members` as there."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.scores(inputs, targets, forcings, num_members, fields=fields)

  def ensemble_spectra(self, inputs, targets, forcings=None, *, num_members, rngs=0, concurrent_members=1, lmax=None,
                       scores=False):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and analyses them against `targets` on the GPU:
    `spectra.EnsembleSpectra` -- spherical-harmonic power per total wavenumber l < `lmax` (default n_lon / 2) of the
    truth, the members, the ensemble mean, their errors and the spread, per batch member and channel.  No member
    leaves the device.  `scores=True`: -> (EnsembleScores, EnsembleSpectra) from the same members, sampled once."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    if scores:
      return runner.scores_and_spectra(inputs, targets, forcings, num_members, lmax=lmax)
    return runner.spectra(inputs, targets, forcings, num_members, lmax=lmax)

  def ensemble_events(self, inputs, targets, forcings=None, *, num_members, spec, rngs=0, concurrent_members=1):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and counts the events of `spec`
    (`verification.EventSpec`: thresholds per variable in the units of `targets`, a direction per event) among them and
    in `targets`, on the GPU: `verification.EventScores` -- Brier score with its decomposition, reliability curve, ROC
    area, relative economic value, per event, batch member and channel.  No member leaves the device."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.events(inputs, targets, forcings, num_members, spec)

  def ensemble_tails(self, inputs, targets, forcings=None, *, num_members, spec, rngs=0, concurrent_members=1):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and forms on the GPU the threshold-weighted CRPS
    (Gneiting & Ranjan 2011) at the thresholds of `spec` (`verification.EventSpec`: thresholds per variable in the units of
    `targets`; direction > 0: the upper tail, weight 1{z >= threshold}, < 0: the lower tail): `verification.TailScores` --
    `.twcrps` (fair), `.twcrps_ensemble`, `.abs_error`, `.pair_distance`, `.base_rate` per threshold, batch member and
    channel, latitude-weighted.  The members of a point are sorted once for all thresholds.  No member leaves the device."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.tails(inputs, targets, forcings, num_members, spec)

  def ensemble_maps(self, inputs, targets, forcings=None, *, num_members, spec, events=None, rngs=0, concurrent_members=1):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and forms on the GPU the score maps of this date:
    `verification.ScoreMaps` -- per grid point and per channel of `spec` (`verification.MapSpec`) the raw planes from which
    `.bias`, `.rmse`, `.spread_skill_ratio`, `.crps`, `.crps_stderr`, `.outlier_low` / `.outlier_high` follow; the planes of
    several dates add (`ScoreMaps.merge`), and any region chosen afterwards is a weighted sum of them (`.region`).  With
    `MapSpec(events=True)` and `events` (an `EventSpec`) -> (ScoreMaps, `verification.EventMaps`: per-point Brier score, base
    rate and forecast probability).  No member leaves the device."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.maps(inputs, targets, forcings, num_members, spec, events)

  def ensemble_regions(self, inputs, targets, forcings=None, *, num_members, spec, rngs=0, concurrent_members=1):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and forms on the GPU the sums of `ensemble_scores` for
    every region of `spec` (`verification.RegionSpec`: named boolean masks over the grid, overlapping or not) from ONE pass
    over the nodes that belong to any region: `verification.RegionScores`, whose `[name]` is an `EnsembleScores` -- `.crps`,
    `.rmse`, `.spread_skill_ratio`, `.rank_histogram` of that region, latitude-weighted.  No member leaves the device."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.regions(inputs, targets, forcings, num_members, spec)

  def ensemble_order(self, inputs, targets, forcings=None, *, num_members, probs=(), quantile_fields=False, rngs=0,
                     concurrent_members=1):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and sorts them point by point on the GPU:
    `verification.OrderScores` -- the ensemble CRPS split into its reliability and potential parts (Hersbach 2000), the
    outlier frequencies, and for the probabilities `probs` (at most 8) the pinball loss and coverage of the quantile
    fields -- per batch member and channel, latitude-weighted.  `quantile_fields=True`: -> (OrderScores, [Q Datasets]),
    the quantile fields (median, p10 / p90 band) shaped like `targets`.  No member leaves the device.  The uncertainty and
    resolution parts of Hersbach's decomposition need a climatology of the observations and are not formed."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.order(inputs, targets, forcings, num_members, probs, quantile_fields=quantile_fields)

  def ensemble_multivariate(self, inputs, targets, forcings=None, *, num_members, energy=None, variogram=None, rngs=0,
                            concurrent_members=1):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and forms on the GPU the two standard proper scores of
    a joint forecast, which no marginal score sees: with `energy` (`verification.EnergySpec`: groups of variables, e.g. the
    two wind components, or a whole field) the energy score of every group, with `variogram` (`verification.VariogramSpec`:
    grid offsets and an order p) the variogram score per batch member, channel and offset, latitude-weighted.
    -> (`verification.EnergyScores` or None, `verification.VariogramScores` or None).  No member leaves the device."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.multivariate(inputs, targets, forcings, num_members, energy, variogram)

  def ensemble_climatology(self, inputs, targets, forcings=None, *, num_members, climatology, rngs=0, concurrent_members=1):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and scores them on the GPU against `climatology`,
    K (2..64) Datasets shaped like `targets` (past states for the same calendar date; a climatological mean is given
    twice): `verification.ClimatologyScores` -- the anomaly correlation coefficient of the ensemble mean (`acc`), the CRPS
    skill score against the climatological ensemble (`crpss`), `msss` -- per batch member and channel, latitude-weighted.
    No member leaves the device."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.climatology(inputs, targets, forcings, num_members, climatology)

  def ensemble_efi(self, inputs, targets, forcings=None, *, num_members, climatology, spec=None, fields=True, rngs=0,
                   concurrent_members=1):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and ranks them on the GPU, point by point, in
    `climatology` (K Datasets, as in `ensemble_climatology`): the Extreme Forecast Index (Lalaurette 2003), in [-1, 1], how
    far the forecast distribution is shifted against the climatological one, weighted towards the tails.
    -> (`verification.EfiScores`, EFI Dataset, observed-index Dataset); `fields=False`: the scores alone.  `spec`: a
    `verification.EfiSpec` (the climatological events of `targets` the index is verified against, the EFI bins).
    `targets=None` -- a real forecast, no analysis yet -- gives the EFI Dataset alone.  No member leaves the device."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.efi(inputs, targets, forcings, num_members, climatology, spec, fields)

  def ensemble_derived(self, inputs, targets, forcings=None, *, num_members, spec, events=None, rngs=0, concurrent_members=1):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and scores, on the GPU, what `spec`
    (`verification.DerivedSpec`) makes of them and of `targets`: wind speed from two components, fields max-, min- or
    mean-pooled over a neighbourhood; or what a `verification.BandSpec` makes of them: every variable low-, band- or
    high-pass filtered per total wavenumber.  -> `verification.EnsembleScores` over the derived channels, with `events` (an
    `EventSpec` keyed by the derived names) -> (EnsembleScores, EventScores).  No member leaves the device.  The members
    are taken in the units they are sampled in; the normalisation wrappers have no such method, because under them a
    single-step sample is a normalised residual and the norm of two residuals is no wind speed (`ensemble_rollout(...,
    derived=...)` derives from member states instead)."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.derived(inputs, targets, forcings, num_members, spec, events)

  def ensemble_features(self, inputs, targets, forcings=None, *, num_members, spec, rngs=0, concurrent_members=1):
    """Samples `num_members` (2..64) members as `ensemble_scores` does and finds, on the GPU, the features of `spec`
    (`verification.FeatureSpec`: named detectors, each a local minimum or maximum of one variable over a great-circle
    radius, with a threshold and a closed-contour depth test) in every member and in `targets`:
    `verification.FeatureScores` -- `.centres` / `.truth_centres` (lat, lon, value per member and of the truth),
    `.strike_probability` (the fraction of members with a centre within the strike radius of a place, a Dataset), `.scores`
    (the `EnsembleScores` of the 0 / 1 strike fields) and `.events` (their `EventScores` at 0.5: Brier score, reliability,
    ROC area, economic value of the strike probability).  Only the lists and the map leave the device.  The members are
    taken in the units they are sampled in, as in `ensemble_derived`; under `InputsAndResiduals` a single-step sample is a
    normalised residual, and that wrapper detects on the member STATES of a one-step `ensemble_rollout` instead."""
    runner = self._ensemble_sampler(rngs, concurrent_members)
    return runner.features(inputs, targets, forcings, num_members, spec)

  def ensemble_rollout(self, inputs, targets, forcings, horizon, num_members, *, rngs=0, norm=None, concurrent_members=1,
                       device_noise=None, **kwargs):
    """Rolls `num_members` (2..64) members out `horizon` autoregressive steps with every member's context resident on
    the GPU and scores their states against `targets[k]` at every lead time: `rollout.EnsembleRolloutResult` (per lead
    time `EnsembleScores`, with `spectra=True` also `EnsembleSpectra`, with `fields=True` the mean and variance, with
    `events=EventSpec` also `EventScores`, with `tails=EventSpec` also `TailScores`, with `regions=RegionSpec` also
    `RegionScores`).  No
    member leaves the device.  `rngs`: the base seed (member m is `DeviceRollout(...).run(rngs=member_seed(rngs, m))`);
    `norm`: an `InputsAndResiduals` whose statistics apply (its own `ensemble_rollout` passes itself); `device_noise`
    defaults to the sampler's; other keywords as `rollout.EnsembleRollout.run`."""
    from .rollout import EnsembleRollout  # pylint: disable=import-outside-toplevel
    runner = EnsembleRollout(self, norm, self.task_config, base_seed=_base_seed(rngs), concurrent_members=concurrent_members,
                             device_noise=self._sampler.device_noise if device_noise is None else device_noise)
    return runner.run(inputs, targets, forcings, horizon, num_members, **kwargs)

  # -- the diffusion objective, forward only -----------------------------------------------------------------
  def _denoising_eval(self, inputs, targets, forcings, rngs, noise_levels, noise, num_noise_draws, per_variable_weights):
    """-> (loss [K, B], per_variable [K, B, V], names, D [G, B, c_out] of the last draw, grid_shape, targets Dataset)."""
    inputs, targets, forcings = (datasets.as_dataset(x) for x in (inputs, targets, forcings))
    if noise_levels is None and self._noise_config is None:
      raise ValueError("Noise config must be specified to train GenCast.")
    draws = 1 if num_noise_draws is None else int(num_noise_draws)
    if draws < 1:
      raise ValueError("num_noise_draws must be >= 1")
    cond, grid_shape, slots = self.denoiser.init_for(inputs, targets, forcings)
    native = self.denoiser.native
    native.set_noisy_slots(slots)
    batch = cond.shape[1]
    shape = (cond.shape[0], batch, self.denoiser.dims.c_out)
    stacked = np.transpose(datasets.dataset_to_stacked(targets, targets.sizes), (1, 2, 0, 3))
    plan = losses.loss_plan(targets, per_variable_weights)
    native.loss_set_weights(plan.node_weight, plan.channel_weight, plan.channel_group, plan.group_weight)
    native.upload_cond(cond)
    native.upload_targets(stacked.reshape(shape))
    if noise_levels is not None:
      sigmas = np.asarray(getattr(noise_levels, "data", noise_levels), dtype=np.float32)
      sigmas = sigmas.reshape(1, -1) if sigmas.ndim == 1 else sigmas
      if sigmas.shape != (draws, batch):
        raise ValueError("noise_levels expected to be shape (batch,).")
    gen = None
    if noise_levels is None or noise is None:
      gen = _generator(self.rngs if rngs is None else rngs)
    if noise is not None:
      noise = np.asarray(noise, dtype=np.float32)
      if noise.shape != shape:
        raise ValueError(f"noise must have shape {shape}")
    nc = self._noise_config
    sampler = self._sampler
    on_device = noise is None and sampler.device_noise and sampler.noise_kind != "white"
    loss = np.empty((draws, batch), np.float32)
    per_var = np.empty((draws, batch, len(plan.names)), np.float32)
    if on_device:                       # every draw a fresh device field: ONE native call for all of them
      sampler.ensure_device_noise(native, targets)
      native.noise_seed(sampler.seed_from(gen), 0)      # the key first, then the levels: draw 0 is the single call's draw
      if noise_levels is None:
        sigmas = np.stack([rho_inverse_cdf(nc.training_min_noise_level, nc.training_max_noise_level, nc.training_noise_level_rho,
                                           gen.random(batch, dtype=np.float32)) for _ in range(draws)]).astype(np.float32)
      loss, per_var = native.loss_resident(sigmas, draw_noise=True)
    else:
      for k in range(draws):            # per draw: noise levels first, then the field (the reference's order, gencast.py:238-253)
        if noise_levels is None:
          sg = rho_inverse_cdf(nc.training_min_noise_level, nc.training_max_noise_level, nc.training_noise_level_rho,
                               gen.random(batch, dtype=np.float32)).astype(np.float32)
        else:
          sg = sigmas[k]
        native.upload_noise(noise if noise is not None else sampler.draw_noise(gen, shape, targets))
        loss[k], per_var[k] = (a[0] for a in native.loss_resident(sg))
    return loss, per_var, plan.names, native, grid_shape, targets

  @staticmethod
  def _loss_outputs(loss, per_var, names, squeeze, given):
    dims = ("batch",) if squeeze else ("draw", "batch")
    if squeeze:
      loss, per_var = loss[0], per_var[0]
    total = Variable(dims, loss)
    diagnostics = Dataset({name: Variable(dims, np.ascontiguousarray(per_var[..., g])) for g, name in enumerate(names)})
    return datasets.loss_like_inputs(total, diagnostics, *given)

  def denoising_loss(self, inputs, targets, forcings=None, *, rngs=None, noise_levels=None, noise=None,
                     num_noise_draws=None, per_variable_weights=None):
    """The value of `GenCast.loss` (gencast/gencast.py:229-280), evaluated forward-only on the GPU: per batch member
    a noise level sigma, x = targets + sigma * noise, the preconditioned denoiser D(x; sigma), the latitude- and
    level-weighted MSE of D against the targets summed over variables (`losses.DEFAULT_PER_VARIABLE_WEIGHTS`) and times
    lambda(sigma) = c_out(sigma)^-2.  Returns (loss, diagnostics) with dims ('batch',): diagnostics are the unweighted
    per-variable means.

    `noise_levels` [batch]: given levels; None draws them as rho_inverse_cdf(NoiseConfig, uniform) from `rngs` (from
    `self.rngs` when that is None too), consumed the way `Sampler` consumes it.  `noise` [G, batch, c_out]: a given
    unit-variance field; None draws spherical white noise on a qualifying grid, else white noise (`Sampler.draw_noise`;
    on the device with the sampler's `device_noise`).  The reference's random stream (jax's `uniform`, dinosaur's
    coefficient order) is not reproduced, as for sampling: equal `rngs` give equal results HERE.
    `num_noise_draws=K` evaluates K independent (levels, field) draws on the conditioning and targets uploaded once and
    returns dims ('draw', 'batch') (`validation_loss`)."""
    loss, per_var, names, *_ = self._denoising_eval(inputs, targets, forcings, rngs, noise_levels, noise, num_noise_draws,
                                                    per_variable_weights)
    return self._loss_outputs(loss, per_var, names, num_noise_draws is None, (targets, inputs, forcings))

  def denoising_loss_and_predictions(self, inputs, targets, forcings=None, *, rngs=None, noise_levels=None, noise=None,
                                     num_noise_draws=None, per_variable_weights=None):
    """((loss, diagnostics), predictions) with predictions = the preconditioned D(x; sigma) of THAT evaluation (of the
    last draw with `num_noise_draws`).  The reference's `loss_and_predictions` (gencast.py:221-227) takes its
    predictions from a second call through its `__call__`, which passes `forcings` where the denoiser expects noise
    levels -- the defect this module already declines to copy -- so there is no reference value to match; D is what
    the loss was computed from."""
    loss, per_var, names, native, grid_shape, tds = self._denoising_eval(
        inputs, targets, forcings, rngs, noise_levels, noise, num_noise_draws, per_variable_weights)
    preds = Denoiser.unpack_outputs(native.download_denoised(), grid_shape, tds)
    given = (targets, inputs, forcings)
    return self._loss_outputs(loss, per_var, names, num_noise_draws is None, given), datasets.like_inputs(preds, *given)

  def loss(self, *args, **kwargs):
    raise NotImplementedError("training (loss) is outside the sampling hot path; the forward-only value of the "
                              "objective is GenCast.denoising_loss / denoising_loss_and_predictions")

  loss_and_predictions = loss


def compute_loss(model, inputs, targets, forcings=None, **kwargs):
  """training/train_helpers.py:221-236: (mean loss over the batch, {variable: batch mean}) of `model.denoising_loss`."""
  loss, diagnostics = model.denoising_loss(inputs, targets, forcings, **kwargs)
  vals = lambda v: np.asarray(getattr(v, "values", getattr(v, "data", v)), dtype=np.float64)
  return float(vals(loss).mean()), {k: float(vals(diagnostics[k]).mean()) for k in diagnostics.keys()}


def validation_loss(model, batches, noise_levels_per_batch: int = 1, rngs=0):
  """A checkpoint's validation loss (what training/train_helpers.py:276-290 `eval_step_packed` is looped for): for every
  (inputs, targets, forcings) of `batches` the conditioning and targets go up once and `noise_levels_per_batch`
  independent (noise levels, noise field) draws are evaluated on them (`gc_loss_resident`).  `model`: a `GenCast` or a
  wrapper stack around one.  Returns (mean loss, {variable: mean}) over all batches, draws and batch members.  One
  generator made from `rngs` runs through all of them.  With host-drawn noise (the default) the result equals the mean of
  the single `denoising_loss(..., rngs=generator)` calls in the same order; with the sampler's `device_noise` a batch's K
  draws are ONE native call on Philox streams 0..K-1 of one key (draw 0 is what a single call would draw, the others
  are not)."""
  gen = _generator(rngs)
  total, per_var, count = 0.0, {}, 0
  for inputs, targets, forcings in batches:
    loss, diagnostics = model.denoising_loss(inputs, targets, forcings, rngs=gen, num_noise_draws=int(noise_levels_per_batch))
    vals = lambda v: np.asarray(getattr(v, "values", getattr(v, "data", v)), dtype=np.float64)
    total += float(vals(loss).sum())
    count += vals(loss).size
    for k in diagnostics.keys():
      per_var[k] = per_var.get(k, 0.0) + float(vals(diagnostics[k]).sum())
  if count == 0:
    raise ValueError("validation_loss: no batches")
  return total / count, {k: v / count for k, v in per_var.items()}


def create_gencast_model(task_config: cfg.TaskConfig = cfg.TASK, *, mesh_size: int = 3,
                         d_model: int = 256, num_layers: int = 2, num_heads: int = 4,
                         stochastic_churn_rate: float = 0.0, params=None, rngs=0,
                         device_id: int = 0) -> GenCast:
  """training/train_helpers.py:94-158 (defaults included)."""
  sampler_config = cfg.SamplerConfig(max_noise_level=80.0, min_noise_level=0.03,
                                     num_noise_levels=20, rho=7.0,
                                     stochastic_churn_rate=float(stochastic_churn_rate))
  arch = cfg.nano_architecture(mesh_size=mesh_size, d_model=d_model, num_layers=num_layers,
                               num_heads=num_heads)
  return GenCast(task_config, arch, sampler_config, cfg.NoiseConfig(), None, params=params,
                 rngs=rngs, device_id=device_id)
