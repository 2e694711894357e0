"""MI355X-native GenCast denoiser + DPM-Solver++2S sampling path.

Python host code -> ctypes -> `libgencast_hip.so` (C ABI, include/gencast_hip.h)
-> hand-written HIP kernels for gfx950.  No PyTorch / JAX / Triton in here.
Import as `gencast_flax_nnx_amd` (alias module at the repo root).

Public surface (mirrors the reference's call contracts):
  Denoiser            gencast/denoiser.py:142-202, gencast/denoisers_base.py:28-52
  Sampler             gencast/dpm_solver_plus_plus_2s.py:21-177
  GenCast             gencast/gencast.py:119-185,282-294  (full_sampling); :229-280 forward-only as denoising_loss
  losses              common/losses.py:58-187 (weighted_mse_per_level; loss_plan = its flat form for the device)
  compute_loss, validation_loss   training/train_helpers.py:221-236,276-290 (evaluation side)
  EnsembleSampler     common/rollout.py:78-176 (members sharded one per GPU)
  verification        EnsembleScores: CRPS, RMSE, spread, rank histogram from sums reduced on the GPU (no reference
                      counterpart: GenCast.ensemble_scores / EnsembleSampler.scores)
  spectra             SphericalAnalysis, EnsembleSpectra: spherical-harmonic power per total wavenumber of a sample or an
                      ensemble, analysed on the GPU (no reference counterpart: GenCast.ensemble_spectra)
                      DerivedSpec: wind speed and spatially pooled fields formed on the GPU in front of every scorer
                      (GenCast.ensemble_derived, EnsembleRollout.run(derived=...))
                      OrderScores: quantile fields and the reliability / potential split of the CRPS from members sorted
                      on the GPU (GenCast.ensemble_order, EnsembleRollout.run(order=...))
                      ClimatologyScores: anomaly correlation and CRPS skill score of an ensemble against K climatological
                      samples held by a second handle (GenCast.ensemble_climatology, EnsembleRollout.run(climatology=...))
                      EfiSpec / EfiScores: the Extreme Forecast Index -- the members ranked, on the GPU, in the K samples of
                      that second handle -- and its verification (GenCast.ensemble_efi, EnsembleRollout.run(efi=...))
                      WindowSpec: accumulations, means, changes and extremes over the last lead times of a rollout, formed
                      on the GPU from a ring of member stores (EnsembleRollout.run(windows=...))
                      EnergySpec / VariogramSpec: the energy score over groups of variables and the variogram score over
                      grid offsets, from pair sums formed on the GPU (GenCast.ensemble_multivariate,
                      EnsembleRollout.run(energy=..., variogram=...))
                      TailScores: the threshold-weighted CRPS at the thresholds of an EventSpec, from members sorted once
                      per point on the GPU (GenCast.ensemble_tails, EnsembleRollout.run(tails=...))
                      FractionsScores: the fractions skill score of the neighbourhood ensemble probability at the
                      `scales_km` of an EventSpec, from the event codes on the GPU (`EventScores.fractions`)
                      RegionSpec / RegionScores: the ensemble scores per region of the grid (tropics, extratropics, land,
                      sea, boxes), every region from one pass on the GPU (GenCast.ensemble_regions,
                      EnsembleRollout.run(regions=...))
                      FeatureSpec / FeatureScores / link_tracks: cyclone centres per member found on the GPU (a local
                      extremum with a depth test), their strike-probability map scored like any field, tracks linked on
                      the host (GenCast.ensemble_features, EnsembleRollout.run(features=...))
                      BandSpec: the members and the truth low-, band- or high-pass filtered per total wavenumber on
                      the GPU (analysis, a response per wavenumber, synthesis) in front of every scorer: scores scale by
                      scale (GenCast.ensemble_derived, EnsembleRollout.run(derived=...))
                      MapSpec / ScoreMaps / EventMaps: WHERE the forecast is good -- bias, RMSE, spread/skill, CRPS, outlier
                      frequency and Brier score per grid point, added up over dates on the GPU, one set of planes per lead
                      time (GenCast.ensemble_maps, EnsembleRollout.run(maps=...))
  NaNCleaner          gencast/nan_cleaning.py:27-156
  rollout             common/normalization.py:31-238 (InputsAndResiduals), training/train_helpers.py:485-622
                      (autoregressive_rollout); DeviceRollout keeps the context in HBM; EnsembleRollout keeps one
                      context per member there and scores the member states at every lead time (no reference
                      counterpart: GenCast.ensemble_rollout)
"""
from . import config, datasets, geometry, launch, losses, rollout, spectra, synthetic, verification, weights  # noqa: F401
from .config import (DenoiserArchitectureConfig, NoiseConfig, NoiseEncoderConfig,  # noqa: F401
                     SamplerConfig, SparseTransformerConfig, TASK, TaskConfig)
from .denoiser import Denoiser  # noqa: F401
from .ensemble import EnsembleSampler, member_seed, member_shard  # noqa: F401
from .gencast import GenCast, compute_loss, create_gencast_model, validation_loss  # noqa: F401
from .nan_cleaning import NaNCleaner  # noqa: F401
from .rollout import (DerivedRolloutResult, DeviceRollout, EnsembleRollout, EnsembleRolloutResult, FeatureRolloutResult,  # noqa: F401
                      InputsAndResiduals, WindowRolloutResult, autoregressive_rollout, state_channels)
from .sampler import Sampler, noise_schedule, stochastic_churn_rate_schedule  # noqa: F401
from .spectra import EnsembleSpectra, SphericalAnalysis  # noqa: F401
from .verification import (BandSpec, ClimatologyScores, DerivedSpec, EfiScores, EfiSpec, EnergyScores, EnergySpec, EnsembleScores, EventScores,  # noqa: F401
                           EventMaps, EventSpec, FeatureScores, FeatureSpec, FractionsScores, MapSpec, OrderScores, RegionScores,
                           RegionSpec, ScoreMaps, TailScores, VariogramScores, VariogramSpec, WindowSpec, efi_table, link_tracks)

__all__ = ["Denoiser", "Sampler", "GenCast", "EnsembleSampler", "create_gencast_model",
           "noise_schedule", "config", "datasets", "geometry", "synthetic", "weights", "rollout",
           "InputsAndResiduals", "autoregressive_rollout", "DeviceRollout", "NaNCleaner", "launch", "losses",
           "compute_loss", "validation_loss", "verification", "EnsembleScores", "spectra", "EnsembleSpectra",
           "SphericalAnalysis", "EnsembleRollout", "EnsembleRolloutResult", "state_channels", "EventScores", "EventSpec",
           "DerivedSpec", "DerivedRolloutResult", "OrderScores", "ClimatologyScores",
           "WindowSpec", "WindowRolloutResult", "EnergySpec", "EnergyScores", "VariogramSpec", "VariogramScores", "TailScores",
           "RegionSpec", "RegionScores", "FeatureSpec", "FeatureScores", "FeatureRolloutResult", "link_tracks",
           "FractionsScores", "BandSpec", "EfiSpec", "EfiScores", "efi_table",
           "MapSpec", "ScoreMaps", "EventMaps"]
