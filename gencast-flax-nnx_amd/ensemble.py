"""Ensemble-member sampling sharded one process per GPU.

Members are independent samples of the same (inputs, forcings) with different
noise (reference: per-member RNG + replicated inputs, common/rollout.py:123-139,
312-322; results pulled per device, :357-360).  Sharding: member m runs on rank
m % world_size; the only exchange is ONE broadcast of the packed conditioning
[G,B,C_in] from rank 0 -- `gc_comm_broadcast_cond`: RCCL over xGMI, issued by the
library itself on the handle's stream (no torch) once `NativeDenoiser.comm_init`
has run; there is no collective inside the denoiser or the sampler.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import numpy as np

from . import datasets, spectra as _spectra, verification
from .denoiser import Denoiser
from .sampler import Sampler


def member_shard(num_members: int, rank: int, world_size: int) -> List[int]:
  """Members handled by `rank` (round-robin so every rank gets ceil or floor)."""
  if not 0 <= rank < world_size:
    raise ValueError("rank out of range")
  return list(range(rank, num_members, world_size))


def member_seed(base_seed: int, member: int) -> int:
  """Noise stream of a member: independent of how members are sharded."""
  return int(np.random.SeedSequence([int(base_seed), int(member)]).generate_state(1)[0])


class EnsembleSampler:
  """Runs this rank's share of an ensemble.

  library_comm=True : the handle's own RCCL communicator (`native.comm_init` done by the caller)
      broadcasts the resident conditioning in place -- the production path.
  broadcast_host(array, src) -> array : broadcasts a host float32 array in place
      (e.g. gloo on CPU-only test boxes); used when no device broadcast is given.
  concurrent_members=K : this rank keeps K of its members in flight at once, each on its own library handle
      (own HIP stream, `Denoiser.member_lanes`); the conditioning reaches the extra handles by a
      device-to-device copy after the exchange.  Every member's result is bit-identical to K = 1.
  """

  def __init__(self, sampler: Sampler, rank: int = 0, world_size: int = 1,
               broadcast_host: Optional[Callable] = None, base_seed: int = 0,
               library_comm: bool = False, concurrent_members: int = 1):
    self._sampler = sampler
    self._denoiser: Denoiser = sampler._denoiser  # pylint: disable=protected-access
    self.rank, self.world_size = rank, world_size
    self._bh = broadcast_host
    self._library_comm = library_comm
    self.base_seed = base_seed
    if concurrent_members < 1:
      raise ValueError("concurrent_members must be >= 1")
    self.concurrent_members = int(concurrent_members)

  def member_noise(self, member: int, shape, template) -> np.ndarray:
    """Initial noise of one member: the SAME generator as `Sampler.__call__` (isotropic spherical
    white noise on an equiangular grid, dpm_solver_plus_plus_2s.py:71-78; `noise_kind` honoured),
    seeded by (base_seed, member) only."""
    gen = np.random.default_rng(member_seed(self.base_seed, member))
    draw = getattr(self._sampler, "draw_noise", None)
    if draw is None:                                       # bare stand-ins in tests
      return gen.standard_normal(shape, dtype=np.float32)
    return np.asarray(draw(gen, shape, template), np.float32)

  def _one_rank(self, what: str) -> None:
    """Refuses what needs all members at every point (the pair term of the CRPS, a sort, a count) on more than one rank."""
    if self.world_size > 1:
      raise ValueError(f"EnsembleSampler.{what} needs all members on one rank (world_size == 1): bring the other "
                       "ranks' members over and push them with NativeDenoiser.ens_push_host")

  def __call__(self, inputs, targets_template, forcings, num_members: int
               ) -> List[Tuple[int, datasets.Dataset]]:
    return self._run(inputs, targets_template, forcings, num_members, None)

  def scores(self, inputs, targets, forcings, num_members: int, *, fields: bool = False):
    """Runs the members as `__call__` does and scores them against `targets` on the device: every finished member
    goes into lane 0's member store by a device-to-device copy (`ens_push(slot, src=lane)`), none is downloaded,
    and one `ens_score` reduces them.  Returns `verification.EnsembleScores` in the units of `targets` (NaN targets
    are skipped point by point); with `fields=True` also the ensemble mean and variance as Datasets shaped like
    `targets` (xarray in, xarray out).  Node weights: `verification.node_weights(targets)`.
    One rank only: the pair term of the CRPS needs all members at every point."""
    self._one_rank("scores")
    return self._run(inputs, targets, forcings, num_members, bool(fields))

  def spectra(self, inputs, targets, forcings, num_members: int, *, lmax: Optional[int] = None):
    """Runs the members as `scores` does and analyses them on the device: `spectra.EnsembleSpectra` (power per total
    wavenumber of the truth, the members, the ensemble mean, the errors and the spread, per batch member and channel)
    in the units of `targets`.  No member is downloaded.  `lmax`: the band limit (default n_lon / 2).  `targets` must
    be finite: a column with a NaN has no transform and comes back NaN."""
    return self._spectral(inputs, targets, forcings, num_members, None, lmax)

  def scores_and_spectra(self, inputs, targets, forcings, num_members: int, *, fields: bool = False,
                         lmax: Optional[int] = None):
    """`scores(...)` and `spectra(...)` of the same members, sampled once: -> (scores, spectra), with `fields=True`
    (scores, mean, variance, spectra)."""
    return self._spectral(inputs, targets, forcings, num_members, bool(fields), lmax)

  def events(self, inputs, targets, forcings, num_members: int, spec):
    """Runs the members as `scores` does and counts, on the device, the events of `spec` (a `verification.EventSpec`:
    thresholds per variable in the units of `targets`, one direction per event) among the members and in the truth:
    `verification.EventScores` (Brier score and its decomposition, reliability curve, ROC, economic value, per event,
    batch member and channel).  No member is downloaded.  Node weights:
    `verification.quantize_node_weights(verification.node_weights(targets))`."""
    self._one_rank("events")
    return self._run(inputs, targets, forcings, num_members, None, events=spec)

  def derived(self, inputs, targets, forcings, num_members: int, spec, events=None):
    """Runs the members as `scores` does, sends them and `targets` through `spec` (a `verification.DerivedSpec`: wind speed
    from two components, fields pooled over a neighbourhood; or a `verification.BandSpec`: the fields low-, band- or high-pass
    filtered per total wavenumber) on the device and scores the derived fields there:
    `verification.EnsembleScores` over the derived channels (`spec.template(targets)` names them), with `events` (an
    `EventSpec` keyed by the derived names) -> (EnsembleScores, EventScores).  No member is downloaded.  The members are
    taken as they are sampled, scale 1 and location 0: under a normalisation wrapper (`InputsAndResiduals`, `NaNCleaner`
    around one) a single-step sample is a normalised RESIDUAL, and the norm of two residuals is no wind speed -- the wrappers
    therefore have no such method; `EnsembleRollout.run(derived=...)` derives from member STATES, which are fields."""
    self._one_rank("derived")
    return self._run(inputs, targets, forcings, num_members, None, derived=(spec, events))

  def features(self, inputs, targets, forcings, num_members: int, spec):
    """Runs the members as `scores` does and looks, on the device, for the features of `spec` (a `verification.FeatureSpec`:
    cyclone centres as local extrema with a depth test) in every member and in `targets`: `verification.FeatureScores` -- the
    centres per member and of the truth, the strike-probability map (the ensemble mean of the 0 / 1 strike fields), the
    `EnsembleScores` of the strike store and its `EventScores` at threshold 0.5.  Only the lists of centres and the
    probability map are downloaded, no member.  The members are taken as they are sampled, scale 1 and location 0, as in
    `derived`; `EnsembleRollout.run(features=...)` detects on member STATES, which are fields."""
    self._one_rank("features")
    return self._run(inputs, targets, forcings, num_members, None, features=spec)

  def order(self, inputs, targets, forcings, num_members: int, probs=(), *, quantile_fields: bool = False):
    """Runs the members as `scores` does and sorts them, point by point, on the device: `verification.OrderScores` in the
    units of `targets` -- the reliability / potential split of the ensemble CRPS (Hersbach 2000), the outlier frequencies
    and, for the probabilities `probs` (at most 8), the pinball loss and the coverage of the quantile fields.  With
    `quantile_fields=True` also those fields (the median, a p10 / p90 band) as Datasets shaped like `targets`; they need no
    truth and exist wherever all members are finite.  No member is downloaded."""
    self._one_rank("order")
    return self._run(inputs, targets, forcings, num_members, None, order=(tuple(probs), bool(quantile_fields)))

  def climatology(self, inputs, targets, forcings, num_members: int, climatology):
    """Runs the members as `scores` does and scores them, on the device, against `climatology`: K (2..64) Datasets shaped
    like `targets` -- past states for the same calendar date; a plain climatological mean is given twice.  Returns
    `verification.ClimatologyScores` in the units of `targets`: the anomaly correlation of the ensemble mean, the CRPS
    skill score against the climatological ensemble, the mean-square skill score.  The K fields are uploaded into the
    store of a second handle (`Denoiser.climatology_handle`); no member is downloaded.  NaNs in `targets` or in a sample
    are points the device does not count."""
    self._one_rank("climatology")
    climatology = list(climatology)
    if not 2 <= len(climatology) <= 64:
      raise ValueError(f"climatology must be 2..64 Datasets shaped like the targets, got {len(climatology)}")
    return self._run(inputs, targets, forcings, num_members, None, climatology=climatology)

  def efi(self, inputs, targets, forcings, num_members: int, climatology, spec=None, fields: bool = True):
    """Runs the members as `scores` does and ranks them, point by point on the device, in `climatology` (K Datasets as in
    `climatology`): the Extreme Forecast Index, verified against `targets` by `spec` (a `verification.EfiSpec`; None: its
    defaults) -> `verification.EfiScores`, with `fields` -> (EfiScores, EFI Dataset, observed-index Dataset), both shaped
    like `targets`.  `targets` None (a forecast without an analysis): -> the EFI Dataset alone, shaped like a sample.  The
    index has no unit.  No member is downloaded."""
    self._one_rank("efi")
    climatology = list(climatology)
    if not 2 <= len(climatology) <= 64:
      raise ValueError(f"climatology must be 2..64 Datasets shaped like the targets, got {len(climatology)}")
    spec = verification.EfiSpec() if spec is None else spec
    return self._run(inputs, climatology[0] if targets is None else targets, forcings, num_members, None,
                     efi=(climatology, spec, bool(fields), targets is not None))

  def multivariate(self, inputs, targets, forcings, num_members: int, energy=None, variogram=None):
    """Runs the members as `scores` does and forms, on the device, the two proper scores of a JOINT forecast: with `energy`
    (a `verification.EnergySpec`: groups of variables) the energy score of every group, with `variogram` (a
    `verification.VariogramSpec`: grid offsets and an order) the variogram score of every channel at every offset.
    -> (`verification.EnergyScores` or None, `verification.VariogramScores` or None), both in the units of `targets`.
    No member is downloaded."""
    self._one_rank("multivariate")
    if energy is None and variogram is None:
      raise ValueError("multivariate needs an EnergySpec, a VariogramSpec or both")
    return self._run(inputs, targets, forcings, num_members, None, multivariate=(energy, variogram))

  def tails(self, inputs, targets, forcings, num_members: int, spec):
    """Runs the members as `scores` does and forms, on the device, the threshold-weighted CRPS at the thresholds of `spec`
    (a `verification.EventSpec`: thresholds per variable in the units of `targets`; direction > 0: the upper tail, weight
    1{z >= threshold}, < 0: the lower tail): `verification.TailScores` -- the CRPS of members and truth clamped at the
    threshold, fair and of the empirical distribution, per threshold, batch member and channel.  The members of a point are
    sorted once for all thresholds.  No member is downloaded."""
    self._one_rank("tails")
    return self._run(inputs, targets, forcings, num_members, None, tails=spec)

  def maps(self, inputs, targets, forcings, num_members: int, spec, events=None):
    """Runs the members as `scores` does and forms, on the device, the score maps of this one date for the channels of `spec`
    (a `verification.MapSpec`): `verification.ScoreMaps` -- the per-point planes of bias, RMSE, spread, CRPS and the outlier
    counts, in the units of `targets`, additive over dates (`ScoreMaps.merge`).  With `MapSpec(events=True)` and `events` (an
    `EventSpec`) -> (ScoreMaps, `verification.EventMaps`).  Only the planes are downloaded, no member."""
    self._one_rank("maps")
    if not isinstance(spec, verification.MapSpec):
      raise TypeError("spec must be a verification.MapSpec")
    if spec.events and events is None:
      raise ValueError("maps: MapSpec(events=True) needs an EventSpec (events=...)")
    return self._run(inputs, targets, forcings, num_members, None, maps=(spec, events if spec.events else None))

  def regions(self, inputs, targets, forcings, num_members: int, spec):
    """Runs the members as `scores` does and forms, on the device, the sums of `scores` for every region of `spec` (a
    `verification.RegionSpec`) from one pass over the nodes of all regions: `verification.RegionScores`, whose `[name]` is the
    region's `EnsembleScores`.  No member is downloaded."""
    self._one_rank("regions")
    return self._run(inputs, targets, forcings, num_members, None, regions=spec)

  def _spectral(self, inputs, targets, forcings, num_members, score_fields, lmax):
    self._one_rank("spectra")
    return self._run(inputs, targets, forcings, num_members, score_fields, spectral=True, lmax=lmax)

  def _run(self, inputs, targets_template, forcings, num_members: int, score_fields: Optional[bool], spectral: bool = False,
           lmax: Optional[int] = None, **asked):
    """`score_fields` None: members come back as Datasets (`__call__`) or, with `spectral`, only their spectra are
    formed, or, with `events` (an EventSpec), only their event tables, or, with `order` (probabilities, want fields), only
    their order statistics, or, with `climatology` (K Datasets), only their skill against it, or, with `multivariate` (an
    EnergySpec or None, a VariogramSpec or None), only their energy and variogram scores, or, with `tails` (an EventSpec), only
    their threshold-weighted CRPS sums, or, with `regions` (a RegionSpec), only their sums per region, or, with `derived` (a
    DerivedSpec, an EventSpec or None), only the scores of the derived fields, or, with `features` (a FeatureSpec), only the
    centres and the scores of their strike fields, or, with `efi` (K Datasets, an EfiSpec, want fields, has a truth), only their
    extreme forecast index, or, with `maps` (a MapSpec, an EventSpec or None), only their score maps of this date; else they
    are scored (`scores`), with
    `spectral` both.  `asked`: at most one of these keywords (one that is None was not asked for)."""
    asked = {what: arg for what, arg in asked.items() if arg is not None}
    events, order, climatology, tails, regions = (asked.get(k) for k in ("events", "order", "climatology", "tails", "regions"))
    fspec = asked.get("features")
    eclim, espec, efields, etruth = asked.get("efi", (None, None, False, False))
    mspec, mev = asked.get("maps", (None, None))
    if mev is not None:                                    # the events a MapSpec(events=True) counts: those of the main store
      events = mev
    (dspec, dev), (energy, variogram) = asked.get("derived", (None, None)), asked.get("multivariate", (None, None))
    template = datasets.as_dataset(targets_template)
    # every rank packs its (possibly stale) local copy to size buffers; rank 0's data wins
    cond, grid_shape, slots = self._denoiser.init_for(inputs, template, forcings)
    native = self._denoiser.native
    native.set_noisy_slots(slots)
    if self.world_size > 1 and self._library_comm:
      if self.rank == 0:
        native.upload_cond(cond)
      native.comm_broadcast_cond(0)
    else:
      if self.world_size > 1 and self._bh is not None:
        cond = self._bh(np.ascontiguousarray(cond, dtype=np.float32), 0)
      native.upload_cond(cond)
    sigmas = np.asarray(self._sampler.noise_levels, dtype=np.float32)
    shape = (cond.shape[0], cond.shape[1], self._denoiser.dims.c_out)
    mine = member_shard(num_members, self.rank, self.world_size)
    lanes = [native]
    k = min(self.concurrent_members, len(mine))
    if k > 1:
      lanes += list(self._denoiser.member_lanes(k - 1))
      native.sync()                                        # the conditioning is complete on lane 0's stream
      ptr, _ = native.cond_device_ptr()
      for lane in lanes[1:]:
        lane.set_noisy_slots(slots)
        lane.upload_cond_dev(ptr)                          # device-to-device, on the lane's own stream
    scoring = score_fields is not None
    main = None                                            # lane 0's member store, where anything is scored at all
    if scoring or spectral or asked:
      weights = None if spectral and not scoring else verification.node_weights(template)
      wq = (None if events is None and dev is None and fspec is None and not (espec is not None and etruth and espec.n_events)
            else verification.quantize_node_weights(weights))
      # (scored once: the thresholds are set by that call, after the members are in; events and derived fields alone need no
      # node weights on the main store)
      main = verification.ScoredStore(native, num_members, weights if scoring or asked.keys() - {"events", "derived", "features"} else None,
                                      events=events, thresholds=None if events is None else events.packed(template), weight_q=wq,
                                      set_per_score=mspec is None, order=None if order is None else order[0],
                                      maps=mspec, map_channels=None if mspec is None else mspec.channels(template),
                                      climatology=None if climatology is None and eclim is None
                                      else self._denoiser.climatology_handle(self._denoiser.dims.c_out),
                                      efi=None if espec is None else espec if wq is not None else verification.EfiSpec((), (), espec.bins),
                                      energy=None if energy is None else energy.plan(template),
                                      variogram=None if variogram is None else variogram.plan(template),
                                      tails=tails, tail_thresholds=None if tails is None else tails.packed(template),
                                      regions=regions, region_bits=None if regions is None else regions.node_bits(template))
      main.setup()
    if spectral:
      _spectra.ensure_tables(native, template, lmax)
    out = []
    for g0 in range(0, len(mine), len(lanes)):
      group = mine[g0:g0 + len(lanes)]
      for lane, m in zip(lanes, group):                    # enqueue only: no host synchronisation in here
        lane.upload_noise(self.member_noise(m, shape, template))
        lane.sample_resident(sigmas, skip_dead_call=True, want_stats=False)
      for lane, m in zip(lanes, group):
        if main is not None:
          native.ens_push(m, src=lane)
        else:
          out.append((m, datasets.like_inputs(Denoiser.unpack_outputs(lane.download_sample(), grid_shape, template),
                                              targets_template, inputs, forcings)))
    if main is None:
      return out
    pack =lambda ds: np.transpose(datasets.dataset_to_stacked(datasets.as_dataset(ds), template.sizes), (1, 2, 0, 3)).reshape(shape)
    truth = pack(template)
    as_given = lambda fields: [datasets.like_inputs(Denoiser.unpack_outputs(f, grid_shape, template), targets_template, inputs,
                                                    forcings) for f in fields]

    def derived_scores():
      plan = dspec.plan(template)
      if isinstance(dspec, verification.BandSpec):           # a band view: a handle with the analysis tables of its band limit
        handle, how = self._denoiser.band_handle(len(plan["band"]), "single"), "band_plan"
        _spectra.ensure_tables(handle, template, plan["response"].shape[1])
      else:
        handle, how = self._denoiser.view_handle(len(plan["op"])), "plan"
      view = verification.ScoredStore(handle, num_members, weights, events=dev,
                                      thresholds=None if dev is None else dev.packed(dspec.template(template)), weight_q=wq,
                                      source=native, set_per_score=True, **{how: plan})
      view.setup()
      scores, event_scores = view.score(truth)
      return scores if dev is None else (scores, event_scores)

    def feature_scores():
      plan, ftemplate, fev = fspec.plan(template), fspec.template(template), fspec.event_spec()
      view = verification.ScoredStore(self._denoiser.feature_handle(len(plan["channel"]), "single"), num_members, weights,
                                      events=fev, thresholds=fev.packed(ftemplate), weight_q=wq, feature_plan=plan, source=native,
                                      set_per_score=True)
      view.setup()
      scores, event_scores = view.score(truth, want_fields=True)
      mean = view.handle.ens_download_fields()[0]
      members, of_truth = verification.split_centres(view.centres())
      probability = datasets.like_inputs(Denoiser.unpack_outputs(mean, grid_shape, ftemplate), targets_template, inputs, forcings)
      return verification.FeatureScores(scores, event_scores, members, of_truth, probability, ftemplate)

    def multivariate_scores():
      en = main.score_energy(truth)
      return en, main.score_variogram(truth if en is None else None)      # (the truth is on the device after the first)

    def efi_scores():
      main.load_climatology([pack(c) for c in eclim])
      if not etruth:                                       # a forecast without an analysis: the field alone
        return as_given([main.efi_field_without_truth()])[0]
      scores = main.score_efi(truth)
      return (scores,) + tuple(as_given(main.efi_fields())) if efields else scores

    def order_scores():
      scores = main.score_order(truth)
      return (scores, as_given(main.quantile_fields())) if order[1] else scores

    def map_scores():                                      # one date into slot 0 of accumulators made for this call
      if mev is not None:
        main.score_events(truth)                             # (leaves the codes and the truth on the device)
      main.accumulate_maps(0, None if mev is not None else truth)
      return main.download_maps(0)

    if asked:                                              # (what was asked for is scored alone)
      return {"derived": derived_scores, "maps": map_scores, "features": feature_scores, "events": lambda: main.score_events(truth),
              "climatology": lambda: main.score_climatology([pack(c) for c in climatology], truth),
              "tails": lambda: main.score_tails(truth), "regions": lambda: main.score_regions(truth),
              "multivariate": multivariate_scores, "order": order_scores, "efi": efi_scores}[next(iter(asked))]()
    if not scoring:
      return _spectra.EnsembleSpectra(native.ens_spectrum(truth), num_members)
    result = (main.score(truth, want_fields=score_fields)[0],)
    if score_fields:
      result += tuple(as_given(native.ens_download_fields()))
    if spectral:
      result += (_spectra.EnsembleSpectra(native.ens_spectrum(None), num_members),)   # the truth is on the device already
    return result if len(result) > 1 else result[0]
