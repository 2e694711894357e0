"""The Extreme Forecast Index through the ensemble rollout and the sampler (EnsembleRollout.run(climatology=..., efi=...),
GenCast.ensemble_efi) against the float64 definition (tests/efi_reference.py) applied to the member
states the device itself kept and to the samples it was given: fields byte for byte, tables ==, sums within
(G + 8) 2^-53 sum|term|.  Size: the nano model (2.5 degree grid, G = 10 512, mesh 4, latent 256, 16 layers, 82 channels),
batch 1, two noise levels, two lead times, M = 3, K = 3; one run, shared by the tests and left unchanged."""
import dataclasses

import numpy as np
import pytest

from gencast_flax_nnx_amd import GenCast, config, datasets, rollout, synthetic, verification, weights
from gencast_flax_nnx_amd.denoiser import dims_from_arch
from gencast_flax_nnx_amd.verification import EfiScores, EfiSpec
from tests import derive_reference, efi_reference as R
from tests.test_gpu_efi import _same_bytes

pytestmark = pytest.mark.gpu

HORIZON, M, K, B, C = 2, 3, 3, 1, 82
SPEC = EfiSpec(quantiles=(0.9, 0.1), directions=(+1, -1), bins=20)
WIND = verification.DerivedSpec([("norm2", "wind10", "10m_u_component_of_wind", "10m_v_component_of_wind")])


def _stretch(ds, nt, rng):
  out = {}
  for k, v in ds.items():
    shape = list(v.data.shape)
    shape[v.dims.index("time")] = nt
    out[k] = datasets.Variable(v.dims, rng.standard_normal(shape).astype(np.float32))
  return datasets.Dataset(out, ds.coords)


def _like(ds, rng, hole=None):
  """A Dataset shaped like `ds` with other values (a climatological sample); `hole`: one NaN in the first variable."""
  out = {}
  for i, (k, v) in enumerate(ds.items()):
    a = (np.asarray(v.data, np.float32) + rng.standard_normal(np.shape(v.data)).astype(np.float32))
    if hole is not None and i == 0:
      a.reshape(-1)[hole] = np.nan
    out[k] = datasets.Variable(v.dims, a)
  return datasets.Dataset(out, ds.coords)


class _Run:
  def __init__(self):
    lat, lon = synthetic.grid_2p5deg()
    arch = dataclasses.replace(config.nano_architecture(mesh_size=4, d_model=256, num_layers=16, num_heads=4), node_output_size=C)
    self.inp, tgt1, frc1 = synthetic.make_example(lat, lon, batch=B, seed=0)
    rng = np.random.default_rng(5)
    self.targets, self.forcings = _stretch(tgt1, HORIZON, rng), _stretch(frc1, HORIZON, rng)
    sc = config.SamplerConfig(num_noise_levels=2, stochastic_churn_rate=0.0)
    params = weights.random_params(dims_from_arch(arch, 262, C), seed=3)
    self.gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=3)
    self.G = len(lat) * len(lon)
    self.shape = (self.G, B, C)
    self.template0 = rollout.isel_time(self.targets, slice(0, 1)).map(np.zeros_like)
    self.climatology = [[_like(rollout.isel_time(self.targets, slice(k, k + 1)), rng, hole=5 if (k, j) == (1, 2) else None)
                         for j in range(K)] for k in range(HORIZON)]
    self.er = rollout.EnsembleRollout(self.gc, None)
    self.res = self.er.run(self.inp, self.targets, self.forcings, HORIZON, M, keep_members=True, derived={"wind": WIND},
                           climatology=self.climatology, efi=SPEC, keep_efi=True)

  def packed(self, ds):
    """[G, B, C] float32 in the members' units: without a normalisation wrapper, one plain cast."""
    return rollout._members_units(ds, self.shape, 1.0, 0.0, False)


@pytest.fixture(scope="module")
def run():
  r = _Run()
  yield r
  r.gc.denoiser.close()


def _check(tag, sc, fields, ref, G, ranks):
  assert isinstance(sc, EfiScores) and (sc.n_members, sc.n_climatology, sc.ranks, sc.directions) == (M, K, ranks, (1, -1))
  _same_bytes(fields[0], ref["efi"], f"{tag}: EFI field")
  _same_bytes(fields[1], ref["observed"], f"{tag}: observed index")
  np.testing.assert_array_equal(sc.weighted, ref["weighted"], err_msg=f"{tag}: weighted")
  np.testing.assert_array_equal(sc.counts, ref["counts"], err_msg=f"{tag}: counts")
  assert sc.invalid == ref["invalid"], f"{tag}: invalid"
  tol, err = R.tolerance(ref, G), np.abs(sc.sums - ref["sums"])
  print(f"{tag}: worst |device - reference| / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
  assert np.all(err <= tol), f"{tag}: a sum outside (G + 8) 2^-53 sum|term|"


def test_efi_per_lead_equals_the_reference_on_the_kept_member_states(run):
  res = run.res
  w = verification.node_weights(run.template0)
  wq, scale = verification.quantize_node_weights(w)
  ranks = SPEC.ranks_for(K)
  assert len(res.efi) == len(res.efi_fields) == HORIZON and "efi_normalized" not in vars(res)
  for k in range(HORIZON):
    members = np.stack(res.members[k])
    clim = np.stack([run.packed(c) for c in run.climatology[k]])
    truth = run.packed(rollout.isel_time(run.targets, slice(k, k + 1)))
    ref = R.reference(members, clim, truth, w, ranks, SPEC.directions, SPEC.bins, wq)
    _check(f"lead {k}", res.efi[k], res.efi_fields[k], ref, run.G, ranks)
    assert res.efi[k].scale == scale and (ref["invalid"] > 0) == (k == 1)    # the hole in a sample of lead 1
    assert res.climatology[k].invalid == res.efi[k].invalid                 # the rule of section 8i: the same points


def test_the_derived_wind_speed_view_equals_the_reference_too(run):
  d = run.res.derived["wind"]
  w = verification.node_weights(run.template0)
  wq, _ = verification.quantize_node_weights(w)
  ranks = SPEC.ranks_for(K)
  plan = WIND.plan(run.template0, np.ones(C), np.zeros(C))
  assert len(d.efi) == len(d.efi_fields) == HORIZON
  cview = run.gc.denoiser.climatology_handle(1, view=True)
  for k in range(HORIZON):
    members = np.stack(d.members[k])
    # the derived samples and the derived truth: the view's plan applied to the samples and to the truth of the lead
    clim = derive_reference.apply(np.stack([run.packed(c) for c in run.climatology[k]]), plan)
    truth = derive_reference.apply(run.packed(rollout.isel_time(run.targets, slice(k, k + 1))), plan)
    if k == HORIZON - 1:                                   # what the device kept in the climatology view: the same bytes
      for j in range(K):
        _same_bytes(cview.ens_download_member(j), clim[j], f"derived sample {j}")
    ref = R.reference(members, clim, truth, w, ranks, SPEC.directions, SPEC.bins, wq)
    _check(f"wind lead {k}", d.efi[k], d.efi_fields[k], ref, run.G, ranks)
    assert d.efi[k].sums.shape == (B, 1, 6)


def test_merge_adds_and_a_run_without_the_index_is_what_it_was(run):
  res = run.res
  merged = res.merge(res)                                  # two start dates
  for k in range(HORIZON):
    np.testing.assert_array_equal(merged.efi[k].sums, 2.0 * res.efi[k].sums)
    np.testing.assert_array_equal(merged.efi[k].weighted, 2 * res.efi[k].weighted)
    np.testing.assert_array_equal(merged.derived["wind"].efi[k].counts, 2 * res.derived["wind"].efi[k].counts)
    np.testing.assert_allclose(merged.efi[k].roc_area, res.efi[k].roc_area, rtol=1e-12)
  assert merged.efi_fields is None
  with pytest.raises(ValueError, match="efi: the extreme forecast index ranks the members in the samples of `climatology`"):
    run.er.run(run.inp, run.targets, run.forcings, HORIZON, M, efi=SPEC)


def test_single_step_ensemble_efi_with_and_without_targets(run):
  """`GenCast.ensemble_efi` on the same model: the scored call and the truth-free call give the same EFI bytes."""
  tgt = rollout.isel_time(run.targets, slice(0, 1))
  clim = run.climatology[0]
  frc = rollout.isel_time(run.forcings, slice(0, 1))
  sc, efi, obs = run.gc.ensemble_efi(run.inp, tgt, frc, num_members=M, climatology=clim, spec=SPEC, rngs=5)
  assert isinstance(sc, EfiScores) and sc.ranks == SPEC.ranks_for(K) and sc.invalid == 0
  alone = run.gc.ensemble_efi(run.inp, None, frc, num_members=M, climatology=clim, rngs=5)
  a, b = run.packed(datasets.as_dataset(efi)), run.packed(datasets.as_dataset(alone))
  _same_bytes(a, b, "EFI with and without targets")
  assert np.all(np.abs(a) <= 1.0) and np.all(np.abs(run.packed(datasets.as_dataset(obs))) <= 1.0)
  only = run.gc.ensemble_efi(run.inp, tgt, frc, num_members=M, climatology=clim, spec=SPEC, fields=False, rngs=5)
  assert only.sums.tobytes() == sc.sums.tobytes() and only.weighted.tobytes() == sc.weighted.tobytes()


def test_the_normalisation_wrapper_passes_the_index_through():
  """Under `InputsAndResiduals` the samples take the map of the targets, which is increasing per point: the index of the
  wrapped call is the index of the inner call on the mapped arguments, with no rescaling, with and without targets."""
  from tests.test_gpu_verification import _small_model
  from tests.test_rollout import _stats
  gc, inp, tgt, frc = _small_model()
  try:
    wrapper = rollout.InputsAndResiduals(gc, *_stats(config.TASK))
    rng = np.random.default_rng(23)
    clim = [_like(tgt, rng) for _ in range(K)]
    sc, efi, obs = wrapper.ensemble_efi(inp, tgt, frc, num_members=M, climatology=clim, spec=SPEC, rngs=5)
    raw, ni, nt, nf = wrapper._normalized_loss_args(inp, tgt, frc)
    nclim = [datasets.Dataset({k: wrapper._subtract_input_and_normalize_target(raw, k, v) for k, v in datasets.as_dataset(c).items()},
                              datasets.as_dataset(c).coords) for c in clim]
    inner, efi_in, _ = gc.ensemble_efi(ni, nt, nf, num_members=M, climatology=nclim, spec=SPEC, rngs=5)
    assert sc.sums.tobytes() == inner.sums.tobytes() and sc.weighted.tobytes() == inner.weighted.tobytes()
    stack = lambda ds: datasets.dataset_to_stacked(datasets.as_dataset(ds), datasets.as_dataset(tgt).sizes)
    alone = wrapper.ensemble_efi(inp, None, frc, num_members=M, climatology=clim, rngs=5)
    assert stack(efi).tobytes() == stack(efi_in).tobytes() == stack(alone).tobytes()
    assert np.all(np.abs(stack(efi)) <= 1.0) and np.all(np.abs(stack(obs)) <= 1.0) and sc.invalid == 0
  finally:
    gc.denoiser.close()
