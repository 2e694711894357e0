"""Multivariate scores through the sampler and the ensemble rollout (EnsembleRollout.run(energy=, variogram=),
GenCast.ensemble_multivariate) against the float64 definition (tests/multivar_reference.py) on the
members the device itself kept.  Size: the tiny model of tests/test_gpu_order_rollout.py (9 x 16 grid, G = 144, batch 2, 82
channels), horizon 2, M = 3.

Variogram: the raw sums within (G + M + 8) 2^-53 sum|term|, counts ==; the physical sums are `scaled` from the raw ones, which
is asserted as an equality.  Energy: a result holds err and pair, means of D = sqrt(D2 / S0).  D2 and S0 are each within
(n + 8) 2^-53 of their reference relative to themselves (every term is >= 0), the quotient and the root add two roundings and
halve the relative error, the mean of at most P values adds P more: |err - reference| <= (n + P + 12) 2^-53 reference, and
the same for pair (`_energy_bound`)."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import EnsembleSampler, rollout, verification
from gencast_flax_nnx_amd.verification import EnergySpec, VariogramSpec
from tests import multivar_reference as R
from tests.test_gpu_derived_rollout import _device_derive
from tests.test_gpu_ensemble_rollout import _Setup, B, C
from tests.test_gpu_multivar import _check_variogram
from tests.test_gpu_verification import _small_model, _stack

pytestmark = pytest.mark.gpu

HORIZON, M = 2, 3
N_LAT, N_LON = 9, 16
U10, V10 = "10m_u_component_of_wind", "10m_v_component_of_wind"
ENERGY = EnergySpec({"wind10": [U10, V10], "z": ["geopotential"], "t2m": ["2m_temperature"]},
                    weights={"geopotential": np.linspace(0.5, 2.0, 13), "2m_temperature": 2.0})
VARIOGRAM = VariogramSpec([(0, 1), (1, 0), (0, 4), (4, 0)], p=0.5)


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  for lane in getattr(s.gc.denoiser, "_lanes", None) or []:
    lane.close()
  s.gc.denoiser.native.close()


@pytest.fixture(scope="module")
def runs(setup):
  """One run with the multivariate scores and one without, the same members: computed once and left unchanged."""
  out = {}
  for which in ("wrapper", "none"):
    er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
    kw = dict(init_noise=setup.noises[:M], keep_members=True, spectra=True)
    plain = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, **kw)
    with_mv = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, energy=ENERGY, variogram=VARIOGRAM, **kw)
    out[which] = (plain, with_mv)
  return out


def _energy_bound(ref, value, M):
  P = M * (M + 1) // 2
  return (ref["n"][None, :] + P + 12.0) * 2.0 ** -53 * np.abs(value)


def _check_energy_scores(tag, got, ref, M):
  want = R.energy_scores(ref["d2"], ref["s0"], M)
  for name in ("err", "pair"):
    err = np.abs(getattr(got, name) - want[name])
    bound = _energy_bound(ref, want[name], M)
    print(f"{tag} {name}: worst |device - reference| / bound {float((err / bound).max()):.3f}")
    assert np.all(err <= bound), f"{tag}: {name}"
  assert got.n_members == M and got.invalid == ref["invalid"]


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_energy_and_variogram_per_lead_equal_the_reference_on_the_kept_members(setup, runs, which):
  _, res = runs[which]
  w = verification.node_weights(setup.template0)
  scale, _ = setup.stats_per_channel(which)
  plan = ENERGY.plan(setup.template0)
  assert len(res.energy) == len(res.variogram) == len(res.variogram_normalized) == HORIZON
  for k in range(HORIZON):
    members, truth = np.stack(res.members[k]), setup.truth(setup.targets, k, which)
    en = res.energy[k]
    assert en.names == ("wind10", "z", "t2m") and en.err.shape == (B, 3)
    _check_energy_scores(f"{which} lead {k}", en, R.energy(members, truth, w, plan["group"], plan["scale"]), M)
    raw = res.variogram_normalized[k]
    assert raw.n_members == M and raw.offsets == VARIOGRAM.offsets and raw.p == 0.5 and raw.sums.shape == (4, B, C, 4)
    _check_variogram(f"{which} lead {k}", (raw.sums, raw.counts), R.variogram(members, truth, w, N_LAT, N_LON, VARIOGRAM.offsets, 0.5),
                     setup.G, M)
    phys = res.variogram[k]
    ap = np.abs(scale) ** 0.5
    np.testing.assert_array_equal(phys.sums[1], raw.sums[1] * (ap * ap)[None, :, None])
    np.testing.assert_array_equal(phys.sums[2], raw.sums[2] * ap[None, :, None])
    np.testing.assert_array_equal(phys.sums[0], raw.sums[0])
    np.testing.assert_array_equal(phys.counts, raw.counts)
    np.testing.assert_allclose(phys.roughness_ratio, raw.roughness_ratio, rtol=1e-12)
  pv = res.variogram[0].per_variable(setup.template0)
  assert pv["variogram_score"]["geopotential"].shape == (B, 13, 4)


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_a_run_without_the_new_arguments_is_byte_identical(runs, which):
  plain, res = runs[which]
  assert plain.energy is None and plain.variogram is None and plain.variogram_normalized is None
  for k in range(HORIZON):
    for a, b in ((plain.scores[k], res.scores[k]), (plain.scores_normalized[k], res.scores_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes() and a.rank_histogram.tobytes() == b.rank_histogram.tobytes()
    for a, b in ((plain.spectra[k], res.spectra[k]), (plain.spectra_normalized[k], res.spectra_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes()
    for m in range(M):
      assert plain.members[k][m].tobytes() == res.members[k][m].tobytes()
  # two start dates: the variogram sums add, the energy scores keep the forecasts of both
  merged = res.merge(res)
  np.testing.assert_array_equal(merged.variogram[0].sums, 2.0 * res.variogram[0].sums)
  np.testing.assert_array_equal(merged.variogram_normalized[1].counts, 2 * res.variogram_normalized[1].counts)
  assert merged.energy[0].n_forecasts == 2 * B
  np.testing.assert_allclose(merged.energy[0].energy_score, res.energy[0].energy_score, rtol=1e-14)
  with pytest.raises(ValueError, match="energy"):
    res.merge(plain)


def test_derived_entries_and_windows_carry_their_own_scores(setup):
  """A derived view is scored over the groups that name ITS variables, a window over those of its source; the variogram
  reaches every store.  The derived truth has no download: it is formed by the same device call on two handles of the
  test's own, as in tests/test_gpu_derived_rollout.py."""
  which = "wrapper"
  dspec = verification.DerivedSpec([("norm2", "wind10", U10, V10), ("copy", "2m_temperature")])
  energy = EnergySpec({"uv": [U10, V10], "speed": ["wind10"], "both": ["2m_temperature"]})
  wspec = verification.WindowSpec("mean", 2)
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
  res = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, init_noise=setup.noises[:M], keep_members=True,
               derived={"wind": dspec}, windows={"mean2": wspec}, energy=energy, variogram=VARIOGRAM)
  w = verification.node_weights(setup.template0)
  s, l = setup.stats_per_channel(which)
  assert res.energy[0].names == ("uv", "both")              # the main store: the groups of target variables
  d = res.derived["wind"]
  assert len(d.energy) == len(d.variogram) == HORIZON and d.energy[0].names == ("speed", "both")
  dplan = dspec.plan(setup.template0, s, l)
  sd, _ = dspec.channel_stats(setup.template0, s, l)
  eplan = energy.restricted(dspec.template(setup.template0)).plan(dspec.template(setup.template0))
  for k in range(HORIZON):
    members = np.stack(d.members[k])                              # the device's own derived members
    truth_raw = setup.truth(setup.targets, k, which)
    truth_d = _device_derive(setup.gc.denoiser.graph, dplan, np.stack([truth_raw, truth_raw]))[0]
    _check_energy_scores(f"derived lead {k}", d.energy[k], R.energy(members, truth_d, w, eplan["group"], eplan["scale"]), M)
    raw = d.variogram_normalized[k]
    assert raw.sums.shape == (4, B, 2, 4)
    _check_variogram(f"derived lead {k}", (raw.sums, raw.counts),
                     R.variogram(members, truth_d, w, N_LAT, N_LON, VARIOGRAM.offsets, 0.5), setup.G, M)
    np.testing.assert_array_equal(d.variogram[k].sums, raw.scaled(sd).sums)
  # the scores of the view are its own: not those of the main store's wind components
  assert not np.allclose(d.energy[0].err[:, 0], res.energy[0].err[:, 0])
  win = res.windows["mean2"]
  assert win.leads == [1] and len(win.energy) == len(win.variogram) == 1 and win.energy[0].names == ("uv", "both")
  members = np.stack(win.members[0])
  mplan = energy.restricted(setup.template0).plan(setup.template0)
  ref = R.energy(members, np.zeros_like(members[0]), w, mplan["group"], mplan["scale"])
  pair = R.energy_scores(ref["d2"], ref["s0"], M)["pair"]
  np.testing.assert_allclose(win.energy[0].pair, pair, rtol=1e-10)             # (the pair term does not see the truth)
  assert win.variogram_normalized[0].sums.shape == (4, B, C, 4)
  with pytest.raises(ValueError, match="no scored store"):
    er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, init_noise=setup.noises[:M],
           energy=EnergySpec({"speed": ["wind10"]}))


def test_single_step_ensemble_multivariate_equals_the_reference_on_the_samplers_own_members():
  gc, inp, tgt, frc = _small_model()
  try:
    n = 4
    ens = EnsembleSampler(gc._sampler, base_seed=5)
    fields = [_stack(d) for _, d in sorted(ens(inp, tgt.map(np.zeros_like), frc, n), key=lambda t: t[0])]
    truth, w = _stack(tgt), verification.node_weights(tgt)
    plan = ENERGY.plan(tgt)
    en, vg = gc.ensemble_multivariate(inp, tgt, frc, num_members=n, energy=ENERGY, variogram=VARIOGRAM, rngs=5)
    _check_energy_scores("ensemble_multivariate", en, R.energy(np.stack(fields), truth, w, plan["group"], plan["scale"]), n)
    _check_variogram("ensemble_multivariate", (vg.sums, vg.counts),
                     R.variogram(np.stack(fields), truth, w, 13, 24, VARIOGRAM.offsets, 0.5), truth.shape[0], n)
    only_e, none_v = gc.ensemble_multivariate(inp, tgt, frc, num_members=n, energy=ENERGY, rngs=5)
    assert none_v is None and only_e.err.tobytes() == en.err.tobytes()
    none_e, only_v = gc.ensemble_multivariate(inp, tgt, frc, num_members=n, variogram=VARIOGRAM, rngs=5)
    assert none_e is None and only_v.sums.tobytes() == vg.sums.tobytes()
    with pytest.raises(ValueError, match="EnergySpec"):
      gc.ensemble_multivariate(inp, tgt, frc, num_members=n, rngs=5)
    with pytest.raises(ValueError, match="ens_push_host"):
      EnsembleSampler(gc._sampler, rank=0, world_size=2).multivariate(inp, tgt, frc, n, ENERGY)
  finally:
    gc.denoiser.native.close()
