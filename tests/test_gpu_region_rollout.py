"""Regional scores through the sampler and the ensemble rollout (EnsembleRollout.run(regions=), GenCast.ensemble_regions;
DESIGN.md section 8m) against the float64 yardstick (tests/region_reference.py) on the members the device itself kept.
Size: the tiny model of tests/test_gpu_tail_rollout.py (9 x 16 grid, G = 144, batch 2, 82 channels), horizon 2, M = 3, both
`norm` settings.

The raw sums lie within (G + M^2 + 8) 2^-53 A_k of the reference (tests/test_gpu_region.py), histograms and invalid ==; the
physical sums are `scaled` from the raw ones, which is asserted as an equality."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import rollout, verification
from gencast_flax_nnx_amd.verification import RegionScores, RegionSpec
from tests import region_reference as R
from tests import window_reference as WR
from tests.test_gpu_derived_rollout import _device_derive
from tests.test_gpu_ensemble_rollout import _Setup, B, C
from tests.test_gpu_region import _check

pytestmark = pytest.mark.gpu

HORIZON, M = 2, 3
U10, V10 = "10m_u_component_of_wind", "10m_v_component_of_wind"
# lat -90, -67.5, .., 90; lon 0, 22.5, .., 337.5: two bands and a box that wraps through 0 degrees and overlaps both
BOUNDS = {"south": dict(lat=(-90, -22.5)), "tropics": dict(lat=(-22.5, 22.5)), "box": dict(lat=(-45, 45), lon=(-45, 45))}


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  for lane in getattr(s.gc.denoiser, "_lanes", None) or []:
    lane.close()
  s.gc.denoiser.native.close()


@pytest.fixture(scope="module")
def spec(setup):
  s = RegionSpec.from_bounds(setup.template0, BOUNDS)
  bits = s.node_bits(setup.template0)
  assert (bits == 0).any() and (bits == 7).any() and (bits == 1).any()            # nodes in none, in all three, in one
  return s


@pytest.fixture(scope="module")
def runs(setup, spec):
  """One run with the regions and one without, the same members: computed once and left unchanged."""
  out = {}
  for which in ("wrapper", "none"):
    er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
    kw = dict(init_noise=setup.noises[:M], keep_members=True, spectra=True)
    plain = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, **kw)
    with_regions = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, regions=spec, **kw)
    out[which] = (plain, with_regions)
  return out


def _raw(r):
  return r.sums, r.rank_histogram, r.invalid


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_regions_per_lead_equal_the_reference_on_the_kept_members(setup, spec, runs, which):
  _, res = runs[which]
  w = verification.node_weights(setup.template0)
  s, _ = setup.stats_per_channel(which)
  bits = spec.node_bits(setup.template0)
  assert len(res.regions) == len(res.regions_normalized) == HORIZON
  for k in range(HORIZON):
    members, truth = np.stack(res.members[k]), setup.truth(setup.targets, k, which)
    raw = res.regions_normalized[k]
    assert isinstance(raw, RegionScores) and raw.names == ("south", "tropics", "box") and raw.n_members == M
    assert raw.sums.shape == (3, B, C, 6)
    _check(f"{which} lead {k}", _raw(raw), R.reference(members, truth, w, bits, 3), setup.G, M, dyadic=False)
    phys = res.regions[k]
    for name in raw.names:                                        # physical = `scaled` of the raw, exactly
      assert phys[name].sums.tobytes() == raw[name].scaled(s).sums.tobytes()
      assert phys[name].rank_histogram.tobytes() == raw[name].scaled(s).rank_histogram.tobytes()
    np.testing.assert_array_equal(phys.invalid, raw.invalid)
    assert np.isfinite(phys["tropics"].crps).all() and (phys["tropics"].valid_points == 3 * 16).all()
  pv = res.regions[0].per_variable(setup.template0)
  assert pv["box"]["crps"]["geopotential"].shape == (B, 13)


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_a_run_without_regions_is_byte_identical_and_two_runs_merge(runs, which):
  plain, res = runs[which]
  assert plain.regions is None and plain.regions_normalized is None and "regions" not in vars(plain)
  for k in range(HORIZON):
    for a, b in ((plain.scores[k], res.scores[k]), (plain.scores_normalized[k], res.scores_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes() and a.rank_histogram.tobytes() == b.rank_histogram.tobytes()
    for a, b in ((plain.spectra[k], res.spectra[k]), (plain.spectra_normalized[k], res.spectra_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes()
    for m in range(M):                                            # the samples: bit-identical with and without `regions=`
      assert plain.members[k][m].tobytes() == res.members[k][m].tobytes()
  merged = res.merge(res)                                         # two start dates: the raw sums add
  np.testing.assert_array_equal(merged.regions_normalized[0].sums, 2.0 * res.regions_normalized[0].sums)
  np.testing.assert_array_equal(merged.regions[1].rank_histogram, 2 * res.regions[1].rank_histogram)
  np.testing.assert_array_equal(merged.regions[1].invalid, 2 * res.regions[1].invalid)
  np.testing.assert_allclose(merged.regions[0]["box"].crps, res.regions[0]["box"].crps, rtol=1e-14)
  with pytest.raises(ValueError, match="region scores"):
    res.merge(plain)


def test_a_derived_view_and_a_window_given_regions_by_name_carry_them(setup, spec):
  """`regions={None: ..., "wind": ..., "sum2": ...}`: every store lives on the same grid nodes, so the same kind of spec
  serves all of them.  The derived truth has no download: it is formed by the same device call on two handles of the test's
  own, as in tests/test_gpu_derived_rollout.py."""
  which = "wrapper"
  dspec = verification.DerivedSpec([("norm2", "wind10", U10, V10), ("copy", "2m_temperature")])
  wspec = verification.WindowSpec("sum", 2)
  box = RegionSpec.from_bounds(setup.template0, {"box": BOUNDS["box"], "north": dict(lat=(22.5, 90))})
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
  args = (setup.inp, setup.targets, setup.forcings, HORIZON, M)
  res = er.run(*args, init_noise=setup.noises[:M], keep_members=True, derived={"wind": dspec}, windows={"sum2": wspec},
               regions={None: spec, "wind": box, "sum2": box})
  w = verification.node_weights(setup.template0)
  s, l = setup.stats_per_channel(which)
  bits = box.node_bits(setup.template0)
  assert len(res.regions) == HORIZON and res.regions[0].names == ("south", "tropics", "box")
  # the view
  d = res.derived["wind"]
  assert len(d.regions) == len(d.regions_normalized) == HORIZON and d.regions[0].names == ("box", "north")
  dplan = dspec.plan(setup.template0, s, l)
  sd, _ = dspec.channel_stats(setup.template0, s, l)
  for k in range(HORIZON):
    members = np.stack(d.members[k])                              # the device's own derived members
    truth_raw = setup.truth(setup.targets, k, which)
    truth_d = _device_derive(setup.gc.denoiser.graph, dplan, np.stack([truth_raw, truth_raw]))[0]
    raw = d.regions_normalized[k]
    assert raw.sums.shape == (2, B, 2, 6)
    _check(f"derived lead {k}", _raw(raw), R.reference(members, truth_d, w, bits, 2), setup.G, M, dyadic=False)
    np.testing.assert_array_equal(d.regions[k].sums, raw.scaled(sd).sums)
  # the window: the sum over both leads of the main store
  win = res.windows["sum2"]
  assert win.leads == [1] and len(win.regions) == len(win.regions_normalized) == 1
  sw, _ = wspec.channel_stats(s, l)
  kind, coef = WR.coefficients("sum", 2)
  truth_w = WR.window(np.stack([setup.truth(setup.targets, k, which) for k in range(2)]), kind, coef)
  raw = win.regions_normalized[0]
  _check("window", _raw(raw), R.reference(np.stack(win.members[0]), truth_w, w, bits, 2), setup.G, M, dyadic=False)
  np.testing.assert_array_equal(win.regions[0].sums, raw.scaled(sw).sums)
  # entries that were given no spec carry no series; an unknown key is refused
  only = er.run(*args, init_noise=setup.noises[:M], derived={"wind": dspec}, windows={"sum2": wspec}, regions={"wind": box})
  assert only.regions is None and only.windows["sum2"].regions is None and len(only.derived["wind"].regions) == HORIZON
  for k in range(HORIZON):
    assert only.derived["wind"].regions_normalized[k].sums.tobytes() == d.regions_normalized[k].sums.tobytes()
  with pytest.raises(ValueError, match="nope"):
    er.run(*args, init_noise=setup.noises[:M], derived={"wind": dspec}, regions={"nope": spec})


def test_single_step_ensemble_regions_is_lead_time_0_of_the_rollout_for_the_same_noise(setup, spec):
  """Without a normalisation wrapper and with host noise, member m of both paths starts from the first field of the
  generator seeded by (base seed, m) and is conditioned on the same inputs: the same samples, hence the same bytes."""
  base = 5
  res = rollout.EnsembleRollout(setup.gc, None, base_seed=base).run(setup.inp, setup.targets, setup.forcings, 1, M,
                                                                     regions=spec)
  tgt0, frc0 = rollout.isel_time(setup.targets, slice(0, 1)), rollout.isel_time(setup.forcings, slice(0, 1))
  got = setup.gc.ensemble_regions(setup.inp, tgt0, frc0, num_members=M, spec=spec, rngs=base)
  assert isinstance(got, RegionScores) and got.names == spec.names and got.n_members == M
  lead0 = res.regions_normalized[0]
  np.testing.assert_array_equal(got.rank_histogram, lead0.rank_histogram)
  np.testing.assert_array_equal(got.invalid, lead0.invalid)
  np.testing.assert_array_equal(got.sums, lead0.sums)
  assert got.sums[..., 0].all() and np.isfinite(got["box"].crps).all()
  whole = setup.gc.ensemble_scores(setup.inp, tgt0, frc0, num_members=M, rngs=base)
  assert (got["tropics"].valid_weight < whole.valid_weight).all()
