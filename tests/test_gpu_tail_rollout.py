"""The threshold-weighted CRPS through the sampler and the ensemble rollout (EnsembleRollout.run(tails=),
GenCast.ensemble_tails) against the float64 definition (tests/tail_reference.py) on the members the
device itself kept.  Size: the tiny model of tests/test_gpu_order_rollout.py (9 x 16 grid, G = 144, batch 2, 82 channels),
horizon 2, M = 3, both `norm` settings.

The raw sums lie within (G + M (M - 1) / 2 + 8) 2^-53 sum|term| of the reference (tests/test_gpu_tail.py), counts and invalid
==; the physical sums are `scaled` from the raw ones, which is asserted as an equality.  The thresholds reach the members'
units by the map of the truth, restated here: (thr - l) / s in float64, rounded once; without a norm one plain cast."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import EnsembleSampler, rollout, verification
from gencast_flax_nnx_amd.verification import EventSpec
from tests import tail_reference as R
from tests import window_reference as WR
from tests.test_gpu_derived_rollout import _device_derive
from tests.test_gpu_ensemble_rollout import _Setup, B, C
from tests.test_gpu_tail import _check
from tests.test_gpu_verification import _small_model, _stack

pytestmark = pytest.mark.gpu

HORIZON, M = 2, 3
U10, V10 = "10m_u_component_of_wind", "10m_v_component_of_wind"
TAILS = EventSpec({"2m_temperature": np.array([0.5, -0.5, 0.0]), U10: np.array([1.0, -1.0, 0.25]),
                   "geopotential": np.array([0.5, -0.5, 0.0]).reshape(3, 1, 1, 1) * np.linspace(0.5, 1.5, 13).reshape(1, 13, 1, 1)},
                  (+1, -1, +1))
TAILS_WIND = EventSpec({"wind10": np.array([1.0, 2.0]), "2m_temperature": np.array([0.0, 0.5])}, (+1, -1))
TAILS_SUM = EventSpec({"2m_temperature": np.array([0.5]), "geopotential": np.array([-0.5])}, (+1,))


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  for lane in getattr(s.gc.denoiser, "_lanes", None) or []:
    lane.close()
  s.gc.denoiser.native.close()


@pytest.fixture(scope="module")
def runs(setup):
  """One run with the tails and one without, the same members: computed once and left unchanged."""
  out = {}
  for which in ("wrapper", "none"):
    er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
    kw = dict(init_noise=setup.noises[:M], keep_members=True, spectra=True)
    plain = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, **kw)
    with_tails = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, tails=TAILS, **kw)
    out[which] = (plain, with_tails)
  return out


def _members_units(thr, s, l, which):
  return ((thr.astype(np.float64) - l) / s).astype(np.float32) if which == "wrapper" else thr.astype(np.float32)


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_tails_per_lead_equal_the_reference_on_the_kept_members(setup, runs, which):
  _, res = runs[which]
  w = verification.node_weights(setup.template0)
  s, l = setup.stats_per_channel(which)
  thr = _members_units(TAILS.packed(setup.template0), s, l, which)
  given = ~np.isnan(thr[0, 0, 0])
  assert 0 < given.sum() < C                                      # some channels carry thresholds, the others are NaN
  assert len(res.tails) == len(res.tails_normalized) == HORIZON
  for k in range(HORIZON):
    members, truth = np.stack(res.members[k]), setup.truth(setup.targets, k, which)
    raw = res.tails_normalized[k]
    assert raw.n_members == M and raw.directions == (1, -1, 1) and raw.sums.shape == (3, B, C, 4)
    ref = R.reference(members, truth, w, thr, TAILS.directions)
    _check(f"{which} lead {k}", (raw.sums, raw.counts, raw.invalid), ref, setup.G, M)
    assert not raw.counts[:, :, ~given].any() and raw.counts[:, :, given].all()
    phys = res.tails[k]
    np.testing.assert_array_equal(phys.sums[..., 1], raw.sums[..., 1] * s)
    np.testing.assert_array_equal(phys.sums[..., 2], raw.sums[..., 2] * s)
    np.testing.assert_array_equal(phys.sums[..., 0], raw.sums[..., 0])
    np.testing.assert_array_equal(phys.sums[..., 3], raw.sums[..., 3])
    np.testing.assert_array_equal(phys.counts, raw.counts)
    np.testing.assert_array_equal(phys.base_rate[:, :, given], raw.base_rate[:, :, given])
  pv = res.tails[0].per_variable(setup.template0)
  assert pv["twcrps"]["geopotential"].shape == (3, B, 13)


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_a_run_without_tails_is_byte_identical_and_two_runs_merge(runs, which):
  plain, res = runs[which]
  assert plain.tails is None and plain.tails_normalized is None and "tails" not in vars(plain)
  for k in range(HORIZON):
    for a, b in ((plain.scores[k], res.scores[k]), (plain.scores_normalized[k], res.scores_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes() and a.rank_histogram.tobytes() == b.rank_histogram.tobytes()
    for a, b in ((plain.spectra[k], res.spectra[k]), (plain.spectra_normalized[k], res.spectra_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes()
    for m in range(M):                                            # the samples: bit-identical with and without `tails=`
      assert plain.members[k][m].tobytes() == res.members[k][m].tobytes()
  merged = res.merge(res)                                         # two start dates: the raw sums add
  np.testing.assert_array_equal(merged.tails[0].sums, 2.0 * res.tails[0].sums)
  np.testing.assert_array_equal(merged.tails_normalized[1].counts, 2 * res.tails_normalized[1].counts)
  np.testing.assert_array_equal(merged.tails[1].invalid, 2 * res.tails[1].invalid)
  ok = res.tails[0].sums[..., 0] > 0
  np.testing.assert_allclose(merged.tails[0].twcrps[ok], res.tails[0].twcrps[ok], rtol=1e-14)
  with pytest.raises(ValueError, match="tail scores"):
    res.merge(plain)


def test_a_derived_view_and_a_window_carry_their_own_specs(setup):
  """`tails={None: ..., "wind": ..., "sum2": ...}`: the view is scored at thresholds keyed by ITS variables, the window at
  thresholds keyed by its source's, each mapped with that store's statistics.  The derived truth has no download: it is
  formed by the same device call on two handles of the test's own, as in tests/test_gpu_derived_rollout.py."""
  which = "wrapper"
  dspec = verification.DerivedSpec([("norm2", "wind10", U10, V10), ("copy", "2m_temperature")])
  wspec = verification.WindowSpec("sum", 2)
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
  args = (setup.inp, setup.targets, setup.forcings, HORIZON, M)
  res = er.run(*args, init_noise=setup.noises[:M], keep_members=True, derived={"wind": dspec}, windows={"sum2": wspec},
               tails={None: TAILS, "wind": TAILS_WIND, "sum2": TAILS_SUM})
  w = verification.node_weights(setup.template0)
  s, l = setup.stats_per_channel(which)
  assert len(res.tails) == HORIZON and res.tails[0].directions == (1, -1, 1)
  # the view
  d = res.derived["wind"]
  assert len(d.tails) == len(d.tails_normalized) == HORIZON and d.tails[0].directions == (1, -1)
  dplan = dspec.plan(setup.template0, s, l)
  sd, ld = dspec.channel_stats(setup.template0, s, l)
  thr_d = _members_units(TAILS_WIND.packed(dspec.template(setup.template0)), sd, ld, which)
  for k in range(HORIZON):
    members = np.stack(d.members[k])                              # the device's own derived members
    truth_raw = setup.truth(setup.targets, k, which)
    truth_d = _device_derive(setup.gc.denoiser.graph, dplan, np.stack([truth_raw, truth_raw]))[0]
    raw = d.tails_normalized[k]
    assert raw.sums.shape == (2, B, 2, 4)
    _check(f"derived lead {k}", (raw.sums, raw.counts, raw.invalid), R.reference(members, truth_d, w, thr_d, (+1, -1)), setup.G, M)
    np.testing.assert_array_equal(d.tails[k].sums, raw.scaled(sd).sums)
  # the window: the sum over both leads of the main store
  win = res.windows["sum2"]
  assert win.leads == [1] and len(win.tails) == len(win.tails_normalized) == 1 and win.tails[0].directions == (1,)
  sw, lw = wspec.channel_stats(s, l)
  thr_w = _members_units(TAILS_SUM.packed(setup.template0), sw, lw, which)
  kind, coef = WR.coefficients("sum", 2)
  truth_w = WR.window(np.stack([setup.truth(setup.targets, k, which) for k in range(2)]), kind, coef)
  raw = win.tails_normalized[0]
  _check("window", (raw.sums, raw.counts, raw.invalid), R.reference(np.stack(win.members[0]), truth_w, w, thr_w, (+1,)),
         setup.G, M)
  np.testing.assert_array_equal(win.tails[0].sums, raw.scaled(sw).sums)
  # entries that were given no spec carry no series; an unknown key is refused
  only = er.run(*args, init_noise=setup.noises[:M], derived={"wind": dspec}, windows={"sum2": wspec}, tails={"wind": TAILS_WIND})
  assert only.tails is None and only.windows["sum2"].tails is None and len(only.derived["wind"].tails) == HORIZON
  for k in range(HORIZON):
    assert only.derived["wind"].tails_normalized[k].sums.tobytes() == d.tails_normalized[k].sums.tobytes()
  with pytest.raises(ValueError, match="nope"):
    er.run(*args, init_noise=setup.noises[:M], derived={"wind": dspec}, tails={"nope": TAILS})


def test_single_step_ensemble_tails_equals_the_reference_on_the_samplers_own_members():
  gc, inp, tgt, frc = _small_model()
  try:
    n = 4
    ens = EnsembleSampler(gc._sampler, base_seed=5)
    fields = [_stack(d) for _, d in sorted(ens(inp, tgt.map(np.zeros_like), frc, n), key=lambda t: t[0])]
    truth, w = _stack(tgt), verification.node_weights(tgt)
    # thresholds at the targets' own quantiles, so that both sides of every threshold are populated
    q = {name: np.quantile(np.asarray(tgt[name].data, np.float64), [0.75, 0.25]) for name in ("2m_temperature", "geopotential")}
    spec = EventSpec(q, (+1, -1))
    got = gc.ensemble_tails(inp, tgt, frc, num_members=n, spec=spec, rngs=5)
    ref = R.reference(np.stack(fields), truth, w, spec.packed(tgt), spec.directions)
    _check("ensemble_tails", (got.sums, got.counts, got.invalid), ref, truth.shape[0], n)
    assert got.n_members == n and got.directions == (1, -1)
    given = ref["counts"][0, 0] > 0
    assert 0 < given.sum() < given.size
    with pytest.raises(ValueError, match="ens_push_host"):
      EnsembleSampler(gc._sampler, rank=0, world_size=2).tails(inp, tgt, frc, n, spec)
  finally:
    gc.denoiser.native.close()
