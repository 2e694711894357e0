"""The fractions skill score through the ensemble rollout (EnsembleRollout.run(events=EventSpec(..., scales_km=...));
DESIGN.md section 8o): `res.events[k].fractions` recomputed by the definition (tests/fss_reference.py) from the members the
device itself kept.  Size: the tiny model of tests/test_gpu_ensemble_rollout.py (9 x 16 grid, G = 144, batch 2, 82 channels),
horizon 2, M = 3, both `norm` settings.

The event codes are integers and compared with == (through the tables); the four sums lie within G 2^-53 ref + spacing(ref) of
the math.fsum reference (tests/test_gpu_fss.py).  The thresholds reach the members' units by the map of the truth, restated
here: (thr - l) / s in float64, rounded once; without a norm one plain cast."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import rollout, verification
from gencast_flax_nnx_amd.verification import EventSpec, FractionsScores, quantize_node_weights
from tests import event_reference as ER
from tests import fss_reference as R
from tests.test_gpu_derived_rollout import _device_derive
from tests.test_gpu_ensemble_rollout import _Setup, B, C
from tests.test_gpu_fss import _check_sums

pytestmark = pytest.mark.gpu

HORIZON, M = 2, 3
N_LAT, N_LON = 9, 16
U10, V10 = "10m_u_component_of_wind", "10m_v_component_of_wind"
THRESHOLDS = {"2m_temperature": np.array([0.5, -0.5, 0.0]), U10: np.array([1.0, -1.0, 0.25]),
              "geopotential": np.array([0.5, -0.5, 0.0]).reshape(3, 1, 1, 1) * np.linspace(0.5, 1.5, 13).reshape(1, 13, 1, 1)}
SCALES = (0.0, 2500.0, 5000.0, 20000.0)                        # the point, two neighbourhoods, the whole sphere
EVENTS = EventSpec(THRESHOLDS, (+1, -1, +1), scales_km=SCALES)
EVENTS_POINT = EventSpec(THRESHOLDS, (+1, -1, +1))
EVENTS_WIND = EventSpec({"wind10": np.array([1.0, 2.0]), "2m_temperature": np.array([0.0, 0.5])}, (+1, -1), scales_km=(0.0, 5000.0))


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  for lane in getattr(s.gc.denoiser, "_lanes", None) or []:
    lane.close()
  s.gc.denoiser.native.close()


@pytest.fixture(scope="module")
def runs(setup):
  """One run with the scales and one without, the same members: computed once and left unchanged."""
  out = {}
  for which in ("wrapper", "none"):
    er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
    kw = dict(init_noise=setup.noises[:M], keep_members=True)
    plain = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, events=EVENTS_POINT, **kw)
    scaled = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, events=EVENTS, **kw)
    out[which] = (plain, scaled)
  return out


def _members_units(thr, s, l, which):
  return ((thr.astype(np.float64) - l) / s).astype(np.float32) if which == "wrapper" else thr.astype(np.float32)


def _reference(members, truth, thr, spec, template, wq):
  code = ER.tables(members, truth, thr, spec.directions, wq)["code"]
  r_lat, r_lon, row_wq = spec.windows(template)
  return R.separable(code, members.shape[0], N_LAT, N_LON, r_lat, r_lon, row_wq, wq), code


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_fractions_per_lead_equal_the_reference_on_the_kept_members(setup, runs, which):
  _, res = runs[which]
  wq, scale = quantize_node_weights(verification.node_weights(setup.template0))
  s, l = setup.stats_per_channel(which)
  thr = _members_units(EVENTS.packed(setup.template0), s, l, which)
  given = ~np.isnan(thr[0, 0, 0])
  assert 0 < given.sum() < C                                      # some channels carry thresholds, the others are NaN
  r_lat, r_lon, _ = EVENTS.windows(setup.template0)
  assert r_lat[0] == 0 and r_lat[-1] >= N_LAT - 1 and (r_lon[-1] == (N_LON - 1) // 2).all() and 0 < r_lat[1] < r_lat[2]
  assert len(res.events) == HORIZON
  for k in range(HORIZON):
    fr = res.events[k].fractions
    assert isinstance(fr, FractionsScores) and fr.sums.shape == (3, 4, B, C, 4)
    assert fr.scales_km == SCALES and fr.n_members == M and fr.directions == (1, -1, 1) and fr.scale == scale
    ref, code = _reference(np.stack(res.members[k]), setup.truth(setup.targets, k, which), thr, EVENTS, setup.template0, wq)
    _check_sums(f"{which} lead {k}", fr.sums, ref["sums"], setup.G)
    np.testing.assert_array_equal(fr.weight, res.events[k].weighted.sum(axis=(-1, -2)))
    assert not fr.sums[:, :, :, ~given].any() and (fr.sums[:, :, :, given, 1] > 0).any()
    assert np.isnan(fr.fss[:, :, :, ~given]).all()
    ok = fr.sums[..., 1] > 0
    assert ((fr.fss[ok] >= -1e-12) & (fr.fss[ok] <= 1.0)).all()
    # radius 0 is the point itself but in the two pole rows, whose nodes are one point and whose window is the whole row
    # (`DerivedSpec.window`): the fractions Brier score lies at or below the Brier score of the same table
    assert (r_lon[0, 1:-1] == 0).all() and (r_lon[0, [0, -1]] == (N_LON - 1) // 2).all()
    with np.errstate(invalid="ignore"):
      assert (fr.fbs[:, 0][:, :, given] <= res.events[k].brier[:, :, given] * (1.0 + 1e-12)).all()
  pv = res.events[0].fractions.per_variable(setup.template0)
  assert pv["fss"]["geopotential"].shape == (3, 4, B, 13)
  assert res.events[0].fractions.skilful_scale_km.shape == (3, B, C)


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_a_run_without_scales_is_byte_identical_and_two_runs_merge(runs, which):
  plain, res = runs[which]
  for k in range(HORIZON):
    assert plain.events[k].fractions is None
    for name in ("weighted", "counts", "invalid"):
      assert getattr(plain.events[k], name).tobytes() == getattr(res.events[k], name).tobytes()
    for a, b in ((plain.scores[k], res.scores[k]), (plain.scores_normalized[k], res.scores_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes() and a.rank_histogram.tobytes() == b.rank_histogram.tobytes()
    for m in range(M):                                            # the samples: bit-identical with and without the scales
      assert plain.members[k][m].tobytes() == res.members[k][m].tobytes()
  merged = res.merge(res)                                         # two start dates: the raw sums add
  for k in range(HORIZON):
    np.testing.assert_array_equal(merged.events[k].fractions.sums, 2.0 * res.events[k].fractions.sums)
    np.testing.assert_array_equal(merged.events[k].fractions.weight, 2 * res.events[k].fractions.weight)
    np.testing.assert_array_equal(merged.events[k].weighted, 2 * res.events[k].weighted)
    ok = res.events[k].fractions.sums[..., 1] > 0
    np.testing.assert_array_equal(merged.events[k].fractions.fss[ok], res.events[k].fractions.fss[ok])
  assert plain.merge(plain).events[0].fractions is None
  with pytest.raises(ValueError, match="only some of the event scores carry fractions"):
    res.merge(plain)


def test_a_derived_wind_speed_view_carries_its_own_fractions(setup):
  """`derived={"wind": (spec, events)}`: the view's events are keyed by ITS variables and mapped with its statistics; the
  windows are those of the same grid.  The derived truth has no download: it is formed by the same device call on two handles
  of the test's own, as in tests/test_gpu_derived_rollout.py."""
  which = "wrapper"
  dspec = verification.DerivedSpec([("norm2", "wind10", U10, V10), ("copy", "2m_temperature")])
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
  res = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, init_noise=setup.noises[:M], keep_members=True,
               derived={"wind": (dspec, EVENTS_WIND)})
  assert res.events is None
  wq, scale = quantize_node_weights(verification.node_weights(setup.template0))
  s, l = setup.stats_per_channel(which)
  d = res.derived["wind"]
  dplan = dspec.plan(setup.template0, s, l)
  dtemplate = dspec.template(setup.template0)
  sd, ld = dspec.channel_stats(setup.template0, s, l)
  thr_d = _members_units(EVENTS_WIND.packed(dtemplate), sd, ld, which)
  for k in range(HORIZON):
    fr = d.events[k].fractions
    assert isinstance(fr, FractionsScores) and fr.sums.shape == (2, 2, B, 2, 4) and fr.scales_km == (0.0, 5000.0)
    truth_raw = setup.truth(setup.targets, k, which)
    truth_d = _device_derive(setup.gc.denoiser.graph, dplan, np.stack([truth_raw, truth_raw]))[0]
    ref, _ = _reference(np.stack(d.members[k]), truth_d, thr_d, EVENTS_WIND, dtemplate, wq)
    _check_sums(f"derived lead {k}", fr.sums, ref["sums"], setup.G)
    np.testing.assert_array_equal(fr.weight, d.events[k].weighted.sum(axis=(-1, -2)))
    assert (fr.sums[..., 1] > 0).any()
