"""Time windows through the stack: `EnsembleRollout.run(windows=...)` on the small model of tests/test_gpu_events.py (9 x 16
grid, batch 2) with horizon 5, M = 3 and `keep_members=True`, both `norm` settings.  "acc": the sum over two lead times of
the main store, tumbling (windows end at leads 1 and 3); "gust": the maximum over three lead times of a derived view (wind
speed and 2 m temperature, max-pooled), sliding (leads 2, 3, 4), with events.

The kept window members are held to tests/window_reference.py applied to the kept per-lead members, bit for bit.  The scores
and the event tables of a window are then compared with verification_reference / event_reference applied to THOSE kept
window members and the windowed truth (sums within `sum_tolerance`, the bound of DESIGN.md section 8c; tables ==).  The truth
of the main store is the targets' frame in the members' units; the derived truth has no download, so the test forms it by the
same device call on two handles of its own, as tests/test_gpu_derived_rollout.py does."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import DerivedSpec, EventSpec, WindowSpec, datasets, rollout, verification
from gencast_flax_nnx_amd.verification import quantize_node_weights
from tests import event_reference as ER
from tests import verification_reference as VR
from tests import window_reference as R
from tests.test_gpu_derived_rollout import WIND, WIND_R_LON, _device_derive
from tests.test_gpu_events import SB, SC, _Setup
from tests.test_gpu_verification import _check_sums

pytestmark = pytest.mark.gpu

HORIZON, M = 5, 3


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  rng = np.random.default_rng(15)

  def stretch(ds, nt):                                        # HORIZON random frames on the axes of the two-frame ones
    out = {}
    for k, v in ds.items():
      shape = list(v.data.shape)
      shape[v.dims.index("time")] = nt
      out[k] = datasets.Variable(v.dims, rng.standard_normal(shape).astype(np.float32))
    return datasets.Dataset(out, ds.coords)

  s.targets, s.forcings = stretch(s.tgt1, HORIZON), stretch(s.frc1, HORIZON)
  yield s
  s.gc.denoiser.close()


def _specs():
  wind = DerivedSpec(WIND, pool="max", r_lat=1, r_lon=WIND_R_LON)
  events = EventSpec({"10m_wind_speed": np.array([1.5, 2.5, 1.0]),
                      "wind_speed": np.array([1.5, 2.5, 1.0]).reshape(3, 1, 1, 1) * np.linspace(0.8, 1.2, 13).reshape(1, 13, 1, 1),
                      "2m_temperature": np.array([0.5, 1.0, 0.0])}, [1, 1, -1])
  return wind, events, WindowSpec("sum", 2), WindowSpec("max", 3, stride=1, source="wind")


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_rollout_windows_equal_the_definitions_on_the_kept_members(setup, which):
  wind, events, acc, gust = _specs()
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which), base_seed=3, concurrent_members=2)
  args = (setup.inp, setup.targets, setup.forcings, HORIZON, M)
  res = er.run(*args, keep_members=True, events=setup.spec, derived={"wind": wind}, windows={"acc": acc, "gust": (gust, events)})
  plain = er.run(*args, keep_members=True, events=setup.spec, derived={"wind": wind})
  assert plain.windows is None and sorted(res.windows) == ["acc", "gust"]
  s, l = setup.stats_per_channel(which)
  w = verification.node_weights(setup.template0)
  wq, wq_scale = quantize_node_weights(w)
  graph = setup.gc.denoiser.graph
  plan = wind.plan(setup.template0, s, l)
  truth = [setup.truth(k, which) for k in range(HORIZON)]
  truth_d = [_device_derive(graph, plan, np.stack([t, t]))[0] for t in truth]

  # ---- "acc": the sum over two leads of the main store
  part = res.windows["acc"]
  assert part.leads == [1, 3] and part.steps == 2 and len(part.scores) == len(part.members) == 2
  assert part.events is None and part.order is None
  sa, la = acc.channel_stats(s, l)
  np.testing.assert_array_equal(sa, s)
  np.testing.assert_array_equal(la, 2.0 * l)
  kind, coef = R.coefficients("sum", 2)
  for i, k in enumerate(part.leads):
    got = np.stack(part.members[i])
    assert got.shape == (M, setup.G, SB, SC) and got.dtype == np.float32
    want = R.window(np.stack([np.stack(res.members[k - 1]), np.stack(res.members[k])]), kind, coef)
    assert R.same_bits(got, want), f"{which} acc window {i}"
    truth_w = R.window(np.stack(truth[k - 1:k + 1]), kind, coef)
    ref = VR.reference(got, truth_w, w)
    sn = part.scores_normalized[i]
    _check_sums(f"{which} acc window {i}", sn.sums, sn.rank_histogram, ref, setup.G, M)
    np.testing.assert_array_equal(part.scores[i].sums, sn.scaled(sa).sums)
  assert part.scores[0].per_variable(part.template)["crps"]["temperature"].shape == (SB, 13)

  # ---- "gust": the maximum over three leads of the derived view, with events
  part = res.windows["gust"]
  assert part.leads == [2, 3, 4] and part.steps == 3 and len(part.scores) == len(part.members) == len(part.events) == 3
  sd, ld = gust.channel_stats(*wind.channel_stats(setup.template0, s, l))
  thr = events.packed(wind.template(setup.template0))
  if which == "wrapper":
    thr = ((thr.astype(np.float64) - ld) / sd).astype(np.float32)
  for i, k in enumerate(part.leads):
    got = np.stack(part.members[i])
    assert got.shape == (M, setup.G, SB, 15)
    want = R.window(np.stack([np.stack(res.derived["wind"].members[j]) for j in range(k - 2, k + 1)]), R.MAX)
    assert R.same_bits(got, want), f"{which} gust window {i}"
    truth_w = R.window(np.stack(truth_d[k - 2:k + 1]), R.MAX)
    ref = VR.reference(got, truth_w, w)
    sn = part.scores_normalized[i]
    _check_sums(f"{which} gust window {i}", sn.sums, sn.rank_histogram, ref, setup.G, M)
    np.testing.assert_array_equal(part.scores[i].sums, sn.scaled(sd).sums)
    tab = ER.tables(got, truth_w, thr, events.directions, wq)
    e = part.events[i]
    np.testing.assert_array_equal(e.weighted, tab["weighted"], err_msg=f"{which} gust window {i}")
    np.testing.assert_array_equal(e.counts, tab["counts"])
    np.testing.assert_array_equal(e.invalid, tab["invalid"])
    assert e.n_members == M and e.scale == wq_scale and e.directions == (1, 1, -1)
    if which == "wrapper":                                  # (without the wrapper the states of this random model grow with
      assert (tab["counts"].sum(axis=(1, 2)) > 0).sum() > 3 * 2   # the lead time, past every threshold) not everything in one bin
  assert part.events[0].per_variable(part.template)["brier"]["10m_wind_speed"].shape == (3, SB, 1)

  # ---- everything else of the same run: the bytes of a run without `windows`
  for k in range(HORIZON):
    assert res.scores[k].sums.tobytes() == plain.scores[k].sums.tobytes()
    assert res.scores[k].rank_histogram.tobytes() == plain.scores[k].rank_histogram.tobytes()
    assert res.scores_normalized[k].sums.tobytes() == plain.scores_normalized[k].sums.tobytes()
    assert res.events[k].weighted.tobytes() == plain.events[k].weighted.tobytes()
    assert res.events[k].counts.tobytes() == plain.events[k].counts.tobytes()
    assert res.derived["wind"].scores[k].sums.tobytes() == plain.derived["wind"].scores[k].sums.tobytes()
    assert res.derived["wind"].scores_normalized[k].rank_histogram.tobytes() == plain.derived["wind"].scores_normalized[k].rank_histogram.tobytes()
    for m in range(M):
      assert res.members[k][m].tobytes() == plain.members[k][m].tobytes()
      assert res.derived["wind"].members[k][m].tobytes() == plain.derived["wind"].members[k][m].tobytes()

  # ---- two start dates add
  merged = res.merge(res)
  np.testing.assert_array_equal(merged.windows["gust"].events[1].weighted, 2 * res.windows["gust"].events[1].weighted)
  np.testing.assert_array_equal(merged.windows["acc"].scores[1].rank_histogram, 2 * res.windows["acc"].scores[1].rank_histogram)
  np.testing.assert_array_equal(merged.windows["acc"].scores_normalized[0].sums, 2 * res.windows["acc"].scores_normalized[0].sums)
  assert merged.windows["acc"].leads == [1, 3] and merged.windows["gust"].members is None
  with pytest.raises(ValueError, match="carries windows"):
    res.merge(plain)
  with pytest.raises(ValueError, match="names no entry"):
    er.run(*args, windows={"gust": gust})
  with pytest.raises(ValueError, match="world_size == 1"):
    rollout.EnsembleRollout(setup.gc, setup.norm(which), world_size=2).run(*args, windows={"acc": acc})
