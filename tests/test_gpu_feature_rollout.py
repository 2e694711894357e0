"""Feature detection through the stack: `EnsembleRollout.run(features=...)`, `GenCast.ensemble_features` and the wrappers'
on the small model of tests/test_gpu_events.py (9 x 16 grid, batch 2), with M = 3 and a horizon of 3.

The centres of every lead time are compared with tests/feature_reference.py applied to the kept member states and the truth
of that lead: counts, nodes and values are equal.  The scores, the event tables and the probability map of the strike store
are compared with `ens_score` / `ens_event_score` of the REFERENCE strike fields pushed into a plain store: the bytes are
equal.  The window on the strike store equals the host maximum of the kept strike fields."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import FeatureSpec, NaNCleaner, WindowSpec, datasets, link_tracks, rollout, verification
from gencast_flax_nnx_amd.verification import quantize_node_weights
from tests import feature_reference as R
from tests.helpers import graph_handle as _handle
from tests.test_gpu_events import SB, _Setup, _stack

pytestmark = pytest.mark.gpu

M, HORIZON = 3, 3
MSLP = "mean_sea_level_pressure"
R_LON = [7, 3, 2, 1, 1, 1, 2, 3, 7]                         # per latitude row, 90 S .. 90 N; 7 = (16 - 1) // 2: the whole row
RING_LON = [7, 5, 3, 2, 2, 2, 3, 5, 7]
STRIKE_LON = [7, 2, 1, 1, 1, 1, 1, 2, 7]


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  rng = np.random.default_rng(15)

  def stretch(ds):                                          # HORIZON frames of the setup's kind
    out = {}
    for k, v in ds.items():
      shape = list(v.data.shape)
      shape[v.dims.index("time")] = HORIZON
      out[k] = datasets.Variable(v.dims, rng.standard_normal(shape).astype(np.float32))
    return datasets.Dataset(out, ds.coords)

  s.targets, s.forcings = stretch(s.tgt1), stretch(s.frc1)
  yield s
  s.gc.denoiser.close()


def _spec(setup, which, max_centres=16):
  """A low of the MSLP below its climatological mean, half a scale deeper than its ring: about half of the minima pass."""
  s, l = setup.stats_per_channel(which)
  ch = {n: o for n, o, _ in datasets.channel_layout(setup.template0)}[MSLP]
  return FeatureSpec({"low": dict(variable=MSLP, kind="min", radius_km=(1, R_LON), threshold=float(l[ch]), ring_km=(2, RING_LON),
                                  depth=float(0.5 * s[ch]), strike_km=(1, STRIKE_LON))}, max_centres=max_centres), ch


def _reference_store(graph, strike, w, wq, thr):
  """(sums, hist, weighted, counts, invalid, mean) of reference strike fields [M + 1, G, B, D] in a plain store."""
  nd = _handle(graph, SB, strike.shape[-1])
  try:
    nd.ens_reserve(M)
    for i in range(M):
      nd.ens_push_host(i, strike[i])
    nd.ens_set_node_weight(w)
    nd.ens_event_set(thr, [1], wq)
    return nd.ens_score(strike[M], want_fields=True) + nd.ens_event_score(None) + nd.ens_download_fields()[:1]
  finally:
    nd.close()


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_rollout_features_equal_the_definition_on_the_kept_members(setup, which):
  spec, ch = _spec(setup, which)
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which), base_seed=3, concurrent_members=2)
  args = (setup.inp, setup.targets, setup.forcings, HORIZON, M)
  res = er.run(*args, keep_members=True, features={"low": spec},
               windows={"low3": WindowSpec("max", 2, stride=1, source="low")})
  plain = er.run(*args, keep_members=True)
  assert plain.features is None and "features" not in vars(plain) and sorted(res.features) == ["low"]
  part = res.features["low"]
  s, l = setup.stats_per_channel(which)
  plan = spec.plan(setup.template0, s, l)
  w = verification.node_weights(setup.template0)
  wq, wq_scale = quantize_node_weights(w)
  thr = spec.event_spec().packed(spec.template(setup.template0))
  assert thr.shape == (1, setup.G, SB, 1) and len(part.scores) == len(part.events) == len(part.centres) == HORIZON
  found = 0
  for k in range(HORIZON):
    fields = np.stack(list(res.members[k]) + [setup.truth(k, which)])
    count, node, value, strike = R.apply(fields, plan)
    got = part.centres[k]["low"]
    for b in range(SB):
      for z in range(M + 1):
        e, n = got[b][z], int(count[z, b, 0])
        assert e["count"] == n <= 16, (k, b, z)
        np.testing.assert_array_equal(e["node"], node[z, b, 0, :n])
        np.testing.assert_array_equal(e["value"], value[z, b, 0, :n].astype(np.float64) * s[ch] + l[ch])
        np.testing.assert_array_equal(e["lat"], setup.lat[node[z, b, 0, :n] // 16])
        np.testing.assert_array_equal(e["lon"], setup.lon[node[z, b, 0, :n] % 16])
        found += n
    np.testing.assert_array_equal(np.stack(part.members[k]), strike[:M])
    sums, hist, weighted, counts, invalid, mean = _reference_store(setup.gc.denoiser.graph, strike, w, wq, thr)
    sn, ev = part.scores_normalized[k], part.events[k]
    assert sn.sums.tobytes() == np.asarray(sums, np.float64).tobytes()
    assert sn.rank_histogram.tobytes() == np.asarray(hist, np.uint64).tobytes()
    assert part.scores[k].sums.tobytes() == sn.sums.tobytes()                # a strike field has no unit
    assert ev.weighted.tobytes() == np.asarray(weighted, np.uint64).tobytes()
    assert ev.counts.tobytes() == np.asarray(counts, np.uint64).tobytes()
    assert ev.invalid.tobytes() == np.asarray(invalid, np.uint64).tobytes()
    assert ev.n_members == M and ev.scale == wq_scale and ev.directions == (1,)
    prob = _stack(part.strike_probability[k])
    assert prob.tobytes() == mean.tobytes() and 0.0 <= prob.min() and prob.max() <= 1.0
  assert found > 2 * HORIZON * SB                           # there was something to find
  assert part.events[0].per_variable(spec.template(setup.template0))["brier"]["low"].shape == (1, SB, 1)
  # the window on the strike store: a strike within two steps is the host maximum of the kept strike fields
  win = res.windows["low3"]
  assert win.leads == [1, 2] and win.steps == 2
  for i, k in enumerate(win.leads):
    np.testing.assert_array_equal(np.stack(win.members[i]), np.maximum(np.stack(part.members[k - 1]), np.stack(part.members[k])))
  # tracks of member 0, batch entry 0: every centre lies on exactly one track
  tracks = link_tracks([part.centres[k]["low"][0][0] for k in range(HORIZON)], 3000.0)
  assert sum(len(t) for t in tracks) == sum(part.centres[k]["low"][0][0]["node"].size for k in range(HORIZON))
  # the merge over dates doubles the additive parts
  both = res.merge(res).features["low"]
  for k in range(HORIZON):
    np.testing.assert_array_equal(both.scores_normalized[k].sums, 2.0 * part.scores_normalized[k].sums)
    np.testing.assert_array_equal(both.scores_normalized[k].rank_histogram, 2 * part.scores_normalized[k].rank_histogram)
    np.testing.assert_array_equal(both.events[k].weighted, 2 * part.events[k].weighted)
  assert both.centres is None and res.merge(res).windows["low3"].leads == [1, 2]
  # everything else of the same run: the bytes of a run without `features`
  for k in range(HORIZON):
    assert res.scores[k].sums.tobytes() == plain.scores[k].sums.tobytes()
    assert res.scores[k].rank_histogram.tobytes() == plain.scores[k].rank_histogram.tobytes()
    assert res.scores_normalized[k].sums.tobytes() == plain.scores_normalized[k].sums.tobytes()
    for m in range(M):
      assert res.members[k][m].tobytes() == plain.members[k][m].tobytes()


def test_rollout_features_take_order_tails_and_regions_by_name(setup):
  spec, _ = _spec(setup, "none")
  er = rollout.EnsembleRollout(setup.gc, None, base_seed=3, concurrent_members=2)
  mask = np.zeros((9, 16), bool)
  mask[:5] = True
  res = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, features={"low": spec}, order=[0.5],
               tails={"low": verification.EventSpec({"low": np.array([0.5])}, [1])},
               regions={"low": verification.RegionSpec({"south": mask})})
  part = res.features["low"]
  assert len(part.order) == len(part.tails) == len(part.regions) == HORIZON and res.tails is None and res.regions is None
  assert part.regions[0]["south"].sums.shape == part.scores[0].sums.shape
  with pytest.raises(ValueError, match="name no entry"):
    er.run(setup.inp, setup.targets, setup.forcings, 1, M, features={"low": spec}, tails={"high": verification.EventSpec({"low": np.array([0.5])}, [1])})
  with pytest.raises(ValueError, match="its source 'high' names no entry"):
    er.run(setup.inp, setup.targets, setup.forcings, 2, M, features={"low": spec}, windows={"w": WindowSpec("max", 2, source="high")})


@pytest.mark.parametrize("which", ["none", "cleaner", "wrapper"])
def test_single_step_features_are_consistent_with_their_own_centres(setup, which):
  """`ensemble_features` keeps no member: the strike fields are rebuilt on the host from the listed centres (every list is
  complete here) and pushed into a plain store, whose scores, tables and mean field must be the result's, byte for byte."""
  spec, ch = _spec(setup, "wrapper" if which == "wrapper" else "none", max_centres=64)
  model = {"none": setup.gc, "cleaner": NaNCleaner(setup.gc, "2m_temperature", datasets.Dataset({"2m_temperature": datasets.Variable((), np.float32(0.25))})), "wrapper": setup.wrapper}[which]
  out = model.ensemble_features(setup.inp, setup.tgt1, setup.frc1, num_members=M, spec=spec, rngs=3)
  plan = spec.plan(setup.template0, *setup.stats_per_channel("wrapper" if which == "wrapper" else "none"))
  flags = np.zeros((M + 1, setup.G, SB), bool)
  for b in range(SB):
    for z in range(M + 1):
      e = out.truth_centres["low"][b] if z == M else out.centres["low"][b][z]
      assert e["count"] == e["node"].size <= 64
      flags[z, e["node"], b] = True
  assert flags[:M].sum() > 0 and sorted(out.centres) == sorted(out.truth_centres) == ["low"]
  strike = np.stack([R.strike(flags[z], np.ones((setup.G, SB), bool), plan, 0) for z in range(M + 1)])[..., None]
  w = verification.node_weights(setup.template0)
  wq, _ = quantize_node_weights(w)
  thr = spec.event_spec().packed(spec.template(setup.template0))
  sums, hist, weighted, counts, invalid, mean = _reference_store(setup.gc.denoiser.graph, strike, w, wq, thr)
  assert out.scores.sums.tobytes() == np.asarray(sums, np.float64).tobytes()
  assert out.scores.rank_histogram.tobytes() == np.asarray(hist, np.uint64).tobytes()
  assert out.events.weighted.tobytes() == np.asarray(weighted, np.uint64).tobytes()
  assert out.events.counts.tobytes() == np.asarray(counts, np.uint64).tobytes()
  assert _stack(datasets.as_dataset(out.strike_probability)).tobytes() == mean.tobytes()
  assert out.events.per_variable(out.template)["roc_area"]["low"].shape == (1, SB, 1)
  merged = verification.FeatureScores.merge([out, out])
  np.testing.assert_array_equal(merged.scores.sums, 2.0 * out.scores.sums)
  np.testing.assert_array_equal(merged.events.counts, 2 * out.events.counts)
