"""Derived and pooled fields through the stack: `EnsembleRollout.run(derived=...)` and `GenCast.ensemble_derived` on the
small model of tests/test_gpu_events.py (9 x 16 grid, batch 2, HORIZON = 2, M = 3, both `norm` settings).

The kept derived members are compared with tests/derive_reference.py applied to the kept raw members, op by op: a copy
channel under MAX pooling is exact; a norm2 channel carries the one float32 ulp of its norm through the maximum; MEAN
carries the bound of its prefix sum.  The scores and the event tables of a derived store are then compared with
verification_reference / event_reference applied to THOSE kept derived members (sums within `sum_tolerance`, tables ==).
The derived truth has no download; the test forms it by the same device call on two handles of its own -- two calls give
the same bytes -- and holds it to the reference with the same per-op tolerances."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import DerivedSpec, EnsembleSampler, EventSpec, _lib, config, datasets, rollout, verification
from gencast_flax_nnx_amd.verification import quantize_node_weights
from tests import derive_reference as R
from tests import event_reference as ER
from tests import verification_reference as VR
from tests.test_gpu_events import HORIZON, SB, SC, _Setup, _stack
from tests.test_gpu_verification import _check_sums

pytestmark = pytest.mark.gpu

M = 3
N_LAT, N_LON = 9, 16
WIND = [("norm2", "10m_wind_speed", "10m_u_component_of_wind", "10m_v_component_of_wind"),
        ("norm2", "wind_speed", "u_component_of_wind", "v_component_of_wind"), ("copy", "2m_temperature")]
WIND_R_LON = [7, 3, 2, 1, 1, 1, 2, 3, 7]                    # per latitude row, 90 S .. 90 N; 7 = (16 - 1) // 2: the whole row
SMOOTH_R_LON = [7, 5, 3, 2, 2, 2, 3, 5, 7]


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  s.gc.denoiser.close()


def _specs():
  wind = DerivedSpec(WIND, pool="max", r_lat=1, r_lon=WIND_R_LON)
  events = EventSpec({"10m_wind_speed": np.array([1.5, 2.5, 1.0]),
                      "wind_speed": np.array([1.5, 2.5, 1.0]).reshape(3, 1, 1, 1) * np.linspace(0.8, 1.2, 13).reshape(1, 13, 1, 1),
                      "2m_temperature": np.array([0.5, 1.0, 0.0])}, [1, 1, -1])
  smooth = DerivedSpec([("copy", v) for v in config.TASK.target_variables], pool="mean", r_lat=2, r_lon=SMOOTH_R_LON)
  return wind, events, smooth


def _device_derive(graph, plan, fields):
  """The device's own derived fields of a stack [n >= 2, G, B, c_src] (the last one rides as the truth)."""
  c_src, c_d, n = plan["c_src"], len(plan["op"]), len(fields)
  mk = lambda c: _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=c + 4, c_out=c, batch=SB)
  src, dst = mk(c_src), mk(c_d)
  try:
    for h in (src, dst):
      h.set_graph(graph)
      h.ens_reserve(n)
    for i, x in enumerate(fields):
      src.ens_push_host(i, x)
    dst.ens_derive_set(**plan)
    dst.ens_derive(src, fields[-1])
    return np.stack([dst.ens_download_member(i) for i in range(n)])
  finally:
    src.close()
    dst.close()


def _check_derived_fields(tag, got, raw, plan):
  """got [n, G, B, c_d] against the reference of raw [n, G, B, c_src], op by op."""
  ref = R.apply(raw, plan)
  op = np.asarray(plan["op"])
  if plan["pool"] == R.MEAN:
    d = R.derive(raw, plan["op"], plan["src_a"], plan["src_b"], plan["affine"])
    err, bound = np.abs(got.astype(np.float64) - ref), R.mean_bound(d, ref, plan["n_lon"])
    print(f"{tag}: mean, worst error / bound {float((err / bound).max()):.3g}")
    assert np.all(err <= bound), tag
    return
  np.testing.assert_array_equal(got[..., op == 0], ref[..., op == 0], err_msg=f"{tag}: copy channels")
  g, r = got[..., op == 1], ref[..., op == 1]
  assert np.all(np.abs(g.astype(np.float64) - r.astype(np.float64)) <= np.spacing(r)), f"{tag}: norm2 channels"


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_rollout_derived_scores_and_events_equal_the_definitions_on_the_kept_members(setup, which):
  wind, events, smooth = _specs()
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which), base_seed=3, concurrent_members=2)
  args = (setup.inp, setup.targets, setup.forcings, HORIZON, M)
  res = er.run(*args, keep_members=True, events=setup.spec, derived={"wind": (wind, events), "smooth": smooth})
  plain = er.run(*args, keep_members=True, events=setup.spec)
  assert plain.derived is None and sorted(res.derived) == ["smooth", "wind"]
  s, l = setup.stats_per_channel(which)
  w = verification.node_weights(setup.template0)
  wq, wq_scale = quantize_node_weights(w)
  graph = setup.gc.denoiser.graph
  for name, spec, ev in (("wind", wind, events), ("smooth", smooth, None)):
    part = res.derived[name]
    plan = spec.plan(setup.template0, s, l)
    sd, ld = spec.channel_stats(setup.template0, s, l)
    c_d = len(plan["op"])
    assert c_d == (15 if name == "wind" else SC) and len(part.scores) == len(part.members) == HORIZON
    assert (part.events is None) == (ev is None)
    for k in range(HORIZON):
      raw = np.stack(res.members[k])
      got = np.stack(part.members[k])
      assert got.shape == (M, setup.G, SB, c_d) and got.dtype == np.float32
      _check_derived_fields(f"{which} {name} lead {k}", got, raw, plan)
      truth_raw = setup.truth(k, which)
      truth_d = _device_derive(graph, plan, np.stack([truth_raw, truth_raw]))[0]
      _check_derived_fields(f"{which} {name} lead {k} truth", truth_d[None], truth_raw[None], plan)
      ref = VR.reference(got, truth_d, w)
      sn = part.scores_normalized[k]
      _check_sums(f"{which} {name} lead {k}", sn.sums, sn.rank_histogram, ref, setup.G, M)
      np.testing.assert_array_equal(part.scores[k].sums, sn.scaled(sd).sums)
      if ev is not None:
        thr = ev.packed(spec.template(setup.template0))
        if which == "wrapper":
          thr = ((thr.astype(np.float64) - ld) / sd).astype(np.float32)
        tab = ER.tables(got, truth_d, thr, ev.directions, wq)
        e = part.events[k]
        np.testing.assert_array_equal(e.weighted, tab["weighted"], err_msg=f"{which} {name} lead {k}")
        np.testing.assert_array_equal(e.counts, tab["counts"])
        np.testing.assert_array_equal(e.invalid, tab["invalid"])
        assert e.n_members == M and e.scale == wq_scale and e.directions == (1, 1, -1)
        assert (tab["counts"].sum(axis=(1, 2)) > 0).sum() > 3 * 2                  # not everything in one bin
    pv = part.scores[0].per_variable(spec.template(setup.template0))
    assert pv["crps"]["wind_speed" if name == "wind" else "temperature"].shape == (SB, 13)
  assert res.derived["wind"].events[0].per_variable(wind.template(setup.template0))["brier"]["10m_wind_speed"].shape == (3, SB, 1)
  # wind speed is in physical units whatever the normalisation: the norm of the un-normalised kept components
  lay = {n: o for n, o, _ in datasets.channel_layout(setup.template0)}
  u, v = lay["10m_u_component_of_wind"], lay["10m_v_component_of_wind"]
  raw = np.stack(res.members[0]).astype(np.float64)
  speed = np.hypot(raw[..., u] * s[u] + l[u], raw[..., v] * s[v] + l[v])
  assert np.all(np.stack(res.derived["wind"].members[0])[..., 0] >= speed * (1 - 1e-6))   # the pooled maximum is no less
  # everything else of the same run: the bytes of a run without `derived`
  for k in range(HORIZON):
    assert res.scores[k].sums.tobytes() == plain.scores[k].sums.tobytes()
    assert res.scores[k].rank_histogram.tobytes() == plain.scores[k].rank_histogram.tobytes()
    assert res.scores_normalized[k].sums.tobytes() == plain.scores_normalized[k].sums.tobytes()
    assert res.events[k].weighted.tobytes() == plain.events[k].weighted.tobytes()
    assert res.events[k].counts.tobytes() == plain.events[k].counts.tobytes()
    for m in range(M):
      assert res.members[k][m].tobytes() == plain.members[k][m].tobytes()
  merged = res.merge(res)
  np.testing.assert_array_equal(merged.derived["wind"].events[1].weighted, 2 * res.derived["wind"].events[1].weighted)
  np.testing.assert_array_equal(merged.derived["smooth"].scores[1].rank_histogram, 2 * res.derived["smooth"].scores[1].rank_histogram)
  with pytest.raises(ValueError, match="carries derived"):
    res.merge(plain)
  with pytest.raises(ValueError, match="world_size == 1"):
    rollout.EnsembleRollout(setup.gc, setup.norm(which), world_size=2).run(*args, derived={"smooth": smooth})


def test_two_entries_of_one_width_share_a_view_handle(setup):
  t2 = DerivedSpec([("copy", "2m_temperature")], pool="max", r_lat=1, r_lon=WIND_R_LON)
  mslp = DerivedSpec([("copy", "mean_sea_level_pressure")], pool="min", r_lat=1, r_lon=WIND_R_LON)
  er = rollout.EnsembleRollout(setup.gc, None, base_seed=3)
  res = er.run(setup.inp, setup.targets, setup.forcings, 1, M, keep_members=True, derived={"warm": t2, "low": mslp})
  raw = np.stack(res.members[0])
  for name, spec in (("warm", t2), ("low", mslp)):
    np.testing.assert_array_equal(np.stack(res.derived[name].members[0]), R.apply(raw, spec.plan(setup.template0)))
  assert setup.gc.denoiser.view_handle(1) is setup.gc.denoiser.view_handle(1)


def test_single_step_derived_agrees_with_the_raw_kernels(setup):
  wind, events, _ = _specs()
  gc, inp, tgt, frc = setup.gc, setup.inp, setup.tgt1, setup.frc1
  ens = EnsembleSampler(gc._sampler, base_seed=5, concurrent_members=2)
  fields = np.stack([_stack(d) for _, d in sorted(ens(inp, tgt.map(np.zeros_like), frc, M), key=lambda t: t[0])])
  plan = wind.plan(tgt)
  w = verification.node_weights(tgt)
  wq, scale = quantize_node_weights(w)
  derived = _device_derive(gc.denoiser.graph, plan, np.concatenate([fields, _stack(tgt)[None]]))
  _check_derived_fields("single step", derived, np.concatenate([fields, _stack(tgt)[None]]), plan)
  got_scores, got_events = gc.ensemble_derived(inp, tgt, frc, num_members=M, spec=wind, events=events, rngs=5, concurrent_members=2)
  ref = VR.reference(derived[:M], derived[M], w)
  _check_sums("single step", got_scores.sums, got_scores.rank_histogram, ref, setup.G, M)
  tab = ER.tables(derived[:M], derived[M], events.packed(wind.template(tgt)), events.directions, wq)
  np.testing.assert_array_equal(got_events.weighted, tab["weighted"])
  np.testing.assert_array_equal(got_events.counts, tab["counts"])
  np.testing.assert_array_equal(got_events.invalid, tab["invalid"])
  assert got_events.scale == scale and got_events.n_members == M
  only = ens.derived(inp, tgt, frc, M, wind)
  assert only.sums.tobytes() == got_scores.sums.tobytes()
  with pytest.raises(ValueError, match="ens_push_host"):
    EnsembleSampler(gc._sampler, rank=0, world_size=2).derived(inp, tgt, frc, M, wind)
  # the normalisation wrappers have no such method: under them a single-step sample is a residual
  from gencast_flax_nnx_amd import NaNCleaner
  assert not hasattr(setup.wrapper, "ensemble_derived") and not hasattr(NaNCleaner, "ensemble_derived")
