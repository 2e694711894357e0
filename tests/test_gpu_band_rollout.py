"""Spectral band views through the stack: `EnsembleRollout.run(derived={name: BandSpec})` and `GenCast.ensemble_derived` on the
small model of tests/test_gpu_events.py (9 x 16 grid, lmax 8, batch 2, HORIZON = 2, M = 3, both `norm` settings).

The kept band members are held to tests/band_reference.py applied to the kept main members, with the float32 tables the
product hands to the device and the derived bound of that module.  The scores of the band view are then compared, bit for bit,
with `ens_score` of a plain handle into which those kept band members were pushed.  The band truth has no download; the
truth goes through the same map as a member, so the test forms it by the same device call on two handles of its own -- two
calls give the same bytes -- and holds it to the reference as well."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import BandSpec, DerivedSpec, EventSpec, SphericalAnalysis, WindowSpec, _lib, datasets, rollout, verification
from tests import band_reference as R
from tests.test_gpu_events import HORIZON, SB, _Setup, _stack

pytestmark = pytest.mark.gpu

M = 3
N_LAT, N_LON, LMAX = 9, 16, 8
VARIABLES = ["2m_temperature", "geopotential"]
WIND = [("norm2", "10m_wind_speed", "10m_u_component_of_wind", "10m_v_component_of_wind"), ("copy", "2m_temperature")]


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  s.gc.denoiser.close()


def _mk(c):
  return _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=c + 4, c_out=c, batch=SB)


def _device_band(graph, plan, atabs, fields):
  """The device's own band fields of a stack [n >= 2, G, B, c_src] (the last one rides as the truth)."""
  src, dst = _mk(plan["c_src"]), _mk(len(plan["band"]))
  try:
    for h in (src, dst):
      h.set_graph(graph)
      h.ens_reserve(len(fields))
    for i, x in enumerate(fields):
      src.ens_push_host(i, x)
    dst.spec_set_tables(*atabs)
    dst.ens_band_set(**plan)
    dst.ens_band(src, fields[-1])
    return np.stack([dst.ens_download_member(i) for i in range(len(fields))])
  finally:
    src.close()
    dst.close()


def _plain_scores(graph, members, truth, w):
  h = _mk(members.shape[-1])
  try:
    h.set_graph(graph)
    h.ens_reserve(len(members))
    for i, x in enumerate(members):
      h.ens_push_host(i, x)
    h.ens_set_node_weight(w)
    return h.ens_score(truth)
  finally:
    h.close()


def _check_band_fields(tag, got, raw, plan, tabs):
  for i in range(len(got)):
    d, tol, _ = R.band_fields(raw[i], N_LAT, N_LON, plan["response"], plan["complement"], plan["src_channel"], plan["band"], *tabs)
    R.check(got[i], d, tol, f"{tag} field {i}")


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_rollout_band_view_matches_the_definition_and_scores_like_a_plain_store(setup, which):
  large = BandSpec({"lo": (0, 3)}, variables=VARIABLES)
  wind = DerivedSpec(WIND)
  tails = EventSpec({"2m_temperature_lo": np.array([0.25]), "geopotential_lo": np.array([0.0])}, [1])
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which), base_seed=3, concurrent_members=2)
  args = (setup.inp, setup.targets, setup.forcings, HORIZON, M)
  res = er.run(*args, keep_members=True, derived={"large": large, "wind": wind}, windows={"large2": WindowSpec("mean", 2, source="large")},
               order=(0.5,), tails={"large": tails})
  plain = er.run(*args, keep_members=True, derived={"wind": wind}, order=(0.5,))
  assert sorted(res.derived) == ["large", "wind"] and sorted(plain.derived) == ["wind"]
  s, l = setup.stats_per_channel(which)
  w = verification.node_weights(setup.template0)
  graph = setup.gc.denoiser.graph
  sa = SphericalAnalysis(setup.lat, setup.lon, LMAX)
  atabs, stabs = sa.device_tables(), sa.synthesis_tables()
  plan = large.plan(setup.template0, s, l)
  sd, ld = large.channel_stats(setup.template0, s, l)
  c_d = len(plan["band"])
  assert c_d == 14 and plan["response"].shape == (1, LMAX)
  lay = {n: (o, k) for n, o, k in datasets.channel_layout(setup.template0)}
  np.testing.assert_array_equal(sd, np.r_[s[lay["2m_temperature"][0]], s[lay["geopotential"][0]:lay["geopotential"][0] + 13]])
  np.testing.assert_array_equal(ld, np.r_[l[lay["2m_temperature"][0]], l[lay["geopotential"][0]:lay["geopotential"][0] + 13]])   # w[0] = 1
  part = res.derived["large"]
  assert len(part.scores) == len(part.members) == len(part.order) == len(part.tails) == HORIZON
  for k in range(HORIZON):
    raw, got = np.stack(res.members[k]), np.stack(part.members[k])
    assert got.shape == (M, setup.G, SB, c_d) and got.dtype == np.float32
    _check_band_fields(f"{which} lead {k}", got, raw, plan, (atabs, stabs))
    truth_raw = setup.truth(k, which)
    truth_d = _device_band(graph, plan, atabs, np.stack([truth_raw, truth_raw]))[0]
    _check_band_fields(f"{which} lead {k} truth", truth_d[None], truth_raw[None], plan, (atabs, stabs))
    sums, hist = _plain_scores(graph, got, truth_d, w)
    sn = part.scores_normalized[k]
    assert sn.sums.tobytes() == sums.tobytes() and sn.rank_histogram.tobytes() == hist.tobytes()
    np.testing.assert_array_equal(part.scores[k].sums, sn.scaled(sd).sums)
    # order statistics and the tail entry under the view's name: finite
    assert np.isfinite(part.order[k].crps_ensemble).all() and np.isfinite(part.tails[k].sums).all()
  pv = part.scores[0].per_variable(large.template(setup.template0))
  assert pv["crps"]["geopotential_lo"].shape == (SB, 13) and pv["crps"]["2m_temperature_lo"].shape == (SB, 1)
  # the window over the view emits once, at the last lead, and its members are the mean of the view's
  win = res.windows["large2"]
  assert list(win.leads) == [1] and len(win.scores) == len(win.members) == 1 and np.isfinite(win.scores[0].sums).all()
  mean2 = 0.5 * (np.stack(part.members[0]).astype(np.float64) + np.stack(part.members[1]).astype(np.float64))
  np.testing.assert_allclose(np.stack(win.members[0]), mean2, rtol=1e-6, atol=1e-6 * np.abs(mean2).max())
  # everything else of the same run: the bytes of a run without the band entry
  for k in range(HORIZON):
    assert res.scores[k].sums.tobytes() == plain.scores[k].sums.tobytes()
    assert res.scores[k].rank_histogram.tobytes() == plain.scores[k].rank_histogram.tobytes()
    assert res.order[k].crps_ensemble.tobytes() == plain.order[k].crps_ensemble.tobytes()
    a, b = res.derived["wind"], plain.derived["wind"]
    assert a.scores[k].sums.tobytes() == b.scores[k].sums.tobytes()
    assert a.scores_normalized[k].rank_histogram.tobytes() == b.scores_normalized[k].rank_histogram.tobytes()
    for m in range(M):
      assert res.members[k][m].tobytes() == plain.members[k][m].tobytes()
      assert a.members[k][m].tobytes() == b.members[k][m].tobytes()


def test_single_step_band_scores_agree_with_the_raw_kernels(setup):
  from gencast_flax_nnx_amd import EnsembleSampler
  spec = BandSpec({"lo": (0, 2), "rest": dict(l=(0, 2), complement=True)}, variables=VARIABLES, taper=0.5)
  gc, inp, tgt, frc = setup.gc, setup.inp, setup.tgt1, setup.frc1
  ens = EnsembleSampler(gc._sampler, base_seed=5, concurrent_members=2)
  fields = np.stack([_stack(d) for _, d in sorted(ens(inp, tgt.map(np.zeros_like), frc, M), key=lambda t: t[0])])
  plan = spec.plan(tgt)
  atabs = SphericalAnalysis(setup.lat, setup.lon, LMAX).device_tables()
  band = _device_band(gc.denoiser.graph, plan, atabs, np.concatenate([fields, _stack(tgt)[None]]))
  w = verification.node_weights(tgt)
  got = gc.ensemble_derived(inp, tgt, frc, num_members=M, spec=spec, rngs=5, concurrent_members=2)
  sums, hist = _plain_scores(gc.denoiser.graph, band[:M], band[M], w)
  assert got.sums.tobytes() == sums.tobytes() and got.rank_histogram.tobytes() == hist.tobytes()
  assert got.sums.shape[1] == 28 and np.isfinite(got.crps).all()


def test_a_band_view_is_scored_against_the_band_climatology(setup):
  """The climatology path of a band view: the K samples in the main climatology handle's store go through the view's band plan
  into a climatology view of the entry's own, and `gc_ens_clim_score` reads both band stores."""
  K, which = 3, "wrapper"
  rng = np.random.default_rng(17)

  def like(ds):
    return datasets.Dataset({k: datasets.Variable(v.dims, np.asarray(v.data, np.float32) + rng.standard_normal(np.shape(v.data)).astype(np.float32))
                             for k, v in ds.items()}, ds.coords)

  def packed(ds):
    y = np.transpose(datasets.dataset_to_stacked(ds, ds.sizes), (1, 2, 0, 3)).reshape(setup.G, SB, -1)
    return setup.normalised(y, which)

  clim = [[like(rollout.isel_time(setup.targets, slice(k, k + 1))) for _ in range(K)] for k in range(HORIZON)]
  large = BandSpec({"lo": (0, 3)}, variables=VARIABLES)
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which), base_seed=3)
  res = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, keep_members=True, derived={"large": large}, climatology=clim)
  d = res.derived["large"]
  assert len(d.climatology) == len(d.climatology_normalized) == HORIZON
  den = setup.gc.denoiser
  view, cview = den.band_handle(14, "large"), den.climatology_handle(14, view=True, key="band:large")
  assert cview is not den.climatology_handle(14, view=True)
  k = HORIZON - 1
  raw = d.climatology_normalized[k]
  assert raw.sums.shape == (SB, 14, 12) and (raw.n_members, raw.n_climatology) == (M, K) and np.isfinite(raw.sums).all()
  # the samples the device kept in the climatology view: the band fields of the lead's samples in the members' units
  s, l = setup.stats_per_channel(which)
  plan = large.plan(setup.template0, s, l)
  atabs = SphericalAnalysis(setup.lat, setup.lon, LMAX).device_tables()
  samples = np.stack([packed(c) for c in clim[k]])
  want = _device_band(den.graph, plan, atabs, samples)
  for j in range(K):
    assert cview.ens_download_member(j).tobytes() == want[j].tobytes()
  # and the score is the one of the two band stores as they stand
  sums, counts, invalid = view.ens_clim_score(cview, None)
  assert sums.tobytes() == raw.sums.tobytes() and counts.tobytes() == raw.counts.tobytes()
  np.testing.assert_array_equal(view.ens_download_member(0), d.members[k][0])
  sd, _ = large.channel_stats(setup.template0, s, l)
  np.testing.assert_array_equal(d.climatology[k].sums, raw.scaled(sd).sums)
