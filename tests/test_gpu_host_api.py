"""The reference-shaped Python surface on a real GPU: Denoiser / Sampler / GenCast
with Datasets in and out."""
import dataclasses

import numpy as np
import pytest

from gencast_flax_nnx_amd import Denoiser, GenCast, config, datasets, synthetic, weights
from gencast_flax_nnx_amd.denoiser import dims_from_arch
from oracle import gencast_oracle as O
from tests import helpers

pytestmark = pytest.mark.gpu


def _small_arch():
  arch = config.nano_architecture(mesh_size=2, d_model=128, num_layers=2, num_heads=2)
  arch.sparse_transformer_config.ffw_hidden = 256
  arch.sparse_transformer_config.attention_k_hop = 2
  return dataclasses.replace(arch, node_output_size=82)


def test_denoiser_call_contract_matches_oracle():
  arch = _small_arch()
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=2, seed=1)
  dims = dims_from_arch(arch, 262, 82)
  params = weights.random_params(dims, seed=3)
  den = Denoiser(None, arch, params)
  sigma = np.array([0.7, 12.0], np.float32)
  out = den(inp, tgt, sigma, frc)
  assert sorted(out.keys()) == sorted(tgt.keys())
  for k in tgt.keys():
    assert out[k].dims == tgt[k].dims and out[k].data.shape == tgt[k].data.shape
  feats, grid_shape, *_ = Denoiser.pack_inputs(inp, frc.assign(tgt))
  y = O.denoiser_forward(params, helpers.graph_dict(den.graph), feats, sigma, num_layers=2,
                         num_heads=2, attention="dense")
  want = Denoiser.unpack_outputs(y, grid_shape, tgt)
  for k in tgt.keys():
    assert np.abs(out[k].data - want[k].data).max() < 1e-4
  # lazy init fixed the data width (gencast/denoiser.py:630-632)
  fewer = datasets.Dataset({k: v for k, v in list(inp.items())[1:]}, inp.coords)
  with pytest.raises(AssertionError, match="Runtime data width changed"):
    den(fewer, tgt, sigma, frc)
  den.native.close()


def test_denoiser_with_two_hidden_layers_matches_oracle():
  """DenoiserArchitectureConfig(hidden_layers=2) (gencast/denoiser.py:135,374,402) through the Denoiser call contract:
  parameter names gain `layers.4`, the result follows the oracle's N-hidden-layer MLP (common/mlp.py:157-199)."""
  import dataclasses
  arch = dataclasses.replace(_small_arch(), hidden_layers=2)
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=2, seed=1)
  dims = dims_from_arch(arch, 262, 82)
  assert dims.hidden_layers == 2
  params = weights.random_params(dims, seed=3)
  den = Denoiser(None, arch, params)
  sigma = np.array([0.7, 12.0], np.float32)
  out = den(inp, tgt, sigma, frc)
  feats, grid_shape, *_ = Denoiser.pack_inputs(inp, frc.assign(tgt))
  y = O.denoiser_forward(params, helpers.graph_dict(den.graph), feats, sigma, num_layers=2, num_heads=2, attention="dense")
  want = Denoiser.unpack_outputs(y, grid_shape, tgt)
  for k in tgt.keys():
    assert np.abs(out[k].data - want[k].data).max() < 1e-4
  den.native.close()


def test_denoiser_on_an_injected_foreign_graph_matches_the_oracle_on_that_graph():
  """VERDICT r2 item 8 / SURVEY a21: a checkpoint trained on the reference's graph has to run on the reference's
  index arrays -- mesh nodes in ANOTHER numbering (the reference's is RCM, gencast/denoiser.py:849-867), edges in
  another order, and a mesh->grid assignment that differs from this build's where trimesh breaks ties differently
  (gencast/denoiser.py:443-600).  Build such arrays (random renumbering, shuffled edge lists, 25 grid points
  re-assigned to other faces), inject them through `Denoiser(graph=...)`, and compare the device result with the
  oracle evaluated on the injected arrays; the same model on the built graph must give ANOTHER answer."""
  from gencast_flax_nnx_amd import geometry
  arch = _small_arch()
  lat, lon = np.linspace(-90, 90, 13), np.arange(24) * 15.0
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=2, seed=4)
  params = weights.random_params(dims_from_arch(arch, 262, 82), seed=3)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=2, attention_k_hop=2)
  rng = np.random.default_rng(11)
  M, G = gr.num_mesh_nodes, gr.num_grid_nodes
  perm = rng.permutation(M)                                  # new id -> old id
  inv = np.empty(M, np.int64)
  inv[perm] = np.arange(M)
  mesh = geometry.get_last_triangular_mesh_for_sphere(2)
  m_lat, m_lon = geometry.mesh_nodes_lat_lon(mesh)
  m2g_s = gr.m2g_senders.reshape(G, 3).copy()                # three mesh vertices per grid point
  assert np.array_equal(gr.m2g_receivers, np.repeat(np.arange(G), 3))
  moved = rng.choice(G, 25, replace=False)
  m2g_s[moved] = mesh.faces[rng.integers(0, len(mesh.faces), 25)]
  e1, e2 = rng.permutation(len(gr.g2m_senders)), rng.permutation(3 * G)
  foreign = geometry.graph_from_reference_arrays(
      grid_lat=lat, grid_lon=lon, mesh_nodes_lat=m_lat[perm], mesh_nodes_lon=m_lon[perm],
      g2m_senders=gr.g2m_senders[e1], g2m_receivers=inv[gr.g2m_receivers][e1],
      m2g_senders=inv[m2g_s.reshape(-1)][e2], m2g_receivers=gr.m2g_receivers[e2],
      mesh_senders=inv[gr.mesh_senders], mesh_receivers=inv[gr.mesh_receivers], attention_k_hop=2)
  den = Denoiser(None, arch, params, graph=foreign)
  sigma = np.array([0.7, 12.0], np.float32)
  out = den(inp, tgt, sigma, frc)
  assert den.graph is foreign
  feats, grid_shape, *_ = Denoiser.pack_inputs(inp, frc.assign(tgt))
  y = O.denoiser_forward(params, helpers.graph_dict(foreign), feats, sigma, num_layers=2, num_heads=2,
                         attention="neighbour")
  want = Denoiser.unpack_outputs(y, grid_shape, tgt)
  worst = max(float(np.abs(out[k].data - want[k].data).max()) for k in tgt.keys())
  assert worst < 1e-4, worst
  y_built = O.denoiser_forward(params, helpers.graph_dict(gr), feats, sigma, num_layers=2, num_heads=2, attention="neighbour")
  assert np.abs(y_built - y).max() > 1e-2                    # the re-assigned grid points matter: it IS another graph
  den.native.close()


def test_gencast_full_sampling_end_to_end():
  arch = _small_arch()
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  sc = config.SamplerConfig(num_noise_levels=5, stochastic_churn_rate=0.0)
  params = weights.random_params(dims_from_arch(arch, 262, 82), seed=3)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=7)
  gc._sampler.noise_kind = "white"       # the oracle leg below redraws white noise from the same seed
  tmpl = datasets.zeros_like(tgt)
  out = gc.full_sampling(inp, tmpl, frc)
  assert gc._sampler.last_stats["denoiser_calls"] == 9
  for k in tgt.keys():
    assert out[k].data.shape == tgt[k].data.shape and np.isfinite(out[k].data).all()
  # oracle sampler on the same packed arrays and the same noise
  den = gc.denoiser
  cond, grid_shape, slots = den.init_for(inp, tmpl, frc)
  noise = np.random.default_rng(7).standard_normal((cond.shape[0], 1, 82), dtype=np.float32)
  net = lambda f, s: O.denoiser_forward(params, helpers.graph_dict(den.graph), f, s, num_layers=2,
                                        num_heads=2, attention="dense")
  ref, _ = O.dpm_solver_2s_sample(net, cond.astype(np.float64), slots, noise.astype(np.float64),
                                  O.noise_schedule(80.0, 0.03, 5, 7.0), skip_dead_call=True)
  want = Denoiser.unpack_outputs(ref, grid_shape, tmpl)
  scale = max(1.0, np.abs(ref).max())
  for k in tgt.keys():
    assert np.abs(out[k].data - want[k].data).max() < 1e-4 * scale
  den.native.close()


def test_device_rollout_matches_host_composed_rollout():
  """the context update done on the device by gc_rollout_advance gives the same
  forecasts as re-normalising and re-packing the host-composed context every step (same noise)."""
  from gencast_flax_nnx_amd import rollout
  from tests.test_rollout import _stats
  arch = _small_arch()
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  horizon = 3
  inp, tgt1, frc1 = synthetic.make_example(lat=lat, lon=lon, batch=2, seed=4)
  rng = np.random.default_rng(5)

  def stretch(ds, nt):
    out = {}
    for k, v in ds.items():
      shape = list(v.data.shape)
      shape[v.dims.index("time")] = nt
      out[k] = datasets.Variable(v.dims, rng.standard_normal(shape).astype(np.float32))
    return datasets.Dataset(out, ds.coords)

  targets, forcings = stretch(tgt1, horizon), stretch(frc1, horizon)
  sc = config.SamplerConfig(num_noise_levels=4, stochastic_churn_rate=0.0)
  params = weights.random_params(dims_from_arch(arch, 262, 82), seed=3)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=1)
  stats = _stats(config.TASK)
  G = len(lat) * len(lon)
  noises = [rng.standard_normal((G, 2, 82)).astype(np.float32) for _ in range(horizon)]
  for norm in (rollout.InputsAndResiduals(gc, *stats), None):
    model = norm if norm is not None else gc
    _, host, _ = rollout.autoregressive_rollout(model, inp, targets, forcings, horizon, init_noise=noises)
    dev = rollout.DeviceRollout(gc, norm).run(inp, targets, forcings, horizon, init_noise=noises)
    for k in tgt1.keys():
      assert dev[k].data.shape == host[k].data.shape == targets[k].data.shape
      scale = max(1.0, float(np.abs(host[k].data).max()))
      assert np.abs(dev[k].data - host[k].data).max() < 2e-4 * scale, k
  # the plan needs a sample and a conditioning on the device, and valid indices
  nd = gc.denoiser.native
  plan, _ = rollout.build_rollout_plan(rollout.isel_time(inp, slice(-2, None)), rollout.isel_time(forcings, slice(0, 1)),
                                       datasets.zeros_like(tgt1), config.TASK, None)
  bad = dict(plan)
  bad["kind"] = plan["kind"].copy()
  bad["kind"][0] = 9
  with pytest.raises(ValueError, match="kind"):
    nd.rollout_plan(**bad)
  with pytest.raises(ValueError, match="forcings"):
    nd.rollout_plan(**plan)
    nd.rollout_advance(np.zeros((G, 2, 3), np.float32))
  nd.close()


def test_rollout_advance_matches_the_rollout_oracle():
  """SURVEY.md 8f row 1 against the ORACLE (not the product's own host rollout): after a resident sample,
  gc_rollout_advance's new conditioning equals oracle/rollout_oracle.apply_plan applied to the old
  conditioning, the downloaded sample and the next forcings -- with the normalisation wrapper (kinds
  1, 2, 3) and without it (kinds 1, 3, 4)."""
  from gencast_flax_nnx_amd import rollout
  from oracle import rollout_oracle as RO
  from tests.test_rollout import _stats
  arch = _small_arch()
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=2, seed=6)
  sc = config.SamplerConfig(num_noise_levels=3, stochastic_churn_rate=0.0)
  params = weights.random_params(dims_from_arch(arch, 262, 82), seed=3)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=1)
  tmpl = datasets.zeros_like(tgt)
  den = gc.denoiser
  cond, grid_shape, slots = den.init_for(inp, tmpl, frc)
  nd = den.native
  nd.set_noisy_slots(slots)
  rng = np.random.default_rng(9)
  G = cond.shape[0]
  sig = np.asarray(gc._sampler.noise_levels, np.float32)
  for norm in (rollout.InputsAndResiduals(gc, *_stats(config.TASK)), None):
    plan, forcing_cols = rollout.build_rollout_plan(rollout.isel_time(inp, slice(-2, None)), frc, tmpl,
                                                    config.TASK, norm)
    kinds = set(plan["kind"].tolist())
    assert kinds >= ({1, 2, 3} if norm is not None else {1, 3, 4})
    nd.rollout_plan(**plan)
    nd.upload_cond(cond)
    nd.upload_noise(rng.standard_normal((G, 2, 82)).astype(np.float32))
    nd.sample_resident(sig, skip_dead_call=True, want_stats=False)
    sample = nd.download_sample()
    forc = rng.standard_normal((G, 2, plan["n_forcing"])).astype(np.float32)
    nd.rollout_advance(forc)
    got = nd.download_cond()
    want = RO.apply_plan(cond.astype(np.float64), sample.astype(np.float64), forc.astype(np.float64), plan)
    keep = np.ones(cond.shape[-1], bool)
    keep[slots] = False                                    # the sampler rewrites the noisy-target slots
    scale = max(1.0, float(np.abs(want[..., keep]).max()))
    assert np.abs(got[..., keep] - want[..., keep]).max() < 2e-6 * scale
    # second step: the plan composes (advance twice == apply_plan twice on the same sample)
    nd.rollout_advance(forc)
    want2 = RO.apply_plan(want, sample.astype(np.float64), forc.astype(np.float64), plan)
    assert np.abs(nd.download_cond()[..., keep] - want2[..., keep]).max() < 4e-6 * scale
  nd.close()


def test_sampler_draws_spherical_noise_by_default():
  """On an equiangular-with-poles grid the initial state is the reference's isotropic spherical
  white noise (noise.py); the sample equals the one obtained by passing that field explicitly."""
  from gencast_flax_nnx_amd import noise
  arch = _small_arch()
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  sc = config.SamplerConfig(num_noise_levels=3, stochastic_churn_rate=0.0)
  params = weights.random_params(dims_from_arch(arch, 262, 82), seed=3)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=11)
  tmpl = datasets.zeros_like(tgt)
  out = gc.full_sampling(inp, tmpl, frc)
  field = noise.packed_noise(noise.SphericalNoise(lat, lon), np.random.default_rng(11), 1, 82)
  ref = gc.full_sampling(inp, tmpl, frc, init_noise=field)
  for k in tgt.keys():
    np.testing.assert_array_equal(out[k].data, ref[k].data)
  gc.denoiser.native.close()


def test_device_noise_matches_the_noise_oracle():
  """SURVEY.md 8f row 2 on the device: gc_noise_draw's field for (seed, stream) against the oracle's Philox +
  direct spherical-harmonic evaluation (no shared tables), stream bookkeeping, unit variance incl. the poles."""
  from oracle import noise_oracle as NO
  from gencast_flax_nnx_amd import noise
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=2)                  # 13 x 24 grid: equiangular with poles
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    lat, lon = np.linspace(-90, 90, 13), np.arange(24) * 15.0
    gen = noise.SphericalNoise(lat, lon)
    with pytest.raises(Exception, match="gc_noise_set_tables"):
      nd.noise_draw()
    nd.noise_set_tables(13, 24, *gen.device_tables())
    N = 2 * dims.c_out
    for seed, stream in ((5, 0), (5, 1), (2 ** 40 + 3, 7)):
      nd.noise_seed(seed, stream)
      nd.noise_draw()
      got = nd.download_noise().reshape(-1, N)
      want = NO.device_field(seed, stream, lat, lon, N)
      assert np.abs(got - want).max() < 2e-5, (seed, stream)
    nd.noise_seed(5, 0)
    nd.noise_draw()
    nd.noise_draw()                                                          # second draw = stream 1
    np.testing.assert_allclose(nd.download_noise().reshape(-1, N), NO.device_field(5, 1, lat, lon, N), atol=2e-5)
    acc = np.zeros((13 * 24, N))
    for k in range(200):
      nd.noise_draw()
      f = nd.download_noise().reshape(-1, N).astype(np.float64)
      acc += f * f
    var = (acc / 200).mean(axis=1)
    assert np.abs(var - 1).max() < 0.2 and abs(var[:24].mean() - 1) < 0.15   # poles are row 0 / row 12
    with pytest.raises(ValueError, match="n_lat"):
      nd.noise_set_tables(12, 24, *gen.device_tables())
  finally:
    nd.close()


def _factorised_field(gen, seed, stream, N):
  """The two-step synthesis of csrc/gc_noise.hip in float64 NumPy from the SAME tables and the oracle's Philox normals
  (grids where the direct harmonic evaluation overflows: P_l^m beyond l ~ 150)."""
  from oracle import noise_oracle as NO
  leg, ct, st = (a.astype(np.float64) for a in gen.device_tables())          # [L, lat, L], [lon, L], [lon, L]
  L = leg.shape[0]
  z = NO.philox_normals(2 * L * L * N, seed, stream).reshape(2, L, L, N).astype(np.float64)
  f = np.matmul(leg[None], z)                                                 # Legendre step: [2, m, lat, N]
  n_lat, n_lon = leg.shape[1], ct.shape[0]
  out = ct @ f[0].reshape(L, -1) + st @ f[1].reshape(L, -1)                   # Fourier step: [lon, lat * N]
  return np.transpose(out.reshape(n_lon, n_lat, N), (1, 0, 2)).reshape(-1, N)


@pytest.mark.parametrize("case", ["three_degree_five_members_of_82_channels", "one_degree_batch_2", "half_degree_grid"])
def test_device_noise_has_no_size_cap(case):
  """Round 4's Fourier kernel staged [2][L][B c_out] floats in LDS and refused more than 160 KB (1 degree with batch 2:
  236 KB) and n_lat > 192; gencast/samplers_utils.py:250-346,434-452 has no such limit and the reference's default sampler
  churns.  Now: wavenumber chunks of 64 columns through a fixed 64 KB, latitudes in blocks of 192.
    * 3 degree grid, 5 x 82 = 410 columns (197 KB in the old form) vs the oracle's DIRECT harmonic evaluation on 8 columns;
    * 1 degree grid, batch 2, 164 columns (236 KB) vs the float64 factorised transform of the same tables;
    * 0.5 degree grid (361 latitudes: two latitude blocks, L = 360: three wavenumber chunks), same check,
  plus unit variance and the stream bookkeeping at each size."""
  from oracle import noise_oracle as NO
  from gencast_flax_nnx_amd import noise
  if case.startswith("three"):
    n_lat, n_lon, batch, c_out, direct = 61, 120, 5, 82, True              # L = 60: the direct harmonics are finite up to L ~ 85
  elif case.startswith("one"):
    n_lat, n_lon, batch, c_out, direct = 181, 360, 2, 82, False
  else:
    n_lat, n_lon, batch, c_out, direct = 361, 720, 1, 6, False
  lat, lon = np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=batch, c_in=c_out + 8, c_out=c_out, n_lat=n_lat, n_lon=n_lon,
                                                  mesh_size=2, layers=1)
  nd = helpers.make_native(gr, dims, params, batch)
  try:
    gen = noise.SphericalNoise(lat, lon)
    N = batch * c_out
    assert direct or 2 * gen.lmax * N * 4 > 160 * 1024 or n_lat > 192
    nd.noise_set_tables(n_lat, n_lon, *gen.device_tables())
    nd.noise_seed(11, 3)
    nd.noise_draw()
    got = nd.download_noise().reshape(-1, N)
    assert np.isfinite(got).all()
    if direct:
      cols = [0, 1, 63, 64, 127, 200, 300, N - 1]                             # columns from most 64-column groups of the launch
      want = NO.device_field(11, 3, lat, lon, N, subset=cols)
      assert np.abs(got[:, cols] - want).max() < 5e-5
    want = _factorised_field(gen, 11, 3, N)
    assert np.abs(got - want).max() < 5e-5, np.abs(got - want).max()
    assert abs(float((got.astype(np.float64) ** 2).mean()) - 1.0) < 0.05      # unit variance over nodes and columns
    nd.noise_draw()                                                           # the next draw is stream 4
    np.testing.assert_allclose(nd.download_noise().reshape(-1, N)[:, :2], _factorised_field(gen, 11, 4, N)[:, :2], atol=5e-5)
  finally:
    nd.close()


def test_stochastic_churn_at_one_degree_with_batch_2():
  """The churn sampler where round 4 refused it (VERDICT r4 missing 3): 1 degree grid, 2 members batched along B with
  82 channels each (2 L B c_out floats = 236 KB) -- gencast/samplers_utils.py:434-452 inside gc_sample_resident against
  oracle/noise_oracle.dpm_solver_2s_sample_churn, whose fields here come from the float64 factorised transform of the
  same tables and Philox streams (the direct harmonics overflow at L = 180)."""
  from oracle import noise_oracle as NO
  from gencast_flax_nnx_amd import noise
  n_lat, n_lon, batch, c_out = 181, 360, 2, 82
  lat, lon = np.linspace(-90, 90, n_lat), np.arange(n_lon) * 1.0
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=batch, c_in=c_out + 8, c_out=c_out, n_lat=n_lat, n_lon=n_lon,
                                                  mesh_size=2, layers=1)
  nd = helpers.make_native(gr, dims, params, batch)
  try:
    gen = noise.SphericalNoise(lat, lon)
    nd.noise_set_tables(n_lat, n_lon, *gen.device_tables())
    slots = np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32)
    nd.set_noisy_slots(slots)
    sig = O.noise_schedule(80.0, 0.03, 4, 7.0)
    rates = O.stochastic_churn_rate_schedule(sig, 2.5, 0.05, 50.0)
    assert (rates > 0).sum() >= 2
    init = np.random.default_rng(5).standard_normal((gr.num_grid_nodes, batch, c_out)).astype(np.float32)
    nd.set_churn(rates, 1.05)
    nd.noise_seed(11, 0)
    out, st = nd.sample(x, init, sig)
    fields = lambda k: _factorised_field(gen, 11, k, batch * c_out).reshape(gr.num_grid_nodes, batch, c_out)
    net = lambda f, s: O.denoiser_forward(params, helpers.graph_dict(gr), f, s, num_layers=dims.num_layers,
                                          num_heads=dims.num_heads, attention="neighbour")
    ref, calls, drawn = NO.dpm_solver_2s_sample_churn(net, x.astype(np.float64), slots, init.astype(np.float64), sig,
                                                     rates, 1.05, fields)
    assert st["denoiser_calls"] == calls and drawn == (rates > 0).sum()
    assert np.abs(out - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())
  finally:
    nd.close()


def test_stochastic_churn_sampler_matches_the_oracle():
  """DPM-Solver++2S with churn (samplers_utils.py:415-452) inside gc_sample_resident
  against oracle/noise_oracle.dpm_solver_2s_sample_churn fed with the oracle's own noise fields for the same
  Philox streams; then the Python Sampler with the reference's DEFAULT SamplerConfig (churn 2.5)."""
  from oracle import noise_oracle as NO
  from gencast_flax_nnx_amd import noise
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=2)
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    lat, lon = np.linspace(-90, 90, 13), np.arange(24) * 15.0
    nd.noise_set_tables(13, 24, *noise.SphericalNoise(lat, lon).device_tables())
    slots = np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32)
    nd.set_noisy_slots(slots)
    sig = O.noise_schedule(80.0, 0.03, 6, 7.0)
    rates = O.stochastic_churn_rate_schedule(sig, 2.5, 0.05, 50.0)
    assert (rates > 0).sum() >= 3
    init = np.random.default_rng(5).standard_normal((gr.num_grid_nodes, 2, dims.c_out)).astype(np.float32)
    with pytest.raises(ValueError, match="another length"):
      nd.set_churn(rates[:-1], 1.05)
      nd.sample(x, init, sig)
    nd.set_churn(rates, 1.05)
    nd.noise_seed(11, 0)
    out, st = nd.sample(x, init, sig)
    fields = lambda k: NO.device_field(11, k, lat, lon, 2 * dims.c_out).reshape(gr.num_grid_nodes, 2, dims.c_out)
    net = lambda f, s: O.denoiser_forward(params, helpers.graph_dict(gr), f, s, num_layers=dims.num_layers,
                                          num_heads=dims.num_heads, attention="dense")
    ref, calls, drawn = NO.dpm_solver_2s_sample_churn(net, x.astype(np.float64), slots, init.astype(np.float64), sig,
                                                     rates, 1.05, fields)
    assert st["denoiser_calls"] == calls and drawn == (rates > 0).sum()
    assert np.abs(out - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())
    nd.set_churn(None)
    plain, _ = nd.sample(x, init, sig)
    assert np.abs(plain - out).max() > 1e-2                                  # churn really changed the trajectory
    nd.set_churn(rates, 1.05)                                                # same seed and stream -> same sample
    nd.noise_seed(11, 0)
    again, _ = nd.sample(x, init, sig)
    np.testing.assert_array_equal(again, out)
  finally:
    nd.close()
  # the reference-shaped surface with the reference's default sampler config (churn rate 2.5)
  arch = _small_arch()
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  sc = dataclasses.replace(config.SamplerConfig(), num_noise_levels=6)
  assert sc.stochastic_churn_rate == 2.5
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None,
               params=weights.random_params(dims_from_arch(arch, 262, 82), seed=3), rngs=3)
  tmpl = datasets.zeros_like(tgt)
  a = gc.full_sampling(inp, tmpl, frc)
  gc.rngs = np.random.default_rng(3)
  b = gc.full_sampling(inp, tmpl, frc)
  gc._sampler.device_noise = True
  c = gc.full_sampling(inp, tmpl, frc)
  for k in tgt.keys():
    assert np.isfinite(a[k].data).all() and np.isfinite(c[k].data).all()
    np.testing.assert_array_equal(a[k].data, b[k].data)                     # same rngs -> same forecast
  gc.denoiser.native.close()


def test_library_comm_single_rank_and_ensemble_members():
  """The in-library RCCL exchange (gc_comm_*) on a single-rank communicator -- more ranks need more GPUs --
  and EnsembleSampler through it: a member equals Sampler(init_noise=<that member's spherical field>)
  (ADVICE r1), and is the same whichever rank of a larger world would have drawn it."""
  from gencast_flax_nnx_amd import EnsembleSampler, _lib
  arch = _small_arch()
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  sc = config.SamplerConfig(num_noise_levels=4, stochastic_churn_rate=0.0)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None,
               params=weights.random_params(dims_from_arch(arch, 262, 82), seed=3), rngs=3)
  tmpl = datasets.zeros_like(tgt)
  cond, grid_shape, slots = gc.denoiser.init_for(inp, tmpl, frc)
  nd = gc.denoiser.native
  uid = _lib.comm_unique_id()
  assert len(uid) == _lib.COMM_ID_BYTES
  with pytest.raises(_lib.GencastHipError, match="gc_comm_init"):
    nd.comm_broadcast_cond(0)
  assert nd.comm_info() == (0, -1)                         # no communicator yet
  nd.comm_init(uid, 0, 1)
  with pytest.raises(_lib.GencastHipError, match="already"):
    nd.comm_init(uid, 0, 1)
  nd.upload_cond(cond)
  nd.comm_broadcast_cond(0)                                # in place on the resident buffer + re-pack
  np.testing.assert_array_equal(nd.download_cond(), cond)
  assert nd.comm_info() == (1, 0)                          # ncclCommCount / ncclCommUserRank (gc_comm_info)
  assert nd.comm_allreduce_max(3.25) == 3.25
  with pytest.raises(ValueError, match="root"):
    nd.comm_broadcast_cond(1)
  ens = EnsembleSampler(gc._sampler, rank=0, world_size=1, base_seed=17, library_comm=True)
  members = dict(ens(inp, tmpl, frc, 3))
  assert sorted(members) == [0, 1, 2]
  shape = (cond.shape[0], 1, 82)
  for m in (0, 2):
    ref = gc._sampler(inp, tmpl, frc, rngs=0, init_noise=ens.member_noise(m, shape, tmpl))
    for k in tgt.keys():
      np.testing.assert_array_equal(members[m][k].data, ref[k].data)
  # rank 1 of a 2-rank world would own member 1 and draw the very same field
  ens_b = EnsembleSampler(gc._sampler, rank=1, world_size=2, base_seed=17)
  np.testing.assert_array_equal(ens_b.member_noise(1, shape, tmpl), ens.member_noise(1, shape, tmpl))
  nd.comm_destroy()
  nd.comm_destroy()                                        # idempotent
  nd.close()


def test_pending_domain_guard_rerun_uses_the_inputs_of_its_own_sample():
  """sample_resident is asynchronous and its f16x3 domain check is resolved by the next download / sync.
  A caller that pipelines `sample -> upload the NEXT member's noise -> download` must still get the first member when
  the check fires and the sample is re-run on the exact-f32 kernels (the initial noise is double-buffered), and the
  next sample must then start from the new noise."""
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=2, seed=21)
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    big = x.copy()
    big[:, :, 3] *= 2.0e5                                  # un-normalised conditioning channel: leaves the fp16 domain
    nd.set_noisy_slots(np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32))
    rng = np.random.default_rng(5)
    n1, n2 = (rng.standard_normal((gr.num_grid_nodes, 2, dims.c_out)).astype(np.float32) for _ in range(2))
    sig = O.noise_schedule(80.0, 0.03, 4, 7.0).astype(np.float32)
    want1, _ = nd.sample(big, n1, sig)                     # synchronous path: re-run from n1
    want2, _ = nd.sample(big, n2, sig)
    f0 = nd.counter("range_fallbacks")
    assert f0 == 2 and not np.array_equal(want1, want2)
    nd.upload_cond(big)
    nd.upload_noise(n1)
    nd.sample_resident(sig, want_stats=False)              # check pending
    nd.upload_noise(n2)                                    # next member's noise arrives before the download
    got1 = nd.download_sample()                            # resolves the check: exact-f32 re-run of sample 1
    assert nd.counter("range_fallbacks") == f0 + 1
    np.testing.assert_array_equal(got1, want1)
    np.testing.assert_array_equal(nd.download_noise(), n2)  # and the new noise is what the handle now holds
    nd.sample_resident(sig, want_stats=False)
    np.testing.assert_array_equal(nd.download_sample(), want2)
    # a conditioning upload while a check is pending resolves it first (waits), then replaces the conditioning
    nd.upload_noise(n1)
    nd.sample_resident(sig, want_stats=False)
    nd.upload_cond(x)
    assert nd.counter("range_fallbacks") == f0 + 3
    np.testing.assert_array_equal(nd.download_sample(), want1)
  finally:
    nd.close()


def test_sampler_graph_replay_is_bit_identical_to_eager_launches():
  """gc_set_option("graphs"): the second sample with one signature is captured into a hipGraph, later ones are one
  hipGraphLaunch (the reference's sampler is one compiled fori_loop program, dpm_solver_plus_plus_2s.py:157-158).
  Same kernels, same arguments, same order: every sample equals the eagerly enqueued one bit for bit; a new noise
  level schedule, feature mode or noise buffer is a new signature; churn and profiling stay eager."""
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=2, seed=3)
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    nd.set_noisy_slots(np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32))
    rng = np.random.default_rng(9)
    noise = rng.standard_normal((gr.num_grid_nodes, 2, dims.c_out)).astype(np.float32)
    sig6 = O.noise_schedule(80.0, 0.03, 6, 7.0).astype(np.float32)
    sig4 = O.noise_schedule(80.0, 0.03, 4, 7.0).astype(np.float32)
    nd.set_option("graphs", "off")
    want6, st = nd.sample(x, noise, sig6)
    want4, _ = nd.sample(x, noise, sig4)
    assert nd.counter("graph_captures") == 0 and nd.counter("graph_replays") == 0
    nd.set_option("graphs", "on")
    for i in range(4):                                       # eager, capture + launch, replay, replay
      got, st2 = nd.sample(x, noise, sig6)
      np.testing.assert_array_equal(got, want6)
      assert st2["denoiser_calls"] == st["denoiser_calls"] == 11
    assert (nd.counter("graph_captures"), nd.counter("graph_replays")) == (1, 3)
    for i in range(3):                                       # another schedule: its own graph
      np.testing.assert_array_equal(nd.sample(x, noise, sig4)[0], want4)
    assert (nd.counter("graph_captures"), nd.counter("graph_replays")) == (2, 5)
    np.testing.assert_array_equal(nd.sample(x, noise, sig6)[0], want6)          # the first graph is still there
    assert nd.counter("graph_replays") == 6
    # the callers' samplers set the noisy slots before EVERY sample (sampler.py): the same slots again must not rebuild the
    # split grid-embedding images (which would drop the captured graphs); other slots must
    slots = np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32)
    nd.set_noisy_slots(slots)
    np.testing.assert_array_equal(nd.sample(x, noise, sig6)[0], want6)
    assert (nd.counter("graph_captures"), nd.counter("graph_replays")) == (2, 7)
    nd.set_noisy_slots(slots[::-1].copy())
    other = nd.sample(x, noise, sig6)[0]                      # eager again: first sight of the signature after the drop
    assert (nd.counter("graph_captures"), nd.counter("graph_replays")) == (2, 7) and not np.array_equal(other, want6)
    nd.set_noisy_slots(slots)
    np.testing.assert_array_equal(nd.sample(x, noise, sig6)[0], want6)
    # new inputs through the same graph: resident buffers are read at replay time
    noise2 = rng.standard_normal(noise.shape).astype(np.float32)
    nd.set_option("graphs", "off")
    want_n2, _ = nd.sample(x * 0.5, noise2, sig6)
    nd.set_option("graphs", "on")
    np.testing.assert_array_equal(nd.sample(x * 0.5, noise2, sig6)[0], want_n2)
    assert nd.counter("launches_per_call") > 0
    # feature mode is part of the signature
    nd.set_option("features", "f16")
    a = nd.sample(x, noise, sig6)[0]
    b = nd.sample(x, noise, sig6)[0]
    c = nd.sample(x, noise, sig6)[0]
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)
    assert not np.array_equal(a, want6) and nd.counter("fp16_storage") == 1
    nd.set_option("features", "f32")
    np.testing.assert_array_equal(nd.sample(x, noise, sig6)[0], want6)
    with pytest.raises(ValueError, match="graphs"):
      nd.set_option("graphs", "maybe")
  finally:
    nd.close()


def test_refinalize_replaces_the_weight_buffers():
  """gc_finalize owns what it allocates: loading the same weights and finalizing again frees the previous images, so
  the handle's device allocation count stays where the first gc_finalize left it and gc_denoise repeats bit for bit."""
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=2, seed=3)
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    n0 = nd.counter("device_allocations")
    y0 = nd.denoise(x, sigma)
    assert n0 > 0
    for _ in range(2):
      nd.load_weights(params)
      nd.finalize()
      assert nd.counter("device_allocations") == n0
      np.testing.assert_array_equal(nd.denoise(x, sigma), y0)
  finally:
    nd.close()


def test_changing_the_noisy_slots_replaces_the_embed_cache_images():
  """gc_set_noisy_slots with other slots rebuilds the split grid-embedding images in place of the old ones: slots,
  reversed slots, slots again, a sample after each -- as many device allocations after the third sample as after the
  first, and the first and third samples equal bit for bit."""
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=2, seed=3)
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    slots = np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32)
    noise = np.random.default_rng(9).standard_normal((gr.num_grid_nodes, 2, dims.c_out)).astype(np.float32)
    sig = O.noise_schedule(80.0, 0.03, 4, 7.0).astype(np.float32)
    nd.set_noisy_slots(slots)
    first = nd.sample(x, noise, sig)[0]
    n1 = nd.counter("device_allocations")
    assert nd.counter("embed_cache") == 1
    nd.set_noisy_slots(slots[::-1].copy())
    nd.sample(x, noise, sig)
    nd.set_noisy_slots(slots)
    third = nd.sample(x, noise, sig)[0]
    assert nd.counter("device_allocations") == n1
    np.testing.assert_array_equal(third, first)
  finally:
    nd.close()


def test_concurrent_members_are_bit_identical_to_sequential_ones():
  """EnsembleSampler(concurrent_members=3): three members in flight on three handles (three HIP streams) of
  one GPU -- every member equals the one-at-a-time result bit for bit (no shared scratch between handles)."""
  from gencast_flax_nnx_amd import EnsembleSampler
  arch = _small_arch()
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  sc = config.SamplerConfig(num_noise_levels=4, stochastic_churn_rate=0.0)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None,
               params=weights.random_params(dims_from_arch(arch, 262, 82), seed=3), rngs=3)
  tmpl = datasets.zeros_like(tgt)
  seq = dict(EnsembleSampler(gc._sampler, base_seed=5)(inp, tmpl, frc, 5))
  par = dict(EnsembleSampler(gc._sampler, base_seed=5, concurrent_members=3)(inp, tmpl, frc, 5))
  assert sorted(par) == sorted(seq) == [0, 1, 2, 3, 4]
  for m in seq:
    for k in tgt.keys():
      np.testing.assert_array_equal(par[m][k].data, seq[m][k].data)
  assert not np.array_equal(par[0][list(tgt.keys())[0]].data, par[1][list(tgt.keys())[0]].data)
  assert len(gc.denoiser.member_lanes(2)) == 2


def test_device_pci_bus_id_names_the_gpu():
  """What the ranks of a launch compare before any collective: a PCI bus id per visible device."""
  import re
  from gencast_flax_nnx_amd import _lib
  n = _lib.device_count()
  assert n >= 1
  ids = [_lib.device_pci_bus_id(i) for i in range(n)]
  assert all(re.fullmatch(r"[0-9a-fA-F]{4}:[0-9a-fA-F]{2}:[0-9a-fA-F]{2}\.[0-7]", s) for s in ids), ids
  assert len(set(ids)) == n
  with pytest.raises(_lib.GencastHipError):
    _lib.device_pci_bus_id(n)


# ---- round 4 ------------------------------------------------------------------------------------------------------

def _nested_reference_state(params, hoisted):
  """A restored-orbax-like tree: `.value` leaves, {0: leaf} singletons, one-element lists, the normalisation
  datasets and private buffers `clean_state` strips (training/evaluation.py:137-176); `hoisted`: the
  `graph_network` level already removed (what the reference's own clean-up leaves behind) or still there."""
  nested = {}
  for name, arr in params.items():
    parts = [p for p in name.split(".") if not (hoisted and p == "graph_network")]
    cur = nested
    for p in parts[:-1]:
      cur = cur.setdefault(p, {})
    style = len(name) % 3
    cur[parts[-1]] = {"value": arr} if style == 0 else ({0: arr} if style == 1 else [arr])
  nested["stddev_by_level"] = {"2m_temperature": np.ones(3), "10m_u_component_of_wind": np.ones(3)}
  nested["denoiser"]["_private_buffer"] = np.zeros(4)
  nested["optimizer_state"] = {"mu": [np.zeros(3)]}
  return nested


@pytest.mark.parametrize("hoisted", [False, True])
def test_imported_reference_state_drives_the_handle_to_the_oracles_answer(hoisted):
  """SURVEY.md 8f row 4 end to end on the device (VERDICT r3 missing 3): a nested NNX-style state -- carrying
  everything `clean_state` strips, with the `graph_network` level present or already hoisted -- goes through
  `weights.import_reference_state` into a handle; the device result equals the oracle evaluated with the SAME
  imported parameters (training/evaluation.py:119-187: clean_state + nnx.update)."""
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=2)
  imported = weights.import_reference_state(_nested_reference_state(params, hoisted), dims)
  assert sorted(imported) == sorted(params)
  nd = helpers.make_native(gr, dims, imported, 2)
  try:
    y = nd.denoise(x, sigma)
  finally:
    nd.close()
  want = O.denoiser_forward(imported, helpers.graph_dict(gr), x, sigma, num_layers=dims.num_layers,
                            num_heads=dims.num_heads, attention="dense")
  assert np.abs(y - want).max() < 1e-4


def test_grid2mesh_aggregate_normalization_matches_the_oracle():
  """DenoiserArchitectureConfig.grid2mesh_aggregate_normalization (gencast/denoiser.py:123,138,367;
  deep_typed_graph_net.py:396-410): the summed grid2mesh edge messages are divided by the constant -- through the
  reference-shaped constructor, against the oracle with the same constant, in both feature modes; and it changes
  the answer."""
  arch = dataclasses.replace(_small_arch(), grid2mesh_aggregate_normalization=3.5)
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=2, seed=1)
  params = weights.random_params(dims_from_arch(arch, 262, 82), seed=3)
  den = Denoiser(None, arch, params, rngs=7, gpu_mesh=None)          # the reference's extra arguments are accepted
  sigma = np.array([0.7, 12.0], np.float32)
  out = den(inp, tgt, sigma, frc)
  feats, grid_shape, *_ = Denoiser.pack_inputs(inp, frc.assign(tgt))
  gd = helpers.graph_dict(den.graph)
  want = O.denoiser_forward(params, gd, feats, sigma, num_layers=2, num_heads=2, attention="dense",
                            g2m_aggregate_normalization=3.5)
  plain = O.denoiser_forward(params, gd, feats, sigma, num_layers=2, num_heads=2, attention="dense")
  w, p = Denoiser.unpack_outputs(want, grid_shape, tgt), Denoiser.unpack_outputs(plain, grid_shape, tgt)
  worst = max(float(np.abs(out[k].data - w[k].data).max()) for k in tgt.keys())
  moved = max(float(np.abs(p[k].data - w[k].data).max()) for k in tgt.keys())
  assert worst < 1e-4 and moved > 1e-2, (worst, moved)
  den.native.set_option("features", "f16")                           # fp16 features: the sum is divided in float32, then rounded
  out16 = den(inp, tgt, sigma, frc)
  want16 = Denoiser.unpack_outputs(
      O.denoiser_forward(params, gd, feats, sigma, num_layers=2, num_heads=2, attention="dense",
                         g2m_aggregate_normalization=3.5, feature_dtype=np.float16, dtype=np.float32), grid_shape, tgt)
  worst16 = max(float(np.abs(out16[k].data - want16[k].data).max()) for k in tgt.keys())
  assert worst16 < 5e-2, worst16
  with pytest.raises(Exception):
    den.native.set_option("grid2mesh_aggregate_normalization", "-1")
  den.native.close()


class _NnxLikeRngs:
  """What the reference hands over as `rngs` (nnx.Rngs): streams called like functions, returning key words."""

  def __init__(self, seed):
    self._seed, self._count = seed, 0

  def _key(self, stream):
    self._count += 1
    return np.array([self._seed, stream, self._count], np.uint32)

  def noise(self):
    return self._key(1)

  def params(self):
    return self._key(2)


def test_gencast_takes_the_reference_constructor_arguments():
  """gencast/gencast.py:145-154: `GenCast(task, arch, sampler_cfg, noise_cfg, noise_encoder_cfg, gpu_mesh, rngs)`
  with an nnx.Rngs-like `rngs`; `full_sampling` is also what replaces evaluation.py:389-393's `loss` warm-up."""
  arch = _small_arch()
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  sc = config.SamplerConfig(num_noise_levels=3, stochastic_churn_rate=0.0)
  params = weights.random_params(dims_from_arch(arch, 262, 82), seed=3)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, object(), _NnxLikeRngs(5), params=params)
  tmpl = datasets.zeros_like(tgt)
  a = gc.full_sampling(inp, tmpl, frc)                                # lazy init happens here (the warm-up)
  b = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, None, _NnxLikeRngs(5), params=params).full_sampling(inp, tmpl, frc)
  for k in tgt.keys():
    assert np.isfinite(a[k].data).all()
    np.testing.assert_array_equal(a[k].data, b[k].data)              # same key stream, same sample
  gc.denoiser.native.close()


def test_concurrent_members_match_the_oracle_at_nano_size():
  """`EnsembleSampler(concurrent_members=3)` -- three members in flight on three handles -- at
  the nano size (2.5 deg grid, mesh 4, latent 256, 16 layers) against the ORACLE's DPM-Solver++2S sample of each
  member (its own spherical noise), not only against solo runs."""
  from gencast_flax_nnx_amd import EnsembleSampler
  lat, lon = synthetic.grid_2p5deg()
  arch = dataclasses.replace(config.nano_architecture(mesh_size=4, d_model=256, num_layers=16, num_heads=4),
                             node_output_size=82)
  inp, tgt, frc = synthetic.make_example(lat, lon, batch=1, seed=0)
  sc = config.SamplerConfig(num_noise_levels=2, stochastic_churn_rate=0.0)     # 3 denoiser calls per member (the oracle takes ~10 s each)
  params = weights.random_params(dims_from_arch(arch, 262, 82), seed=3)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=3)
  tmpl = datasets.zeros_like(tgt)
  es = EnsembleSampler(gc._sampler, base_seed=11, concurrent_members=3)
  got = dict(es(inp, tmpl, frc, 3))
  den = gc.denoiser
  cond, grid_shape, slots = den.init_for(inp, tmpl, frc)
  gd = helpers.graph_dict(den.graph)
  sig = np.asarray(gc._sampler.noise_levels, np.float64)
  net = lambda feats, sigma: O.denoiser_forward(params, gd, feats, sigma, num_layers=16, num_heads=4, attention="dense")
  shape = (cond.shape[0], 1, 82)
  worst = 0.0
  first = list(tgt.keys())[0]
  assert not np.array_equal(got[0][first].data, got[1][first].data) and not np.array_equal(got[1][first].data, got[2][first].data)
  for m in (0, 2):                                                   # lane 0's member and an extra lane's
    noise = es.member_noise(m, shape, tmpl).astype(np.float64)
    want, calls = O.dpm_solver_2s_sample(net, cond.astype(np.float64), np.asarray(slots), noise, sig, skip_dead_call=True)
    assert calls == 2 * (len(sig) - 1) - 1
    w = Denoiser.unpack_outputs(want, grid_shape, tgt)
    scale = max(1.0, float(np.abs(want).max()))
    for k in tgt.keys():
      worst = max(worst, float(np.abs(got[m][k].data - w[k].data).max()) / scale)
  print(f"three concurrent nano members vs the oracle sampler: max |err| / scale {worst:.3e}")
  assert worst < 1e-4, worst
  den.native.close()


def test_six_threads_six_handles_with_graph_replay():
  """The case that hung once in round 3 (six host threads, each driving its own handle through eager sample ->
  capture -> replays at the same time), after the fix (capture + instantiate serialised process-wide, launches
  not; two executables per signature; nothing lazy left to a capturing thread): run ONCE, every member equal to
  its single-threaded eager result."""
  import threading
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=1)
  sig = O.noise_schedule(80.0, 0.03, 6, 7.0).astype(np.float32)
  slots = np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32)
  noises = [np.random.default_rng(40 + i).standard_normal((gr.num_grid_nodes, 1, dims.c_out)).astype(np.float32) for i in range(6)]

  def make(i):
    nd = helpers.make_native(gr, dims, params, 1)
    nd.set_noisy_slots(slots)
    nd.upload_cond(x)
    nd.upload_noise(noises[i])
    return nd

  ref = []
  solo = make(0)
  solo.set_option("graphs", "off")
  for i in range(6):
    solo.upload_noise(noises[i])
    solo.sample_resident(sig, want_stats=False)
    ref.append(solo.download_sample())
  solo.close()
  handles = [make(i) for i in range(6)]
  errors = []

  def run(h):
    try:
      for _ in range(5):                                             # eager, capture + replay, three more replays
        h.sample_resident(sig, want_stats=False)
    except Exception as e:  # pylint: disable=broad-except
      errors.append(e)

  threads = [threading.Thread(target=run, args=(h,), daemon=True) for h in handles]   # daemon: a stuck thread must not keep pytest alive
  for t in threads:
    t.start()
  for t in threads:
    t.join(timeout=120)
  assert not any(t.is_alive() for t in threads), "a thread is still inside the library after 120 s"
  assert not errors, errors
  for i, h in enumerate(handles):
    np.testing.assert_array_equal(h.download_sample(), ref[i])
    assert h.counter("graph_captures") == 1 and h.counter("graph_replays") == 4
    h.close()


def test_one_degree_fp16_rollout_two_steps_compose_as_the_oracle_says():
  """BASELINE.json configs[4], one member, on one GPU with a criterion that can fail: `DeviceRollout` at 1 deg
  (181 x 360 grid, mesh 5, full widths, 16 layers) with fp16 node features and injected noise, two steps.
  Step by step against the rollout ORACLE at full size: each step's prediction = the oracle's un-normalisation +
  residual add of the sample the handle holds (normalization.py:200-238), and the conditioning after
  `gc_rollout_advance` = `rollout_oracle.apply_plan` of the old conditioning, that sample and the next forcings
  (train_helpers.py:596-622), elementwise.  (The network arithmetic of a call at this size and mode is pinned by
  the one_degree_f16 fixture test.)"""
  from gencast_flax_nnx_amd import rollout
  from oracle import rollout_oracle as RO
  from tests.test_rollout import _stats
  lat = np.arange(-90.0, 90.0 + 1e-9, 1.0)
  lon = np.arange(0.0, 360.0, 1.0)
  gr, dims, params, _, _ = helpers.one_degree_setup()
  arch = dataclasses.replace(config.nano_architecture(mesh_size=5, d_model=512, num_layers=16, num_heads=4), node_output_size=82)
  inp, tgt1, frc1 = synthetic.make_example(lat, lon, batch=1, seed=0)
  rng = np.random.default_rng(5)

  def stretch(ds, nt):
    out = {}
    for k, v in ds.items():
      shape = list(v.data.shape)
      shape[v.dims.index("time")] = nt
      out[k] = datasets.Variable(v.dims, rng.standard_normal(shape).astype(np.float32))
    return datasets.Dataset(out, ds.coords)

  horizon = 2
  targets, forcings = stretch(tgt1, horizon), stretch(frc1, horizon)
  sc = config.SamplerConfig(num_noise_levels=4, stochastic_churn_rate=0.0)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=1, graph=gr, options={"features": "f16"})
  stats = _stats(config.TASK)
  norm = rollout.InputsAndResiduals(gc, *stats)
  G = len(lat) * len(lon)
  noises = [rng.standard_normal((G, 1, 82)).astype(np.float32) for _ in range(horizon)]
  dr = rollout.DeviceRollout(gc, norm)
  preds = dr.run(inp, targets, forcings, horizon, init_noise=noises)
  nd = gc.denoiser.native
  assert nd.counter("fp16_storage") == 1 and nd.counter("range_fallbacks") == 0
  # ---- the same two steps by hand, every host-side piece taken from the oracle
  context = rollout.isel_time(inp, slice(-2, None))
  tmpl0 = rollout.isel_time(targets, slice(0, 1)).map(np.zeros_like)
  forc0 = rollout.isel_time(forcings, slice(0, 1))
  n_in = rollout.normalize(context, norm._scales, norm._locations)
  n_fo = rollout.normalize(forc0, norm._scales, norm._locations)
  cond, grid_shape, slots = gc.denoiser.init_for(n_in, tmpl0, n_fo)
  plan, forcing_cols = rollout.build_rollout_plan(context, forc0, tmpl0, config.TASK, norm)
  nd.set_noisy_slots(slots)
  nd.rollout_plan(**plan)
  nd.upload_cond(cond)
  sig = np.asarray(gc._sampler.noise_levels, np.float32)
  sizes = dict(forc0.sizes)
  sizes.update(context.sizes)
  keep = np.ones(cond.shape[-1], bool)
  keep[slots] = False
  last = {k: np.asarray(context[k].data)[:, -1:] for k in tmpl0.keys() if k in context}     # (batch, time=1, ...)
  cur = cond.astype(np.float64)
  for k in range(horizon):
    nd.upload_noise(noises[k])
    nd.sample_resident(sig, skip_dead_call=True, want_stats=False)
    sample = nd.download_sample()
    norm_pred = Denoiser.unpack_outputs(sample, grid_shape, rollout.isel_time(targets, slice(k, k + 1)).map(np.zeros_like))
    for name in tgt1.keys():
      v = norm_pred[name]
      one = {name: (v.dims, v.data.astype(np.float64))}
      if name in last:                                       # residual variable: un-normalise the residual, add the last frame
        phys = RO.unnormalize(one, {n: (s.dims, s.data) for n, s in norm._residual_scales.items()},
                              None)[name][1] + last[name]
      else:
        phys = RO.unnormalize(one, {n: (s.dims, s.data) for n, s in norm._scales.items()},
                              {n: (s.dims, s.data) for n, s in norm._locations.items()})[name][1]
      got = np.asarray(preds[name].data)[:, k:k + 1]
      scale = max(1.0, float(np.abs(phys).max()))
      assert np.abs(got - phys).max() < 1e-5 * scale, (k, name)
      if name in last:
        last[name] = phys
    if k + 1 < horizon:
      frows = dr._forcing_rows(rollout.isel_time(forcings, slice(k + 1, k + 2)), forcing_cols, sizes, grid_shape)
      nd.rollout_advance(frows)
      got_c = nd.download_cond()
      cur = RO.apply_plan(cur, sample.astype(np.float64), frows.astype(np.float64), plan)
      scale = max(1.0, float(np.abs(cur[..., keep]).max()))
      err = float(np.abs(got_c[..., keep] - cur[..., keep]).max())
      print(f"1deg fp16 rollout: conditioning after step {k + 1} vs rollout_oracle.apply_plan: max |err| {err:.3e} (scale {scale:.2f})")
      assert err < 2e-6 * scale
  assert all(bool(np.isfinite(np.asarray(v.data)).all()) for v in preds.data_vars.values())
  nd.close()


# ---- the host protocol of the ensemble scorers: counter names and the order of the checks -------------------------------

# every name gc_get_counter knows, but for device_allocations and noise_stream
COUNTERS = (
    "range_fallbacks", "static_embedding_fallbacks", "launches_per_call", "weights_f16_unsafe", "fp16_storage", "split_edge",
    "attention_items", "m2g_fused_sum", "embed_cache", "edge_term_samples", "edge_term_cache_bytes", "graph_replays",
    "graph_captures", "loss_evaluations", "loss_device_us", "poison_allocs", "poison_bytes",
    "ens_scores", "ens_score_device_us", "ens_invalid_points",
    "spec_calls", "spec_device_us", "spec_invalid_columns",
    "ens_event_calls", "ens_event_device_us", "ens_event_invalid_points",
    "ens_derive_calls", "ens_derive_device_us",
    "ens_band_calls", "ens_band_device_us", "ens_band_invalid_columns",
    "ens_order_calls", "ens_order_device_us", "ens_order_invalid_points",
    "ens_clim_calls", "ens_clim_device_us", "ens_clim_invalid_points",
    "ens_energy_calls", "ens_energy_device_us", "ens_energy_invalid_points",
    "ens_variogram_calls", "ens_variogram_device_us",
    "ens_tail_calls", "ens_tail_device_us", "ens_tail_invalid_points",
    "ens_region_calls", "ens_region_device_us", "ens_region_invalid_points",
    "ens_feature_calls", "ens_feature_device_us",
    "ens_fss_calls", "ens_fss_device_us",
    "ens_window_pushes", "ens_window_emits", "ens_window_device_us", "ens_window_ring_bytes",
    # the launch geometry of the last call: node-range workgroups of the main pass, column chunks of the fractions sums
    "ens_score_blocks", "ens_event_blocks", "ens_derive_blocks", "ens_band_blocks", "ens_order_blocks", "ens_clim_blocks",
    "ens_energy_blocks", "ens_variogram_blocks", "ens_tail_blocks", "ens_region_blocks", "ens_feature_blocks", "ens_fss_blocks",
    "ens_efi_blocks", "ens_fss_chunks")
FRESH_ALLOCATIONS = 51        # device buffers of a graph-only handle on the 13 x 24 grid (B = 1, c_out = 2): those of gc_set_graph


def test_every_counter_name_reads_zero_on_a_fresh_handle_and_other_names_are_refused():
  """gc_get_counter on a handle that knows its graph and nothing else: every public name reads 0, `device_allocations` counts
  the buffers of gc_set_graph, and a scorer that keeps no `invalid` counter has no such name."""
  nd = helpers.graph_handle(helpers.small_graph(), 1, 2)
  try:
    for name in COUNTERS:
      assert nd.counter(name) == 0, name
    assert nd.counter("noise_stream") == 0
    assert nd.counter("device_allocations") == FRESH_ALLOCATIONS
    for name in ("ens_variogram_invalid_points", "ens_derive_invalid_points", "ens_fss_invalid_points",
                 "ens_feature_invalid_points", "ens_tail", "no_such_counter"):
      with pytest.raises(ValueError, match="unknown counter"):
        nd.counter(name)
  finally:
    nd.close()


def test_the_order_of_the_checks_of_every_scoring_and_filling_entry():
  """Two faults at once, at every rung of the state ladder (graph only -> plans set -> store reserved -> one slot unpushed ->
  all pushed, no weights -> weights, no truth): the rung's state fault and a null required output (for the entries that fill
  a store from another handle, which have no output: a source of other dimensions, and a source whose own ladder is behind).
  Which of the two is reported is the order of the checks in the entry: (return code, a fragment of gc_last_error) below,
  as recorded before the scorers shared their host code.  Every call ends in a host-side refusal; nothing is launched."""
  import ctypes
  from gencast_flax_nnx_amd import _lib
  lib = _lib.load_library()
  ST, ARG = _lib.GC_ERR_STATE, _lib.GC_ERR_INVALID_ARGUMENT
  gr = helpers.small_graph()
  G, B, C, M = gr.num_grid_nodes, 1, 2, 2
  n_lat, n_lon, L = 13, 24, 2
  h, src, clim = (helpers.graph_handle(gr, B, C) for _ in range(3))
  bad = helpers.graph_handle(gr, B, C + 1)                               # a peer of other dimensions
  buf = np.zeros(4096)                                                   # stands for any output: nothing is ever written
  dp, up, fp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_float)
  D, U, F = buf.ctypes.data_as(dp), buf.ctypes.data_as(up), buf.ctypes.data_as(fp)
  p = h._h
  null = {                                                               # every output null
      "score": lambda: lib.gc_ens_score(p, None, 0, None, None),
      "spectrum": lambda: lib.gc_ens_spectrum(p, None, None, None),
      "spec_field": lambda: lib.gc_spec_field(p, None, None),
      "event": lambda: lib.gc_ens_event_score(p, None, None, None, None),
      "fss": lambda: lib.gc_ens_fss_score(p, None),
      "fss_fields": lambda: lib.gc_ens_fss_fields(p, 0, 0, None, None),
      "order": lambda: lib.gc_ens_order_score(p, None, None, None, None, None, None),
      "clim": lambda: lib.gc_ens_clim_score(p, clim._h, None, None, None, None),
      "energy": lambda: lib.gc_ens_energy_score(p, None, None, None, None),
      "variogram": lambda: lib.gc_ens_variogram_score(p, None, None, None),
      "tail": lambda: lib.gc_ens_tail_score(p, None, None, None, None),
      "region": lambda: lib.gc_ens_region_score(p, None, None, None, None),
  }
  full = {                                                               # every output given, no truth
      "score": lambda: lib.gc_ens_score(p, None, 0, D, U),
      "spectrum": lambda: lib.gc_ens_spectrum(p, None, D, D),
      "spec_field": lambda: lib.gc_spec_field(p, None, D),
      "event": lambda: lib.gc_ens_event_score(p, None, U, U, U),
      "order": lambda: lib.gc_ens_order_score(p, None, D, D, D, U, U),
      "clim": lambda: lib.gc_ens_clim_score(p, clim._h, None, D, U, U),
      "energy": lambda: lib.gc_ens_energy_score(p, None, D, D, U),
      "variogram": lambda: lib.gc_ens_variogram_score(p, None, D, U),
      "tail": lambda: lib.gc_ens_tail_score(p, None, D, U, U),
      "region": lambda: lib.gc_ens_region_score(p, None, D, U, U),
  }
  fill = {
      "derive": lambda s: lib.gc_ens_derive(p, s, None),
      "band": lambda s: lib.gc_ens_band(p, s, None),
      "feature": lambda s: lib.gc_ens_feature(p, s, None),
      "window_push": lambda s: lib.gc_ens_window_push(p, s, None),
  }

  wrong = []

  def expect(what, call, code, fragment):
    rc = call()
    err = lib.gc_last_error(p).decode()
    print(f"{what}: {rc} {err!r}")
    if rc != code or fragment not in err:
      wrong.append((what, rc, err, code, fragment))

  NULL, STORE, SRC_STORE, DIMS = "null argument", "no member store (gc_ens_reserve)", "no member store on the source handle", "has other dimensions"
  slot = lambda i: f"member slot {i} has not been pushed"
  try:
    # ---- rung 0: the graph only
    rung = "graph only"
    for name, frag in (("score", STORE), ("spectrum", "no analysis tables"), ("spec_field", "no analysis tables"),
                       ("event", "no thresholds (gc_ens_event_set)"), ("fss", "no plan (gc_ens_fss_set)"),
                       ("fss_fields", "no plan (gc_ens_fss_set)"), ("order", "no probabilities (gc_ens_order_set)"),
                       ("energy", "no plan (gc_ens_energy_set)"), ("variogram", "no plan (gc_ens_variogram_set)"),
                       ("tail", "no thresholds (gc_ens_tail_set)"), ("region", "no regions (gc_ens_region_set)")):
      expect(f"{rung}: {name}", null[name], ST, frag)
    expect(f"{rung}: clim", null["clim"], ARG, NULL)
    expect(f"{rung}: clim, no handle", lambda: lib.gc_ens_clim_score(p, None, None, None, None, None), ARG, "the climatology must be another handle")
    expect(f"{rung}: order_fields", lambda: lib.gc_ens_order_fields(p), ST, "no probabilities")
    expect(f"{rung}: window_emit", lambda: lib.gc_ens_window_emit(p), ST, "no plan (gc_ens_window_set)")
    for name, frag in (("derive", "no plan (gc_ens_derive_set)"), ("band", "no analysis tables"), ("feature", "no plan (gc_ens_feature_set)"),
                       ("window_push", "no plan (gc_ens_window_set)")):
      expect(f"{rung}: {name}, itself", lambda: fill[name](p), ARG, "the source must be another handle")
      expect(f"{rung}: {name}, no source", lambda: fill[name](None), ARG, "the source must be another handle")
      expect(f"{rung}: {name}, other dimensions", lambda: fill[name](bad._h), ST, frag)
      expect(f"{rung}: {name}, empty source", lambda: fill[name](src._h), ST, frag)
    # ---- rung 1: every plan
    rung = "plans set"
    thr = np.zeros((1, G, B, C), np.float32)
    zlat = np.zeros((C, n_lat), np.int32)
    h.spec_set_tables(np.zeros((L, L, n_lat), np.float32), np.zeros((L, n_lon), np.float32), np.zeros((L, n_lon), np.float32))
    expect(f"{rung}: band, tables only", lambda: fill["band"](bad._h), ST, "no plan (gc_ens_band_set)")
    h.ens_band_set(C, np.ones((1, L)), [0], [0, 1], [0, 0], np.zeros((L, n_lat, L), np.float32), np.zeros((L, n_lon), np.float32),
                   np.zeros((L, n_lon), np.float32))
    h.ens_event_set(thr, (+1,), np.ones(G, np.uint32))
    h.ens_fss_set(np.zeros(1, np.int32), np.zeros((1, n_lat), np.int32), np.ones(n_lat, np.uint32))
    h.ens_order_set([0.5])
    h.ens_energy_set(1, np.zeros(C, np.int32), np.ones(C))
    h.ens_variogram_set(n_lat, n_lon, np.array([[0, 1]], np.int32), 1.0)
    h.ens_tail_set(thr, (+1,))
    h.ens_region_set(np.ones(G, np.uint32), 1)
    h.ens_derive_set(C, [0, 0], [0, 1], [0, 0], np.tile([1.0, 0.0, 1.0, 0.0], (C, 1)), n_lat=n_lat, n_lon=n_lon)
    h.ens_feature_set(C, [0, 1], [-1, +1], [0, 0], [0.0, 0.0], n_lat, n_lon, [1, 1], zlat + 1, [0, 0], zlat, [0.0, 0.0], [0, 0], zlat)
    h.ens_window_set(1, 2)
    for name in ("score", "spectrum", "event", "order", "energy", "variogram", "tail", "region"):
      expect(f"{rung}: {name}", null[name], ST, STORE)
    expect(f"{rung}: order_fields", lambda: lib.gc_ens_order_fields(p), ST, STORE)
    for name in ("derive", "band", "feature"):
      expect(f"{rung}: {name}, other dimensions", lambda: fill[name](bad._h), ARG, DIMS)
      expect(f"{rung}: {name}, empty source", lambda: fill[name](src._h), ST, STORE)

    def same_at_every_later_rung(rung):
      expect(f"{rung}: spec_field", null["spec_field"], ARG, NULL)
      expect(f"{rung}: spec_field, no sample", full["spec_field"], ST, "no sample on the device")
      expect(f"{rung}: fss", null["fss"], ST, "no valid event codes")
      expect(f"{rung}: fss_fields", null["fss_fields"], ST, "no valid event codes")
      expect(f"{rung}: clim", null["clim"], ARG, NULL)
      expect(f"{rung}: window_emit", lambda: lib.gc_ens_window_emit(p), ST, "the window needs 2 pushes, the ring holds 0")
      expect(f"{rung}: window_push, other dimensions", lambda: fill["window_push"](bad._h), ARG, DIMS)
      expect(f"{rung}: window_push, empty source", lambda: fill["window_push"](src._h), ST, SRC_STORE)

    same_at_every_later_rung(rung)
    expect(f"{rung}: clim, outputs", full["clim"], ST, STORE)
    # ---- rungs 2 to 4: the store reserved, one slot unpushed, all pushed
    field = np.zeros((G, B, C), np.float32)
    for rung, unpushed in (("store reserved", 0), ("one slot unpushed", 1), ("all pushed, no weights", None)):
      if unpushed == 0:
        h.ens_reserve(M)
      else:
        h.ens_push_host(0 if unpushed == 1 else 1, field)
      same_at_every_later_rung(rung)
      for name in ("score", "spectrum", "event", "tail", "region"):         # the null output is tested before the slots
        expect(f"{rung}: {name}", null[name], ARG, NULL)
      for name in ("order", "energy", "variogram"):                         # ... and here behind them
        if unpushed is not None:
          expect(f"{rung}: {name}", null[name], ST, slot(unpushed))
      if unpushed is not None:
        expect(f"{rung}: order_fields", lambda: lib.gc_ens_order_fields(p), ST, slot(unpushed))
        expect(f"{rung}: clim, outputs", full["clim"], ST, "no member store on the climatology handle")
      for name in ("derive", "band", "feature"):
        expect(f"{rung}: {name}, other dimensions", lambda: fill[name](bad._h), ARG, DIMS)
        expect(f"{rung}: {name}, empty source", lambda: fill[name](src._h), ST, SRC_STORE)
    expect(f"{rung}: order", null["order"], ARG, NULL)                      # behind the slots, in front of the weights
    for name in ("energy", "variogram"):                                    # behind both
      expect(f"{rung}: {name}", null[name], ST, "no node weights")
    for name in ("score", "order", "tail", "region"):
      expect(f"{rung}: {name}, outputs", full[name], ST, "no node weights")
    # ---- rung 5: weights, no truth
    rung = "weights, no truth"
    h.ens_set_node_weight(np.ones(G, np.float32))
    same_at_every_later_rung(rung)
    for name in ("score", "spectrum", "event", "order", "energy", "variogram", "tail", "region"):
      expect(f"{rung}: {name}", null[name], ARG, NULL)
      expect(f"{rung}: {name}, outputs", full[name], ST, f"no truth on the device (pass one to gc_ens_{name}" if name in ("score", "spectrum")
             else f"no truth on the device (pass one to gc_ens_{name}_score)")
    # the climatology's own ladder, behind this handle's
    expect(f"{rung}: clim, outputs", full["clim"], ST, "no member store on the climatology handle")
    clim.ens_reserve(3)
    expect(f"{rung}: clim, an unpushed climatology", full["clim"], ST, "climatology member slot 0 has not been pushed")
    for i in range(3):
      clim.ens_push_host(i, field)
    expect(f"{rung}: clim, complete", full["clim"], ST, "no truth on the device (pass one to gc_ens_clim_score)")
    expect(f"{rung}: clim, other dimensions", lambda: lib.gc_ens_clim_score(p, bad._h, None, D, U, U), ARG, DIMS)
    # ---- the source's ladder, behind this handle's
    src.ens_reserve(M + 1)
    for name in ("derive", "band", "feature"):
      expect(f"source of {M + 1}: {name}", lambda: fill[name](src._h), ST, "the two member stores hold different numbers of members")
    expect(f"source of {M + 1}: window_push", lambda: fill["window_push"](src._h), ST, "source " + slot(0))
    src.ens_reserve(M)
    for i in range(M):
      for name in fill:
        expect(f"source slot {i} unpushed: {name}", lambda: fill[name](src._h), ST, "source " + slot(i))
      src.ens_push_host(i, field)
    for name in fill:
      expect(f"source complete: {name}", lambda: fill[name](src._h), ST, f"no truth on the source handle (pass one to gc_ens_{name})")
    for nd in (h, src, clim, bad):
      for name in COUNTERS:
        if name != "launches_per_call":
          assert nd.counter(name) == 0, name
    assert not wrong, wrong
  finally:
    for nd in (h, src, clim, bad):
      nd.close()
