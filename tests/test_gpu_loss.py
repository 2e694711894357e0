"""The denoising loss on the device (gc_loss*, GenCast.denoising_loss) against a float64 reference built on the
oracle's denoiser forward.

Tolerance of the parity tests, derived (not measured): the project's per-element bound on the raw network output F
against the float64 oracle in the same mode is d = 1e-4 for float32 features (tests/test_gpu_parity.py TOL) and
d = 2e-2 for fp16 features (F16_TOL_MAX there).  D - t = c_out(s) (F + ...), so an error e with |e| <= d per element
of F moves a unit-mean-weighted mean of squares l_v = <(D - t)^2> by at most (Cauchy-Schwarz)
    |l'_v - l_v| <= c_out d (2 sqrt(l_v) + c_out d),
and loss = c_out^-2 sum_v w_v l_v by at most
    |loss' - loss| <= d sum_v w_v (2 sqrt(l_v) / c_out + d).
The reduction itself forms and adds every term in double and rounds once, so it adds one float32 rounding
(test_reduction_alone checks exactly that); it is not part of the bound's budget in any visible way (6e-8 relative).
"""
import numpy as np
import pytest

from oracle import gencast_oracle as O
from tests import helpers

pytestmark = pytest.mark.gpu
TOL, F16_TOL_MAX = 1e-4, 2e-2          # tests/test_gpu_parity.py:14 and :813
SIGMA_ENDS = np.array([0.02, 88.0], np.float32)      # NoiseConfig's training range


def _slots(dims):
  return np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32)


def _lat_weights_with_poles(n_lat):
  """Unit-mean weights of an equiangular grid with pole rows (common/losses.py:169-180)."""
  lat = np.linspace(-90.0, 90.0, n_lat)
  d = 180.0 / (n_lat - 1)
  w = np.cos(np.deg2rad(lat)) * np.sin(np.deg2rad(d / 2))
  w[[0, -1]] = np.sin(np.deg2rad(d / 4)) ** 2
  return w / w.mean()


def _tiny_weights(n_lat=13, n_lon=24):
  """3 groups over tiny's 6 output channels: two surface channels and one variable on levels 50 / 250 / 500 / 1000."""
  level = np.array([50.0, 250.0, 500.0, 1000.0])
  node = np.repeat(_lat_weights_with_poles(n_lat), n_lon) / (n_lat * n_lon)
  chan = np.concatenate([[1.0, 1.0], level / level.mean() / 4.0])
  return (node.astype(np.float32), chan.astype(np.float32), np.array([0, 1, 2, 2, 2, 2], np.int32),
          np.array([0.1, 1.0, 1.0], np.float32))


def _nano_weights():
  from gencast_flax_nnx_amd import losses, synthetic
  plan = losses.loss_plan(synthetic.make_example()[1])          # config.TASK on the 2.5 degree grid
  return plan.node_weight, plan.channel_weight, plan.channel_group, plan.group_weight


def _reference(weights, cond, targets, noise, sigma, slots, network=None, F=None):
  """Float64, the literal form of gencast/gencast.py:229-280: x = t + s n, D = c_out F(c_in x; s) + c_skip x,
  per_group = weighted mean of (D - t)^2, loss = c_out^-2 sum_g w_g per_group.  `F` given: the network is not run."""
  node, chan, group, gw = (np.asarray(a) for a in weights)
  s = np.asarray(sigma, np.float32).astype(np.float64)[None, :, None]
  t, n = targets.astype(np.float64), noise.astype(np.float64)
  c_in, c_out, c_skip = (s * s + 1.0) ** -0.5, s * (s * s + 1.0) ** -0.5, 1.0 / (s * s + 1.0)
  x = t + s * n
  if F is None:
    feats = cond.astype(np.float64).copy()
    feats[:, :, slots] = c_in * x
    F = network(feats, np.asarray(sigma, np.float32))
  D = c_out * np.asarray(F, np.float64) + c_skip * x
  cols = np.einsum("i,ibc->bc", node.astype(np.float64), (D - t) ** 2) * chan.astype(np.float64)
  per_group = np.zeros((t.shape[1], len(gw)))
  for c, g in enumerate(group):
    per_group[:, g] += cols[:, c]
  loss = (per_group @ gw.astype(np.float64)) * c_out[0, :, 0] ** -2
  return loss, per_group, D


def _network(params, gr, dims, **kw):
  return lambda f, s: O.denoiser_forward(params, helpers.graph_dict(gr), f, s, num_layers=dims.num_layers,
                                         num_heads=dims.num_heads, **kw)


def _assert_within_bound(tag, loss, per_group, ref_loss, ref_pg, sigma, gw, delta):
  s = np.asarray(sigma, np.float32).astype(np.float64)
  c_out = s / np.sqrt(s * s + 1.0)
  pg_bound = c_out[:, None] * delta * (2.0 * np.sqrt(ref_pg) + c_out[:, None] * delta)
  loss_bound = delta * ((2.0 * np.sqrt(ref_pg) / c_out[:, None] + delta) @ gw.astype(np.float64))
  pg_err, loss_err = np.abs(per_group - ref_pg), np.abs(loss - ref_loss)
  print(f"{tag}: loss {ref_loss} |err| {loss_err} bound {loss_bound}; per_group |err| max {pg_err.max(axis=1)} "
        f"bound min {pg_bound.min(axis=1)}")
  assert np.isfinite(loss).all() and np.isfinite(per_group).all()
  assert (pg_err <= pg_bound).all(), (tag, pg_err, pg_bound)
  assert (loss_err <= loss_bound).all(), (tag, loss_err, loss_bound)


def _tiny_case(seed=0):
  gr, dims, params, x, _ = helpers.tiny_setup(batch=2, seed=seed)
  rng = np.random.default_rng(100 + seed)
  targets = rng.standard_normal((gr.num_grid_nodes, 2, dims.c_out)).astype(np.float32)
  noise = rng.standard_normal((gr.num_grid_nodes, 2, dims.c_out)).astype(np.float32)
  return gr, dims, params, x, targets, noise


def _ready(nd, dims, weights):
  nd.set_noisy_slots(_slots(dims))
  nd.loss_set_weights(weights[0], weights[1], weights[2], weights[3])


# ---- 1. parity, tiny ------------------------------------------------------------------------------------
@pytest.mark.parametrize("features", ["f32", "f16"])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_loss_matches_the_float64_reference_tiny(precision, features):
  gr, dims, params, cond, targets, noise = _tiny_case()
  weights = _tiny_weights()
  nd = helpers.make_native(gr, dims, params, 2, precision=precision)
  try:
    if features == "f16":
      nd.set_option("features", "f16")
    _ready(nd, dims, weights)
    loss, per_group = nd.loss(cond, targets, noise, SIGMA_ENDS)
    kw = dict(attention="neighbour", feature_dtype=np.float16) if features == "f16" else dict(attention="dense")
    ref_loss, ref_pg, _ = _reference(weights, cond, targets, noise, SIGMA_ENDS, _slots(dims), _network(params, gr, dims, **kw))
    _assert_within_bound(f"tiny {precision}/{features}", loss, per_group, ref_loss, ref_pg, SIGMA_ENDS, weights[3],
                         F16_TOL_MAX if features == "f16" else TOL)
    assert nd.counter("loss_evaluations") == 1 and nd.counter("range_fallbacks") == 0
  finally:
    nd.close()


# ---- 2. parity, nano ------------------------------------------------------------------------------------
def test_loss_matches_the_float64_reference_nano():
  gr, dims, params, cond, _ = helpers.nano_setup()
  rng = np.random.default_rng(7)
  targets = rng.standard_normal((gr.num_grid_nodes, 1, dims.c_out)).astype(np.float32)
  noise = rng.standard_normal((gr.num_grid_nodes, 1, dims.c_out)).astype(np.float32)
  weights = _nano_weights()
  assert len(weights[3]) == 10
  sigma = np.array([3.0], np.float32)
  ref_loss, ref_pg, _ = _reference(weights, cond, targets, noise, sigma, _slots(dims), _network(params, gr, dims, attention="dense"))
  for precision in ("f16x3", "f32"):
    nd = helpers.make_native(gr, dims, params, 1, precision=precision)
    try:
      _ready(nd, dims, weights)
      loss, per_group = nd.loss(cond, targets, noise, sigma)
      _assert_within_bound(f"nano {precision}", loss, per_group, ref_loss, ref_pg, sigma, weights[3], TOL)
      # 3. (nano) the reduction alone, from the device's own F
      F = nd.debug_fetch("y").reshape(targets.shape)
      host_loss, host_pg, _ = _reference(weights, cond, targets, noise, sigma, _slots(dims), F=F)
      assert (np.abs(per_group - host_pg) <= 2.0 ** -23 * host_pg).all()
      assert (np.abs(loss - host_loss) <= 2.0 ** -23 * host_loss).all()
    finally:
      nd.close()


# ---- 3. the reduction alone -------------------------------------------------------------------------------
def test_reduction_alone_is_one_float32_rounding_from_float64():
  """per_group and loss recomputed on the host in float64 from the device's OWN F, the same targets, noise and
  float32 weight arrays, in the literal form: the device forms and adds in double, so what is left is the final cast
  (2^-24 relative) plus the order of the double sums -- asserted with a factor 2: 2^-23."""
  gr, dims, params, cond, targets, noise = _tiny_case(seed=1)
  weights = _tiny_weights()
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    _ready(nd, dims, weights)
    loss, per_group, den = nd.loss(cond, targets, noise, SIGMA_ENDS, want_denoised=True)
    F = nd.debug_fetch("y").reshape(targets.shape)
    host_loss, host_pg, host_D = _reference(weights, cond, targets, noise, SIGMA_ENDS, _slots(dims), F=F)
    print("reduction alone: rel err per_group", np.abs(per_group - host_pg) / host_pg, "loss", np.abs(loss - host_loss) / host_loss)
    assert (np.abs(per_group - host_pg) <= 2.0 ** -23 * host_pg).all()
    assert (np.abs(loss - host_loss) <= 2.0 ** -23 * host_loss).all()
    # D is float32 arithmetic on float32 x = t + s n: a few ulps of its largest term
    assert np.abs(den - host_D).max() <= 8 * 2.0 ** -24 * np.abs(host_D).max()
  finally:
    nd.close()


# ---- 4. determinism and isolation -------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", ["on", "off"])
def test_evaluations_are_deterministic_and_leave_the_sampler_alone(graphs):
  gr, dims, params, cond, targets, noise = _tiny_case(seed=2)
  weights = _tiny_weights()
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    nd.set_option("graphs", graphs)
    _ready(nd, dims, weights)
    nd.upload_cond(cond)
    nd.upload_targets(targets)
    nd.upload_noise(noise)
    sig3 = np.array([[0.02, 88.0], [1.0, 5.0], [40.0, 0.3]], np.float32)
    a = nd.loss_resident(sig3[0])
    b = nd.loss_resident(sig3[0])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    many = nd.loss_resident(sig3)
    assert many[0].shape == (3, 2) and many[1].shape == (3, 2, 3)
    for k in range(3):
      one = nd.loss_resident(sig3[k])
      np.testing.assert_array_equal(many[0][k], one[0][0])
      np.testing.assert_array_equal(many[1][k], one[1][0])
    # sample, sample (with graphs on: captured here), loss evaluation, sample again (a replay): identical bits
    sched = O.noise_schedule(80.0, 0.03, 4, 7.0).astype(np.float32)
    nd.sample_resident(sched)
    first = nd.download_sample()
    nd.sample_resident(sched)
    np.testing.assert_array_equal(nd.download_sample(), first)
    replays = nd.counter("graph_replays")
    again = nd.loss_resident(sig3)
    np.testing.assert_array_equal(again[0], many[0])                       # and the sampler left the loss state alone
    np.testing.assert_array_equal(nd.download_sample(), first)             # the last sample is still there
    nd.sample_resident(sched)
    np.testing.assert_array_equal(nd.download_sample(), first)
    np.testing.assert_array_equal(nd.download_noise(), noise)
    if graphs == "on":
      assert nd.counter("graph_captures") == 1 and nd.counter("graph_replays") == replays + 1
    else:
      assert nd.counter("graph_captures") == 0
    assert nd.counter("loss_evaluations") == 2 + 3 + 3 + 3
  finally:
    nd.close()


# ---- 5. identity and negative control ---------------------------------------------------------------------
def test_group_weights_select_groups_and_the_group_map_matters():
  gr, dims, params, cond, targets, noise = _tiny_case(seed=3)
  node, chan, group, gw = _tiny_weights()
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    nd.set_noisy_slots(_slots(dims))
    nd.loss_set_weights(node, chan, group, gw)
    _, pg = nd.loss(cond, targets, noise, SIGMA_ENDS)
    s = SIGMA_ENDS.astype(np.float64)
    lam = (s * s + 1.0) / (s * s)
    for g in range(3):
      only = np.zeros(3, np.float32)
      only[g] = 0.7
      nd.loss_set_weights(node, chan, group, only)
      loss_g, pg_g = nd.loss(cond, targets, noise, SIGMA_ENDS)
      np.testing.assert_array_equal(pg_g, pg)
      want = lam * np.float32(0.7).astype(np.float64) * pg[:, g].astype(np.float64)
      assert (np.abs(loss_g - want) <= 2.0 ** -22 * want).all()             # per_group was rounded once already
    swapped = group.copy()
    swapped[[1, 2]] = swapped[[2, 1]]                                       # columns 1 and 2 change groups
    nd.loss_set_weights(node, chan, swapped, gw)
    _, pg_s = nd.loss(cond, targets, noise, SIGMA_ENDS)
    np.testing.assert_array_equal(pg_s[:, 0], pg[:, 0])
    assert (pg_s[:, 1] != pg[:, 1]).all() and (pg_s[:, 2] != pg[:, 2]).all()
  finally:
    nd.close()


# ---- 6. device noise ---------------------------------------------------------------------------------------
def test_evaluation_on_a_device_drawn_field():
  from oracle import noise_oracle as NO
  from gencast_flax_nnx_amd import noise as noise_mod
  gr, dims, params, cond, targets, _ = _tiny_case(seed=4)
  weights = _tiny_weights()
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    _ready(nd, dims, weights)
    lat, lon = np.linspace(-90, 90, 13), np.arange(24) * 15.0
    nd.upload_cond(cond)
    nd.upload_targets(targets)
    with pytest.raises(Exception, match="gc_noise_set_tables"):
      nd.loss_resident(SIGMA_ENDS, draw_noise=True)
    nd.noise_set_tables(13, 24, *noise_mod.SphericalNoise(lat, lon).device_tables())
    seed, stream, N = 9, 3, 2 * dims.c_out
    nd.noise_seed(seed, stream)
    loss, pg = nd.loss_resident(SIGMA_ENDS, draw_noise=True)
    field = nd.download_noise()
    assert np.abs(field.reshape(-1, N) - NO.device_field(seed, stream, lat, lon, N)).max() < 2e-5
    loss_given, pg_given = nd.loss(cond, targets, field, SIGMA_ENDS)         # the same field as GIVEN noise: same bits
    np.testing.assert_array_equal(loss_given, loss[0])
    np.testing.assert_array_equal(pg_given, pg[0])
    nd.loss_resident(SIGMA_ENDS, draw_noise=True)                            # the next evaluation used stream + 1
    assert np.abs(nd.download_noise().reshape(-1, N) - NO.device_field(seed, stream + 1, lat, lon, N)).max() < 2e-5
    both = nd.loss_resident(np.stack([SIGMA_ENDS, SIGMA_ENDS]), draw_noise=True)   # streams + 2 and + 3
    assert np.abs(nd.download_noise().reshape(-1, N) - NO.device_field(seed, stream + 3, lat, lon, N)).max() < 2e-5
    assert (both[0][0] != both[0][1]).all()
  finally:
    nd.close()


# ---- 7. domain guard -----------------------------------------------------------------------------------------
def test_out_of_range_conditioning_takes_the_exact_f32_kernels():
  gr, dims, params, x, _ = helpers.tiny_setup(batch=2, seed=21)
  rng = np.random.default_rng(121)
  targets = rng.standard_normal((gr.num_grid_nodes, 2, dims.c_out)).astype(np.float32)
  noise = rng.standard_normal((gr.num_grid_nodes, 2, dims.c_out)).astype(np.float32)
  weights = _tiny_weights()
  big = x.copy()
  big[:, :, 3] *= 2.0e5                                    # one un-normalised conditioning channel (not a noisy slot)
  nd = helpers.make_native(gr, dims, params, 2)
  nd32 = helpers.make_native(gr, dims, params, 2, precision="f32")
  try:
    _ready(nd, dims, weights)
    _ready(nd32, dims, weights)
    loss, pg = nd.loss(big, targets, noise, SIGMA_ENDS)
    assert nd.counter("range_fallbacks") == 1
    ref_loss, ref_pg, _ = _reference(weights, big, targets, noise, SIGMA_ENDS, _slots(dims), _network(params, gr, dims, attention="dense"))
    _assert_within_bound("guard vs oracle", loss, pg, ref_loss, ref_pg, SIGMA_ENDS, weights[3], TOL)
    loss32, pg32 = nd32.loss(big, targets, noise, SIGMA_ENDS)
    assert nd32.counter("range_fallbacks") == 0
    _assert_within_bound("guard vs the f32 handle", loss, pg, loss32.astype(np.float64), pg32.astype(np.float64), SIGMA_ENDS,
                         weights[3], TOL)
    edge = x.copy()
    edge[:, :, 3] = np.where(edge[:, :, 3] > 0, 65000.0, -65000.0)          # inside the domain: no re-run
    loss_e, _ = nd.loss(edge, targets, noise, SIGMA_ENDS)
    assert nd.counter("range_fallbacks") == 1 and np.isfinite(loss_e).all()
    # several evaluations in one call, all poisoned: every one is re-run and counted
    nd.upload_cond(big)
    many = nd.loss_resident(np.stack([SIGMA_ENDS, SIGMA_ENDS[::-1]]))
    assert nd.counter("range_fallbacks") == 3
    np.testing.assert_array_equal(many[0][0], loss)
    # ... and on device-drawn fields: each re-run draws ITS Philox stream again, the buffer ends on the last field
    from oracle import noise_oracle as NO
    from gencast_flax_nnx_amd import noise as noise_mod
    lat, lon = np.linspace(-90, 90, 13), np.arange(24) * 15.0
    tables = noise_mod.SphericalNoise(lat, lon).device_tables()
    nd.noise_set_tables(13, 24, *tables)
    nd32.noise_set_tables(13, 24, *tables)
    nd32.upload_cond(big)
    nd32.upload_targets(targets)
    sig2 = np.stack([SIGMA_ENDS, SIGMA_ENDS[::-1]])
    nd.noise_seed(17, 4)
    drawn = nd.loss_resident(sig2, draw_noise=True)
    assert nd.counter("range_fallbacks") == 5
    N = 2 * dims.c_out
    last_field = nd.download_noise()
    assert np.abs(last_field.reshape(-1, N) - NO.device_field(17, 5, lat, lon, N)).max() < 2e-5
    for e in range(2):
      nd32.noise_seed(17, 4 + e)
      l32, p32 = nd32.loss_resident(sig2[e], draw_noise=True)
      _assert_within_bound(f"guard, drawn field {e} vs the f32 handle", drawn[0][e], drawn[1][e], l32[0].astype(np.float64),
                           p32[0].astype(np.float64), sig2[e], weights[3], TOL)
    given = nd.loss(big, targets, last_field, sig2[1])                      # the same field as given noise: the same bits
    np.testing.assert_array_equal(given[0], drawn[0][1])
    np.testing.assert_array_equal(given[1], drawn[1][1])
    nd.loss_resident(SIGMA_ENDS, draw_noise=True)                           # the stream counter went on from the last evaluation
    assert np.abs(nd.download_noise().reshape(-1, N) - NO.device_field(17, 6, lat, lon, N)).max() < 2e-5
  finally:
    nd.close()
    nd32.close()


# ---- 8. Dataset level ----------------------------------------------------------------------------------------
def _small_model(rngs=7, batch=2, seed=4):
  import dataclasses
  from gencast_flax_nnx_amd import GenCast, config, synthetic, weights
  from gencast_flax_nnx_amd.denoiser import dims_from_arch
  arch = config.nano_architecture(mesh_size=2, d_model=128, num_layers=2, num_heads=2)
  arch.sparse_transformer_config.ffw_hidden = 256
  arch.sparse_transformer_config.attention_k_hop = 2
  arch = dataclasses.replace(arch, node_output_size=82)
  lat, lon = np.linspace(-90, 90, 13), np.arange(24) * 15.0
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=batch, seed=seed)
  params = weights.random_params(dims_from_arch(arch, 262, 82), seed=3)
  sc = config.SamplerConfig(num_noise_levels=4, stochastic_churn_rate=0.0)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=rngs)
  return gc, inp, tgt, frc


def test_dataset_level_loss():
  from gencast_flax_nnx_amd import GenCast, NaNCleaner, compute_loss, config, datasets, losses, rollout, synthetic, validation_loss
  from gencast_flax_nnx_amd.datasets import Dataset, Variable
  gc, inp, tgt, frc = _small_model()
  try:
    loss, diag = gc.denoising_loss(inp, tgt, frc, rngs=11)
    assert loss.dims == ("batch",) and loss.data.shape == (2,) and np.isfinite(loss.data).all() and (loss.data > 0).all()
    assert sorted(diag.keys()) == sorted(config.TASK.target_variables)
    assert all(diag[k].dims == ("batch",) and diag[k].data.shape == (2,) for k in diag.keys())
    loss2, diag2 = gc.denoising_loss(inp, tgt, frc, rngs=11)                 # equal rngs: equal results
    np.testing.assert_array_equal(loss.data, loss2.data)
    assert (gc.denoising_loss(inp, tgt, frc, rngs=12)[0].data != loss.data).all()
    # loss = lambda sum_v w_v l_v with the reference's table, from the returned diagnostics
    sig = np.array([0.5, 7.0], np.float32)
    G = 13 * 24
    field = np.random.default_rng(3).standard_normal((G, 2, 82)).astype(np.float32)
    (l3, d3), preds = gc.denoising_loss_and_predictions(inp, tgt, frc, noise_levels=sig, noise=field)
    s = sig.astype(np.float64)
    want = sum(losses.DEFAULT_PER_VARIABLE_WEIGHTS.get(k, 1.0) * d3[k].data.astype(np.float64) for k in d3.keys()) * (s * s + 1) / (s * s)
    np.testing.assert_allclose(l3.data, want, rtol=1e-6)
    # the predictions are the D of that evaluation: the host loss of (preds, targets) is the device's
    host_total, host_diag = losses.weighted_mse_per_level(preds, tgt, losses.DEFAULT_PER_VARIABLE_WEIGHTS)
    for k in d3.keys():
      np.testing.assert_allclose(host_diag[k].data, d3[k].data, rtol=2e-5)   # D is stored as float32: (D - t)^2 to ~1e-6
    np.testing.assert_allclose(host_total.data * (s * s + 1) / (s * s), l3.data, rtol=2e-5)
    D = gc.denoiser.native.download_denoised()
    np.testing.assert_array_equal(datasets.dataset_to_stacked(preds, preds.sizes).transpose(1, 2, 0, 3).reshape(G, 2, 82), D)
    # ... and D = c_out F + c_skip x for the F the device holds
    F = gc.denoiser.native.debug_fetch("y").reshape(G, 2, 82).astype(np.float64)
    t = datasets.dataset_to_stacked(tgt, tgt.sizes).transpose(1, 2, 0, 3).reshape(G, 2, 82).astype(np.float64)
    sb = s[None, :, None]
    D_ref = sb / np.sqrt(sb * sb + 1) * F + (t + sb * field) / (sb * sb + 1)
    assert np.abs(D - D_ref).max() <= 8 * 2.0 ** -24 * np.abs(D_ref).max()
    # compute_loss: batch means
    m, md = compute_loss(gc, inp, tgt, frc, noise_levels=sig, noise=field)
    assert m == pytest.approx(float(l3.data.astype(np.float64).mean()), rel=1e-12)
    assert md["temperature"] == pytest.approx(float(d3["temperature"].data.astype(np.float64).mean()), rel=1e-12)
    # InputsAndResiduals: the inner loss on hand-normalised data; predictions un-normalised
    srng = np.random.default_rng(5)
    def stat(lo, hi):                         # a statistic per variable: per level for the atmospheric ones
      names = set(config.TASK.input_variables) | set(config.TASK.target_variables)
      return Dataset({n: (Variable(("level",), srng.uniform(lo, hi, 13).astype(np.float32)) if n in config.ALL_ATMOSPHERIC_VARS
                          else Variable((), np.float32(srng.uniform(lo, hi)))) for n in sorted(names)})
    stats = (stat(0.5, 2.0), stat(-1.0, 1.0), stat(0.1, 0.5))       # stddev, mean, stddev of the differences
    norm = rollout.InputsAndResiduals(gc, *stats)
    ln, dn = norm.denoising_loss(inp, tgt, frc, noise_levels=sig, noise=field)
    def by_level(st, v):                      # a () or ('level',) statistic against a variable's dims
      a = np.asarray(st.data)
      return a.reshape([-1 if d == "level" else 1 for d in v.dims]) if a.ndim else a
    def plain(ds):                            # (x - mean) / stddev
      return Dataset({k: Variable(v.dims, (v.data - by_level(stats[1][k], v)) / by_level(stats[0][k], v)) for k, v in ds.items()}, ds.coords)
    def residual(k, v):                       # every target is an input too: (target - last input frame) / stddev of differences
      last = np.take(inp[k].data, [-1], axis=inp[k].dims.index("time"))
      return Variable(v.dims, (v.data - last) / by_level(stats[2][k], v))
    assert set(tgt.keys()) <= set(inp.keys())
    ni, nf = plain(inp), plain(frc)
    nt = Dataset({k: residual(k, v) for k, v in tgt.items()}, tgt.coords)
    li, _ = gc.denoising_loss(ni, nt, nf, noise_levels=sig, noise=field)
    np.testing.assert_array_equal(ln.data, li.data)
    assert (ln.data != l3.data).all()
    (_, _), pn = norm.denoising_loss_and_predictions(inp, tgt, frc, noise_levels=sig, noise=field)
    _, inner_pred = gc.denoising_loss_and_predictions(ni, nt, nf, noise_levels=sig, noise=field)
    k = "2m_temperature"
    back = inner_pred[k].data * np.asarray(stats[2][k].data) + inp[k].data[:, -1:]
    np.testing.assert_array_equal(pn[k].data, back)
    # NaNCleaner cleans the targets (and inputs): a NaN target point would otherwise poison the loss
    dirty = tgt.assign(Dataset({k: Variable(tgt[k].dims, tgt[k].data.copy())}))
    dirty[k].data[0, 0, 5, 7] = np.nan
    nc = NaNCleaner(gc, k, Dataset({k: Variable((), np.float32(0.25))}))
    lc, _ = nc.denoising_loss(inp, dirty, frc, noise_levels=sig, noise=field)
    filled = tgt.assign(Dataset({k: Variable(tgt[k].dims, np.where(np.isnan(dirty[k].data), np.float32(0.25), dirty[k].data))}))
    lf, _ = gc.denoising_loss(inp, filled, frc, noise_levels=sig, noise=field)
    np.testing.assert_array_equal(lc.data, lf.data)
    assert np.isfinite(lc.data).all() and np.isnan(dirty[k].data).sum() == 1
    # validation_loss: two batches x 3 draws = the mean of six single evaluations drawn from one generator
    inp_b, tgt_b, frc_b = synthetic.make_example(lat=np.linspace(-90, 90, 13), lon=np.arange(24) * 15.0, batch=2, seed=9)
    mean, per_var = validation_loss(gc, [(inp, tgt, frc), (inp_b, tgt_b, frc_b)], noise_levels_per_batch=3, rngs=5)
    gen = np.random.default_rng(5)
    singles, singles_t = [], []
    for batch_ in ((inp, tgt, frc), (inp_b, tgt_b, frc_b)):
      for _ in range(3):
        l1, d1 = gc.denoising_loss(*batch_, rngs=gen)
        singles.append(l1.data.astype(np.float64))
        singles_t.append(d1["temperature"].data.astype(np.float64))
    assert mean == pytest.approx(float(np.mean(singles)), rel=1e-12)
    assert per_var["temperature"] == pytest.approx(float(np.mean(singles_t)), rel=1e-12)
    assert len(per_var) == 10
    # device noise: a batch's K draws are ONE native call on Philox streams 0..K-1 of one key
    from oracle import noise_oracle as NO
    from gencast_flax_nnx_amd import Sampler
    native = gc.denoiser.native
    gc._sampler.device_noise = True
    before = native.counter("loss_evaluations")
    lk, dk = gc.denoising_loss(inp, tgt, frc, rngs=21, num_noise_draws=3)
    assert native.counter("loss_evaluations") == before + 3
    assert lk.dims == ("draw", "batch") and lk.data.shape == (3, 2) and np.isfinite(lk.data).all()
    assert len({float(v) for v in lk.data[:, 0]}) == 3
    key = Sampler.seed_from(np.random.default_rng(21))                    # the key is drawn first, then the levels
    lat13, lon24 = np.linspace(-90, 90, 13), np.arange(24) * 15.0
    assert np.abs(native.download_noise().reshape(G, -1) - NO.device_field(key, 2, lat13, lon24, 2 * 82)).max() < 2e-5
    l1, d1 = gc.denoising_loss(inp, tgt, frc, rngs=21)                    # draw 0 is what a single call draws
    np.testing.assert_array_equal(l1.data, lk.data[0])
    np.testing.assert_array_equal(d1["geopotential"].data, dk["geopotential"].data[0])
    assert np.abs(native.download_noise().reshape(G, -1) - NO.device_field(key, 0, lat13, lon24, 2 * 82)).max() < 2e-5
    mean_dev, _ = validation_loss(gc, [(inp, tgt, frc)], noise_levels_per_batch=3, rngs=21)
    assert mean_dev == pytest.approx(float(lk.data.astype(np.float64).mean()), rel=1e-12)
    gc._sampler.device_noise = False
    # what does not change
    with pytest.raises(NotImplementedError):
      gc.loss(inp, tgt, frc)
    no_cfg = GenCast.__new__(GenCast)
    no_cfg.__dict__.update(gc.__dict__)
    no_cfg._noise_config = None
    with pytest.raises(ValueError, match="Noise config must be specified"):
      no_cfg.denoising_loss(inp, tgt, frc, rngs=1)
  finally:
    gc.denoiser.native.close()


# ---- 9. state and argument errors ------------------------------------------------------------------------------
def test_state_and_argument_errors():
  from gencast_flax_nnx_amd import _lib
  gr, dims, params, cond, targets, noise = _tiny_case(seed=5)
  node, chan, group, gw = _tiny_weights()
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    nd.set_noisy_slots(_slots(dims))
    nd.upload_cond(cond)
    nd.upload_noise(noise)
    with pytest.raises(_lib.GencastHipError, match="error 4.*weights"):       # GC_ERR_STATE
      nd.loss_resident(SIGMA_ENDS)
    nd.loss_set_weights(node, chan, group, gw)
    with pytest.raises(_lib.GencastHipError, match="error 4.*targets"):
      nd.loss_resident(SIGMA_ENDS)
    with pytest.raises(_lib.GencastHipError, match="error 4"):
      nd.download_denoised()
    nd.upload_targets(targets)
    with pytest.raises(ValueError, match="> 0"):                              # GC_ERR_INVALID_ARGUMENT
      nd.loss_resident(np.array([0.0, 1.0], np.float32))
    with pytest.raises(ValueError, match="> 0"):
      nd.loss_resident(np.array([[1.0, 1.0], [1.0, -2.0]], np.float32))
    bad = group.copy()
    bad[0] = 3
    with pytest.raises(ValueError, match="n_groups"):
      nd.loss_set_weights(node, chan, bad, gw)
    with pytest.raises(ValueError, match="1..64"):
      nd.loss_set_weights(node, chan, np.zeros(6, np.int32), np.ones(65, np.float32))
    loss, pg = nd.loss_resident(SIGMA_ENDS)                                   # the failed calls changed nothing
    assert loss.shape == (1, 2) and pg.shape == (1, 2, 3) and np.isfinite(loss).all()
  finally:
    nd.close()
