"""Ensemble verification on the device (gc_ens_*) against the float64 definition (tests/verification_reference.py).

Tolerances are derived, not measured.  For every sum S_k: |device - reference| <= (G + M^2 + 8) 2^-53 A_k, A_k the
reference's sum of the absolute values of the same terms -- G terms are added per column, at most about M^2 roundings
go into one term, and summation order is the only difference between the two computations.  A mean / variance field
value equals np.float32(reference) or one of its two float32 neighbours; the rank histogram is exact."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, geometry, verification
from gencast_flax_nnx_amd.verification import EnsembleScores
from tests import helpers
from tests.helpers import graph_handle as _handle, small_graph as _graph
from tests import verification_reference as R

pytestmark = pytest.mark.gpu


def _data(M, G, B, C, seed, scale=None):
  rng = np.random.default_rng(seed)
  scale = np.logspace(-3, 5, C) if scale is None else scale
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  return members, truth, w


def _push_all(nd, members, w):
  nd.ens_reserve(len(members))
  nd.ens_set_node_weight(w)
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _check_sums(tag, sums, hist, ref, G, M):
  tol = R.sum_tolerance(ref, G, M)
  err = np.abs(sums - ref["sums"])
  for k, name in enumerate(R.SUM_NAMES):
    print(f"{tag} {name}: max |device - reference| {err[..., k].max():.3e}, bound at that column "
          f"{tol[..., k].reshape(-1)[err[..., k].argmax()]:.3e}, worst ratio {np.max(err[..., k] / np.maximum(tol[..., k], 1e-300)):.3f}")
  for k, name in enumerate(R.SUM_NAMES):
    assert np.all(err[..., k] <= tol[..., k]), f"{tag}: {name} outside (G + M^2 + 8) 2^-53 A_k"
  np.testing.assert_array_equal(hist, ref["hist"], err_msg=tag)


def _check_fields(tag, mean, var, ref):
  for name, got, want in (("mean", mean, ref["mean"]), ("variance", var, ref["variance"])):
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{tag} {name}: NaN entries")
    lo, hi = R.float32_neighbours(want[~nan])
    g = got[~nan]
    print(f"{tag} {name}: {int((g != want[~nan].astype(np.float32)).sum())} of {g.size} values are a float32 neighbour")
    assert np.all((g >= lo) & (g <= hi)), f"{tag}: {name} field further than one float32 neighbour from the reference"


# ---- 1. tiny graph, every M ------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 8, 50, 64])
def test_scores_match_the_float64_definition_tiny(M):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w = _data(M, G, B, C, seed=M)
  ref = R.reference(members, truth, w)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    sums, hist = nd.ens_score(truth, want_fields=True)
    assert sums.shape == (B, C, 6) and hist.shape == (B, C, M + 1) and hist.dtype == np.uint64
    _check_sums(f"tiny M={M}", sums, hist, ref, G, M)
    _check_fields(f"tiny M={M}", *nd.ens_download_fields(), ref)
    assert nd.counter("ens_invalid_points") == 0 and nd.counter("ens_scores") == 1
    np.testing.assert_array_equal(hist.sum(-1), np.full((B, C), G, np.uint64))
    # the truth stays on the device; without fields the sums are the same bytes
    again, hist2 = nd.ens_score(None)
    np.testing.assert_array_equal(again, sums)
    np.testing.assert_array_equal(hist2, hist)
    # derived scores against the reference's
    sc = EnsembleScores(sums, hist, M)
    for name, want in R.scores(ref, M).items():
      np.testing.assert_allclose(getattr(sc, name), want, rtol=1e-9, err_msg=name)
  finally:
    nd.close()


def test_a_second_column_tile_of_one_column():
  """(B, C) = (1, 257): the second column tile is one column wide, so it has 256 node lanes -- more than the 8 nodes of a
  block, most lanes walk nothing -- and the finish folds 256 lanes of at most one block each."""
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 1, 257, 3
  members, truth, w = _data(M, G, B, C, seed=257)
  ref = R.reference(members, truth, w)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    sums, hist = nd.ens_score(truth, want_fields=True)
    _check_sums("W=257", sums, hist, ref, G, M)
    _check_fields("W=257", *nd.ens_download_fields(), ref)
  finally:
    nd.close()


# ---- 2. full-size grids, set_graph only ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["nano", "one_degree"])
def test_scores_match_the_float64_definition_full_size(case):
  if case == "nano":
    gr, M, hw = _graph(73, 144, mesh_size=4, k_hop=8), 50, dict(latent=256, heads=4, ffw=2048)
  else:
    lat, lon = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0)
    gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=5, attention_k_hop=8)
    M, hw = 8, dict(latent=512, heads=4, ffw=2048)
  G, B, C = gr.num_grid_nodes, 1, 82
  assert G == (10512 if case == "nano" else 65160)
  members, truth, w = _data(M, G, B, C, seed=11, scale=np.logspace(-2, 4, C))
  ref = R.reference(members, truth, w)
  nd = _handle(gr, B, C, **hw)
  try:
    _push_all(nd, members, w)
    sums, hist = nd.ens_score(truth, want_fields=True)
    _check_sums(case, sums, hist, ref, G, M)
    _check_fields(case, *nd.ens_download_fields(), ref)
    print(f"{case}: ens_score_device_us {nd.counter('ens_score_device_us')}")
    # the regime: loss_reduce_blocks with W = 82, q = 3 node lanes: min(kLossMaxBlocks = 2048, ceil(G / (8 q))) -- below the
    # cap at nano (ceil(10512 / 24) = 438), capped at one degree (2715 -> 2048, per = 32, 11 trailing workgroups without nodes)
    assert nd.counter("ens_score_blocks") == (438 if case == "nano" else 2048)
  finally:
    nd.close()


# ---- 3. ties and invalid points -----------------------------------------------------------------------------------
def test_ties_and_invalid_points_are_counted_exactly():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, _ = _data(M, G, B, C, seed=21)
  w = (np.arange(G) % 7 + 1).astype(np.float32) / 8.0             # dyadic: their sums are exact in any order
  ties = np.array([0, 5, 77, 200, G - 1])
  nan_nodes = np.array([3, 4, 150, 151, 152, 300])
  inf_nodes = np.array([9, 120, 250])
  truth[ties] = members[3][ties]
  truth[nan_nodes] = np.nan
  members[5, inf_nodes, 1, 2] = np.inf
  members[6, inf_nodes[0], 0, 4] = -np.inf
  ref = R.reference(members, truth, w)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    sums, hist = nd.ens_score(truth, want_fields=True)
    mean, var = nd.ens_download_fields()
    _check_sums("ties", sums, hist, ref, G, M)
    _check_fields("ties", mean, var, ref)
    # ranks at the tied points: the members strictly below member 3; the tie itself does not count
    for b in range(B):
      for c in range(C):
        if (b, c) in ((1, 2), (0, 4)):
          continue
        rest = np.ones(G, bool)
        rest[np.concatenate([ties, nan_nodes])] = False
        below = (members[:, :, b, c] < truth[None, :, b, c]).sum(0)
        want = np.bincount(below[rest], minlength=M + 1) + \
            np.bincount((members[:, ties, b, c] < members[3][ties, b, c]).sum(0), minlength=M + 1)
        np.testing.assert_array_equal(hist[b, c], want.astype(np.uint64))
        assert hist[b, c, M] == np.bincount(below[rest], minlength=M + 1)[M]      # a tie is never "above all members"
    # S0, exactly: the weight of the nodes that are neither NaN in the truth nor Inf in a member
    keep = np.ones((G, B, C), bool)
    keep[nan_nodes] = False
    keep[inf_nodes, 1, 2] = False
    keep[inf_nodes[0], 0, 4] = False
    np.testing.assert_array_equal(sums[..., 0], (w.astype(np.float64)[:, None, None] * keep).sum(0))
    np.testing.assert_array_equal(hist.sum(-1), keep.sum(0).astype(np.uint64))
    assert nd.counter("ens_invalid_points") == int((~keep).sum()) == len(nan_nodes) * B * C + len(inf_nodes) + 1
    # the fields need no truth: NaN exactly where a member is not finite
    want_nan = np.zeros((G, B, C), bool)
    want_nan[inf_nodes, 1, 2] = True
    want_nan[inf_nodes[0], 0, 4] = True
    np.testing.assert_array_equal(np.isnan(mean), want_nan)
    np.testing.assert_array_equal(np.isnan(var), want_nan)
    assert np.isfinite(sums).all()
  finally:
    nd.close()


# ---- 4. determinism and ownership ---------------------------------------------------------------------------------------
def test_scoring_is_deterministic_and_the_store_is_replaced_not_grown():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w = _data(M, G, B, C, seed=31)
  nd = _handle(gr, B, C)
  try:
    base = nd.counter("device_allocations")
    _push_all(nd, members, w)
    a = nd.ens_score(truth, want_fields=True)
    fa = nd.ens_download_fields()
    b = nd.ens_score(truth, want_fields=True)
    fb = nd.ens_download_fields()
    for x, y in zip(a + fa, b + fb):
      assert x.tobytes() == y.tobytes()
    held = nd.counter("device_allocations")
    assert held > base
    for _ in range(3):
      nd.ens_reserve(M)
      for i in reversed(range(M)):                                # push order does not matter, slots do
        nd.ens_push_host(i, members[i])
      c = nd.ens_score(None, want_fields=True)
      fc = nd.ens_download_fields()
      for x, y in zip(a + fa, c + fc):
        assert x.tobytes() == y.tobytes()
      assert nd.counter("device_allocations") == held
    nd.ens_reserve(3)                                             # another M: still replaced
    assert nd.counter("device_allocations") == held
    assert nd.counter("ens_scores") == 5
  finally:
    nd.close()


# ---- 5. through the sampler --------------------------------------------------------------------------------------------
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


def _stack(ds):
  from gencast_flax_nnx_amd import datasets
  a = np.transpose(datasets.dataset_to_stacked(ds, ds.sizes), (1, 2, 0, 3))
  return np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]), dtype=np.float32)


@pytest.mark.parametrize("concurrent", [1, 2])
def test_sampler_scores_equal_the_reference_on_the_members_it_returns(concurrent):
  from gencast_flax_nnx_amd import EnsembleSampler
  gc, inp, tgt, frc = _small_model()
  try:
    ens = EnsembleSampler(gc._sampler, base_seed=5, concurrent_members=concurrent)
    fields = [_stack(d) for _, d in sorted(ens(inp, tgt.map(np.zeros_like), frc, 4), key=lambda t: t[0])]
    truth, w = _stack(tgt), verification.node_weights(tgt)
    ref = R.reference(np.stack(fields), truth, w)
    sc, mean, var = ens.scores(inp, tgt, frc, 4, fields=True)
    G = truth.shape[0]
    _check_sums(f"sampler x{concurrent}", sc.sums, sc.rank_histogram, ref, G, 4)
    _check_fields(f"sampler x{concurrent}", _stack(mean), _stack(var), ref)
    assert sc.n_members == 4 and np.isfinite(sc.crps).all() and (sc.crps > 0).all()
    # GenCast.ensemble_scores is the same run
    sc2 = gc.ensemble_scores(inp, tgt, frc, num_members=4, rngs=5, concurrent_members=concurrent)
    np.testing.assert_array_equal(sc2.sums, sc.sums)
    np.testing.assert_array_equal(sc2.rank_histogram, sc.rank_histogram)
    with pytest.raises(ValueError, match="ens_push_host"):
      EnsembleSampler(gc._sampler, rank=0, world_size=2).scores(inp, tgt, frc, 4)
  finally:
    gc.denoiser.native.close()


@pytest.mark.parametrize("graphs", ["on", "off"])
def test_pushing_and_scoring_leave_the_sampler_state_alone(graphs):
  from oracle import gencast_oracle as O
  gr, dims, params, cond, _ = helpers.tiny_setup(batch=2, seed=2)
  rng = np.random.default_rng(8)
  G = gr.num_grid_nodes
  noise = rng.standard_normal((G, 2, dims.c_out)).astype(np.float32)
  truth = rng.standard_normal((G, 2, dims.c_out)).astype(np.float32)
  nd = helpers.make_native(gr, dims, params, 2)
  other = helpers.make_native(gr, dims, params, 2)
  try:
    for h in (nd, other):
      h.set_option("graphs", graphs)
      h.set_noisy_slots(np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32))
      h.upload_cond(cond)
    nd.upload_noise(noise)
    other.upload_noise(-noise)
    sched = O.noise_schedule(80.0, 0.03, 4, 7.0).astype(np.float32)
    nd.sample_resident(sched)
    first = nd.download_sample()
    nd.sample_resident(sched)                                      # with graphs on: captured here
    np.testing.assert_array_equal(nd.download_sample(), first)
    nd.stash_sample()
    other.sample_resident(sched)
    second = other.download_sample()
    replays, captures = nd.counter("graph_replays"), nd.counter("graph_captures")
    nd.ens_reserve(2)
    nd.ens_set_node_weight(np.ones(G, np.float32))
    nd.ens_push(0)
    nd.ens_push(1, src=other)
    sums, hist = nd.ens_score(truth, want_fields=True)
    ref = R.reference(np.stack([first, second]), truth, np.ones(G, np.float32))
    _check_sums("pushed samples", sums, hist, ref, G, 2)
    _check_fields("pushed samples", *nd.ens_download_fields(), ref)
    np.testing.assert_array_equal(nd.download_sample(), first)      # the last sample is still there
    np.testing.assert_array_equal(nd.download_stash(), first)
    np.testing.assert_array_equal(other.download_sample(), second)
    np.testing.assert_array_equal(nd.download_cond(), cond)
    np.testing.assert_array_equal(nd.download_noise(), noise)
    nd.sample_resident(sched)                                      # a replay of the captured graph: the same bytes
    np.testing.assert_array_equal(nd.download_sample(), first)
    assert nd.counter("graph_captures") == captures
    if graphs == "on":
      assert nd.counter("graph_replays") == replays + 1
  finally:
    nd.close()
    other.close()


# ---- 6. Dataset level ------------------------------------------------------------------------------------------------
def test_dataset_level_scores_in_physical_units(monkeypatch):
  import sys
  from gencast_flax_nnx_amd import EnsembleSampler, NaNCleaner, config, datasets, rollout
  from gencast_flax_nnx_amd.datasets import Dataset, Variable
  from tests import fake_xarray
  monkeypatch.setitem(sys.modules, "xarray", fake_xarray)
  gc, inp, tgt, frc = _small_model()
  M = 4
  try:
    srng = np.random.default_rng(5)
    def stat(lo, hi):
      names = set(config.TASK.input_variables) | set(config.TASK.target_variables)
      return Dataset({n: (Variable(("level",), srng.uniform(lo, hi, 13).astype(np.float32)) if n in config.ALL_ATMOSPHERIC_VARS
                          else Variable((), np.float32(srng.uniform(lo, hi)))) for n in sorted(names)})
    stats = (stat(0.5, 2.0), stat(-1.0, 1.0), stat(0.1, 0.5))
    norm = rollout.InputsAndResiduals(gc, *stats)
    sc, mean, var = norm.ensemble_scores(inp, tgt, frc, num_members=M, rngs=5, fields=True)
    assert isinstance(mean, Dataset) and isinstance(var, Dataset)
    # The members in float64 physical units: x -> a x + last input frame, from the normalised float32 members the
    # sampler returns for the same seeds; the truth the device saw, mapped the same way.  Every target is an input.
    assert set(tgt.keys()) <= set(inp.keys())
    _, ni, nt, nf = norm._normalized_loss_args(inp, tgt, frc)
    ens = EnsembleSampler(gc._sampler, base_seed=5)
    members_n = [_stack(d) for _, d in sorted(ens(ni, nt.map(np.zeros_like), nf, M), key=lambda t: t[0])]
    a = np.concatenate([rollout._per_channel_stat(stats[2], name, tgt[name], 1.0) for name, _, _ in datasets.channel_layout(tgt)])
    last = _stack(Dataset({k: Variable(v.dims, np.broadcast_to(np.take(inp[k].data, [-1], axis=inp[k].dims.index("time")), v.data.shape))
                           for k, v in tgt.items()}, tgt.coords)).astype(np.float64)
    phys = np.stack([a * x.astype(np.float64) + last for x in members_n])
    truth_phys = a * _stack(nt).astype(np.float64) + last
    w = verification.node_weights(tgt).astype(np.float64)[:, None, None]
    # float64 definition on float64 inputs (the reference proper takes float32): the same loops
    m = sum(phys[i] for i in range(M)) / M
    e = m - truth_phys
    s2 = sum((phys[i] - m) ** 2 for i in range(M)) / (M - 1)
    ae = sum(np.abs(phys[i] - truth_phys) for i in range(M)) / M
    d = R.pair_sum_brute(phys) / (M * (M - 1) / 2)
    terms = [w * np.ones_like(e), w * e, w * e * e, w * s2, w * ae, w * d]
    G = phys.shape[1]
    vmax = max(np.abs(phys).max(), np.abs(truth_phys).max())
    ev = 4 * 2.0 ** -53 * vmax                                     # what the affine map in float64 adds to one value
    for k, name in enumerate(R.SUM_NAMES):
      want, A = terms[k].sum(0), np.abs(terms[k]).sum(0)
      S0 = terms[0].sum(0)
      # the (G + M^2 + 8) 2^-53 A_k of the device sum, carried through scaled(); plus the map's own rounding: 2 ev per
      # difference of two values in the linear sums, 2 |e| 2 ev per square (Cauchy-Schwarz: sum w |e| <= sqrt(S0 S_k))
      extra = {0: 0.0, 1: 2 * ev * S0, 4: 2 * ev * S0, 5: 2 * ev * S0}.get(k)
      if extra is None:
        extra = 4 * ev * np.sqrt(S0 * want) * (2 if k == 3 else 1) + 4 * ev * ev * S0
      tol = (G + M * M + 8 + 4) * 2.0 ** -53 * A + extra
      err = np.abs(sc.sums[..., k] - want)
      print(f"dataset {name}: worst ratio {np.max(err / tol):.3f}")
      assert np.all(err <= tol), name
    # fields: float32 un-normalisation of float32 fields against the float64 values
    np.testing.assert_allclose(_stack(mean), m, rtol=0, atol=8 * 2.0 ** -24 * vmax)
    np.testing.assert_allclose(_stack(var), s2, rtol=4 * 2.0 ** -24, atol=16 * 2.0 ** -53 * vmax * vmax)
    pv = sc.per_variable(tgt)
    assert pv["crps"]["temperature"].shape == (2, 13) and (pv["crps"]["temperature"] > 0).all()
    # xarray in, xarray out for the fields
    to_x = lambda ds: fake_xarray.Dataset({k: (v.dims, v.data) for k, v in ds.items()},
                                          coords={k: v for k, v in ds.coords.items() if k in ("lat", "lon")})
    _, xmean, _ = norm.ensemble_scores(to_x(inp), to_x(tgt), to_x(frc), num_members=M, rngs=5, fields=True)
    assert isinstance(xmean, fake_xarray.Dataset)
    np.testing.assert_array_equal(xmean["2m_temperature"].values, mean["2m_temperature"].data)
    # NaNCleaner: NaN truth over a "land mask" -- the device skips those points, the inputs are cleaned
    k = "2m_temperature"
    land = np.zeros((13, 24), bool)
    land[2:6, 3:11] = True
    dirty_t = tgt.assign(Dataset({k: Variable(tgt[k].dims, np.where(land, np.nan, tgt[k].data).astype(np.float32))}))
    dirty_i = inp.assign(Dataset({k: Variable(inp[k].dims, np.where(land, np.nan, inp[k].data).astype(np.float32))}))
    fill = Dataset({k: Variable((), np.float32(0.25))})
    nc = NaNCleaner(gc, k, fill)
    got = nc.ensemble_scores(dirty_i, dirty_t, frc, num_members=M, rngs=5)
    clean_i = inp.assign(Dataset({k: Variable(inp[k].dims, np.where(land, np.float32(0.25), inp[k].data).astype(np.float32))}))
    members = [_stack(dd) for _, dd in sorted(ens(clean_i, tgt.map(np.zeros_like), frc, M), key=lambda t: t[0])]
    ref = R.reference(np.stack(members), _stack(dirty_t), verification.node_weights(tgt))
    _check_sums("nan cleaner", got.sums, got.rank_histogram, ref, G, M)
    off = {name: o for name, o, _ in datasets.channel_layout(tgt)}[k]
    np.testing.assert_array_equal(got.valid_points[:, off], np.full(2, 13 * 24 - land.sum(), np.uint64))
    assert gc.denoiser.native.counter("ens_invalid_points") == 2 * land.sum()
    assert np.isfinite(got.crps).all()
  finally:
    gc.denoiser.native.close()


# ---- 7. errors --------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w = _data(3, G, B, C, seed=41)
  nd = _handle(gr, B, C)
  other = _handle(gr, 1, C)
  full = None
  try:
    for bad in (1, 65, 0, -3):
      with pytest.raises(ValueError, match="2..64"):
        nd.ens_reserve(bad)
    with pytest.raises(_lib.GencastHipError):                      # nothing reserved
      nd.ens_score(truth)
    nd.ens_reserve(3)
    for i in (0, 1):
      nd.ens_push_host(i, members[i])
    nd.ens_set_node_weight(w)
    with pytest.raises(_lib.GencastHipError, match="slot 2"):      # an unfilled slot
      nd.ens_score(truth)
    for slot in (-1, 3):
      with pytest.raises(ValueError, match="slot"):
        nd.ens_push_host(slot, members[0])
    with pytest.raises(ValueError):
      nd.ens_push_host(0, members[0][:, :1])
    nd.ens_push_host(2, members[2])
    with pytest.raises(_lib.GencastHipError, match="truth"):       # no truth yet
      nd.ens_score(None)
    with pytest.raises(_lib.GencastHipError, match="fields"):      # fields never computed
      nd.ens_score(truth)
      nd.ens_download_fields()
    with pytest.raises(ValueError, match="dimensions"):            # a source with another batch size
      nd.ens_push(0, src=other)
    with pytest.raises(_lib.GencastHipError, match="sample"):      # a source without a sample
      nd.ens_push(0)
    nd.ens_score(truth, want_fields=True)
    nd.ens_download_fields()
    nd.ens_reserve(3)                                              # empties the store, and the fields with it
    with pytest.raises(_lib.GencastHipError, match="fields"):
      nd.ens_download_fields()
    with pytest.raises(_lib.GencastHipError, match="slot 0"):
      nd.ens_score(truth)
    # scoring before the weights are set
    full = _handle(gr, B, C)
    full.ens_reserve(2)
    full.ens_push_host(0, members[0])
    full.ens_push_host(1, members[1])
    with pytest.raises(_lib.GencastHipError, match="node weights"):
      full.ens_score(truth)
    with pytest.raises(ValueError):
      full.ens_set_node_weight(w[:-1])
  finally:
    nd.close()
    other.close()
    if full is not None:
      full.close()


# ---- the truth of the store: uploaded by one scorer, used by all ----------------------------------------------------------
def test_truth_uploaded_by_one_scorer_is_the_truth_of_the_others():
  """gc_ens_score, gc_ens_spectrum and gc_ens_event_score take the truth through one path into one buffer: whichever of
  them uploads it, the other two given None score against it, bit for bit as if it had been passed to them; a truth that
  gc_ens_derive uploads goes into the SOURCE handle's buffer and is there for the source's own scorers."""
  from gencast_flax_nnx_amd import SphericalAnalysis
  from gencast_flax_nnx_amd.verification import quantize_node_weights
  gr = _graph()
  G, B, C, M, T, lmax = gr.num_grid_nodes, 2, 3, 3, 2, 6
  members, truth, w = _data(M, G, B, C, seed=31, scale=np.ones(C))
  rng = np.random.default_rng(32)
  thr = rng.standard_normal((T, G, B, C)).astype(np.float32)
  wq, _ = quantize_node_weights(w)
  tabs = SphericalAnalysis(np.linspace(-90, 90, 13), np.arange(24) * 15.0, lmax=lmax).device_tables()

  def fresh():
    nd = _handle(gr, B, C)
    _push_all(nd, members, w)
    nd.spec_set_tables(*tabs)
    nd.ens_event_set(thr, [1, -1], wq)
    return nd

  scorers = {"score": lambda nd, t: nd.ens_score(t), "spectrum": lambda nd, t: (nd.ens_spectrum(t),),
             "events": lambda nd, t: nd.ens_event_score(t)}
  nd = fresh()
  try:
    explicit = {name: f(nd, truth) for name, f in scorers.items()}
  finally:
    nd.close()
  assert all(np.isfinite(a).all() for a in explicit["score"][:1] + explicit["spectrum"])

  def same(tag, got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
      assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"{tag}: output {i} differs"

  for uploader in scorers:
    nd = fresh()
    try:
      for name, f in scorers.items():
        if name != uploader:
          with pytest.raises(_lib.GencastHipError, match="truth"):   # nothing uploaded yet
            f(nd, None)
      same(f"{uploader} uploads", scorers[uploader](nd, truth), explicit[uploader])
      for name, f in scorers.items():
        same(f"{uploader} uploaded, {name} given None", f(nd, None), explicit[name])
    finally:
      nd.close()

  src, view = fresh(), _handle(gr, B, 2)
  try:
    view.ens_derive_set(c_src=C, op=[0, 1], src_a=[0, 1], src_b=[0, 2], affine=np.tile([1.0, 0.0, 1.0, 0.0], (2, 1)),
                        n_lat=13, n_lon=24)
    view.ens_reserve(M)
    with pytest.raises(_lib.GencastHipError, match="no truth on the source handle"):
      view.ens_derive(src)
    view.ens_derive(src, truth)
    same("derive uploaded, source score given None", src.ens_score(None), explicit["score"])
    same("derive uploaded, source score given the truth", src.ens_score(truth), explicit["score"])
  finally:
    view.close()
    src.close()
