"""The edge-term route of the sampler ("edge terms") on the GPU.

Inside a sample the first layer of the two edge MLPs is `T(sigma)[e] + P_snd[snd] + P_rcv[rcv] + b1`: T (the conditioned
static edge embedding times the edge block of W1), the conditioned mesh embedding m0 and its product with the grid2mesh
receiver block are made once per noise-level list; the other node products are one GEMM per node set and call.
GC_TUNE_EDGE_TERMS=0 is the route with the K = 768 product in the edge kernels.

Bounds: the ones tests/test_gpu_parity.py applies to the same quantities (test_tiny_every_stage_matches_oracle): 5e-5 for
e1 / g1 / y, 5e-5 x max(1, max |reference|) for the aggregates agg1 / agg2 (sums of up to 60 unit-scale rows).

Shapes.  BIG (61 x 132 grid, mesh 3, latent 256): E1 = 12 822 grid2mesh rows (not a multiple of 32; below 24 000, so the
edge update pairs with the grid-node update in one launch: both halves), E2 = 24 156 mesh2grid rows (from 24 000 rows on
the 64-row form: 21 triples per tile, the last tile holds 9).  SMALL (19 x 36 grid): the 32-row forms, 10 triples per
tile.  Batch 2 keeps the route with the products (the cache is built for batch 1), which is checked."""
import dataclasses

import numpy as np
import pytest

from oracle import gencast_oracle as O
from tests import helpers

pytestmark = pytest.mark.gpu

SIG = O.noise_schedule(80.0, 0.03, 2, 7.0)          # 2 steps: 3 denoiser calls at 3 distinct noise levels
SIG_OTHER = O.noise_schedule(40.0, 0.05, 2, 7.0)
SIG_ONE_CALL = np.array([80.0, 0.0])                # 1 step whose mid-point call is dead: 1 denoiser call
STAGES = ("e1", "g1", "agg1", "agg2", "y")
LATENT = 256


def _setup(batch, n_lat, n_lon, seed=13):
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=batch, seed=seed, latent=LATENT, heads=4, ffw=256, layers=1, mesh_size=3,
                                                  k_hop=2, n_lat=n_lat, n_lon=n_lon)
  noise = np.random.default_rng(5).standard_normal((gr.num_grid_nodes, batch, dims.c_out)).astype(np.float32)
  slots = np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32)
  return dict(gr=gr, dims=dims, params=params, x=x, sigma=sigma, noise=noise, slots=slots, batch=batch)


@pytest.fixture(scope="module")
def big():
  s = _setup(1, 61, 132)
  gr = s["gr"]
  E1, E2, G = len(gr.g2m_senders), len(gr.m2g_senders), gr.num_grid_nodes
  assert E1 % 32 != 0 and E1 < 24000 and G < 24000      # a partly filled last 32-row tile; the pair launch has both halves
  assert E2 == 3 * G and E2 >= 24000 and G % 21 != 0    # 64-row tiles of 21 triples, the last one partly filled
  return s


@pytest.fixture(scope="module")
def small():
  return _setup(1, 19, 36)


@pytest.fixture(scope="module")
def small_b2():
  return _setup(2, 19, 36)


def _native(monkeypatch, s, switch, gr=None, options=()):
  monkeypatch.setenv("GC_TUNE_EDGE_TERMS", switch)
  nd = helpers.make_native(gr if gr is not None else s["gr"], s["dims"], s["params"], s["batch"])
  for k, v in options:
    nd.set_option(k, v)
  nd.set_noisy_slots(s["slots"])
  return nd


def _sample(nd, s, sig=SIG, x=None, noise=None):
  out, st = nd.sample(s["x"] if x is None else x, s["noise"] if noise is None else noise, sig)
  assert st["denoiser_calls"] == 2 * (len(sig) - 1) - 1
  return out


def _fetch(nd):
  return {k: nd.debug_fetch(k) for k in STAGES}


def _within_bound(got, ref, what):
  for k in STAGES:
    a, r = got[k], ref[k].reshape(got[k].shape)
    scale = max(1.0, np.abs(r).max()) if k.startswith("agg") else 1.0
    err = np.abs(a - r).max() / scale
    print(f"{what}: {k} max err {err:.3e}")
    assert err < 5e-5, (what, k, err)


def _last_call_oracle(s, sig):
  """The oracle's sample, and its intermediates of the last denoiser call (the buffers gc_debug_fetch reads afterwards)."""
  gr, dims, params = s["gr"], s["dims"], s["params"]
  calls = []
  def net(f, sg):
    calls.append((f, sg))
    return O.denoiser_forward(params, helpers.graph_dict(gr), f, sg, num_layers=dims.num_layers, num_heads=dims.num_heads,
                              attention="neighbour")
  ref, n = O.dpm_solver_2s_sample(net, s["x"].astype(np.float64), s["slots"], s["noise"].astype(np.float64), sig, skip_dead_call=True)
  y, inter = O.denoiser_forward(params, helpers.graph_dict(gr), calls[-1][0], calls[-1][1], num_layers=dims.num_layers,
                                num_heads=dims.num_heads, attention="neighbour", return_intermediates=True)
  inter = dict(inter, y=y)
  return ref, {k: np.asarray(inter[k]) for k in STAGES}


@pytest.mark.parametrize("size", ["big", "small"])
def test_route_agrees_with_the_products_and_with_the_oracle(size, big, small, monkeypatch):
  """(a) Batch 1, inside a sample: every stage the two edge updates feed, route against GC_TUNE_EDGE_TERMS=0 and against
  the oracle, within the parity bound; two launches more per call (three node GEMMs, no affine pass); the cache holds one
  slot per noise level."""
  s = big if size == "big" else small
  gr, L = s["gr"], LATENT
  res = {}
  for switch in ("1", "0"):
    nd = _native(monkeypatch, s, switch)
    try:
      out = _sample(nd, s)
      res[switch] = (out, _fetch(nd), nd.counter("edge_term_samples"), nd.counter("edge_term_cache_bytes"),
                     nd.counter("launches_per_call"), nd.debug_fetch("m0"))
    finally:
      nd.close()
  assert res["1"][2] == 1 and res["0"][2] == 0
  per_slot = (len(gr.g2m_senders) + len(gr.m2g_senders) + 2 * gr.num_mesh_nodes) * L * 4
  assert res["1"][3] == 3 * per_slot and res["0"][3] == 0
  assert res["1"][4] == res["0"][4] + 2
  np.testing.assert_array_equal(res["1"][5], res["0"][5])              # m0 of the slot = m0 of the call's affine pass
  _within_bound(res["1"][1], res["0"][1], f"{size}: terms vs products")
  ref, inter = _last_call_oracle(s, SIG)
  _within_bound(res["1"][1], inter, f"{size}: terms vs oracle")
  scale = max(1.0, np.abs(ref).max())
  assert np.abs(res["1"][0] - ref).max() < 1e-4 * scale
  assert np.abs(res["1"][0] - res["0"][0]).max() < 5e-5 * scale


def test_batch_two_keeps_the_products(small_b2, monkeypatch):
  """(a) Batch 2: the cache is built for batch 1 only, so the switch changes nothing -- bit for bit, and no sample counts."""
  s = small_b2
  res = {}
  for switch in ("1", "0"):
    nd = _native(monkeypatch, s, switch)
    try:
      out = _sample(nd, s)
      res[switch] = (out, _fetch(nd))
      assert nd.counter("edge_term_samples") == 0 and nd.counter("edge_term_cache_bytes") == 0
    finally:
      nd.close()
  np.testing.assert_array_equal(res["1"][0], res["0"][0])
  for k in STAGES:
    np.testing.assert_array_equal(res["1"][1][k], res["0"][1][k])
  ref, _ = _last_call_oracle(s, SIG)
  assert np.abs(res["1"][0] - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())


def test_outside_a_sample_and_with_fp16_features_the_route_does_not_engage(small, monkeypatch):
  """(b) gc_denoise -- before and after a sample that built the cache -- and a sample with fp16 features: switch on against
  switch off, bit for bit; `edge_term_samples` counts only the float32-feature sample in between."""
  s = small
  res = {}
  for switch in ("1", "0"):
    nd = _native(monkeypatch, s, switch)
    try:
      y0 = nd.denoise(s["x"], s["sigma"])
      st0 = _fetch(nd)
      assert nd.counter("edge_term_samples") == 0
      _sample(nd, s)
      assert nd.counter("edge_term_samples") == int(switch)
      y1 = nd.denoise(s["x"], s["sigma"])                               # the cache is live now: still the one-call form
      st1 = _fetch(nd)
      nd.set_option("features", "f16")
      assert nd.counter("edge_term_cache_bytes") == 0                   # the static embeddings were made again
      out16 = _sample(nd, s)
      assert nd.counter("edge_term_samples") == int(switch)
      res[switch] = (y0, st0, y1, st1, out16)
    finally:
      nd.close()
  np.testing.assert_array_equal(res["1"][0], res["1"][2])
  for a, b in ((0, 0), (2, 2), (4, 4)):
    np.testing.assert_array_equal(res["1"][a], res["0"][b])
  for i in (1, 3):
    for k in STAGES:
      np.testing.assert_array_equal(res["1"][i][k], res["0"][i][k])


def test_cache_is_reused_rebuilt_for_another_list_and_after_a_reload(small, monkeypatch):
  """(c) The second sample of a noise-level list is served from the cache (and, captured, from the graph) bit for bit; another
  list replaces the cache and coming back rebuilds the same terms; so does reloading the weights."""
  s = small
  nd = _native(monkeypatch, s, "1")
  try:
    first = _sample(nd, s)
    bytes1 = nd.counter("edge_term_cache_bytes")
    assert bytes1 > 0 and nd.counter("edge_term_samples") == 1
    for n in (2, 3):                                                   # the second is captured, the third replayed
      np.testing.assert_array_equal(_sample(nd, s), first)
      assert nd.counter("edge_term_samples") == n
    assert nd.counter("graph_replays") >= 1
    other = _sample(nd, s, SIG_OTHER)
    assert nd.counter("edge_term_samples") == 4 and nd.counter("edge_term_cache_bytes") == bytes1
    assert np.abs(other - first).max() > 1e-3
    np.testing.assert_array_equal(_sample(nd, s), first)               # rebuilt for the first list: the same terms
    np.testing.assert_array_equal(_sample(nd, s, SIG_OTHER), other)
    assert nd.counter("edge_term_samples") == 6
    nd.load_weights(s["params"])
    nd.finalize()
    assert nd.counter("edge_term_cache_bytes") == 0                    # dropped with the weights it was made from
    nd.set_noisy_slots(s["slots"])
    np.testing.assert_array_equal(_sample(nd, s), first)
    assert nd.counter("edge_term_cache_bytes") == bytes1 and nd.counter("edge_term_samples") == 7
  finally:
    nd.close()
  nd = _native(monkeypatch, s, "0")
  try:
    ref = _sample(nd, s, SIG_OTHER)
  finally:
    nd.close()
  assert np.abs(other - ref).max() < 5e-5 * max(1.0, np.abs(ref).max())


def test_a_cap_below_the_cache_size_keeps_the_products(small, monkeypatch):
  """(d) A 1 MiB cap (the cache needs 3 slots of about 4 MB here): the route with the products, bit for bit; raising the cap
  afterwards lets the next sample build it."""
  s = small
  nd0 = _native(monkeypatch, s, "0")
  try:
    ref = _sample(nd0, s)
    ref_st = _fetch(nd0)
  finally:
    nd0.close()
  nd = _native(monkeypatch, s, "1", options=(("edge_term_cache_mb", "1"),))
  try:
    np.testing.assert_array_equal(_sample(nd, s), ref)
    st = _fetch(nd)
    for k in STAGES:
      np.testing.assert_array_equal(st[k], ref_st[k])
    np.testing.assert_array_equal(_sample(nd, s), ref)                 # (captured)
    assert nd.counter("edge_term_samples") == 0 and nd.counter("edge_term_cache_bytes") == 0
    nd.set_option("edge_term_cache_mb", "4096")
    out = _sample(nd, s)
    assert nd.counter("edge_term_samples") == 1 and nd.counter("edge_term_cache_bytes") > (1 << 20)
    assert np.abs(out - ref).max() < 5e-5 * max(1.0, np.abs(ref).max())
    with pytest.raises(Exception):
      nd.set_option("edge_term_cache_mb", "lots")
  finally:
    nd.close()


def test_an_input_that_trips_the_domain_guard_gives_the_exact_f32_result(small, monkeypatch):
  """(e) A conditioning channel beyond fp16 range poisons the f16x3 sample; the re-run on the exact-f32 kernels takes the
  route with the products whatever the switch says: bit for bit the switch-off result.  The cache survives the re-run."""
  s = small
  huge = s["x"].copy()
  huge[:, :, 3] *= 2.0e5
  res = {}
  for switch in ("1", "0"):
    nd = _native(monkeypatch, s, switch)
    try:
      out = _sample(nd, s, x=huge)
      assert nd.counter("range_fallbacks") == 1 and np.isfinite(out).all()
      res[switch] = (out, nd.counter("edge_term_cache_bytes"))
    finally:
      nd.close()
  np.testing.assert_array_equal(res["1"][0], res["0"][0])
  assert res["1"][1] > 0 and res["0"][1] == 0


@pytest.mark.parametrize("size", ["big", "small"])
def test_a_rows_result_does_not_depend_on_where_it_sits_in_the_tile(size, big, small, monkeypatch):
  """(f) The method of test_gpu_parity.test_a_rows_result_does_not_depend_on_where_it_sits_in_the_launch on the first layer
  without a product: rolling the grid nodes by 5 and by 32 moves every grid node's triple of mesh2grid rows by 15 and 96
  rows (another place in its 63- or 30-row tile, another wave), and rolling the grid2mesh edge list moves every updated
  edge inside its 32-row tile; e1 and agg2 must come back bit for bit.  (The edge list is rolled in a handle of its own
  that samples with ONE denoiser call: the roll changes the order of the grid2mesh segment sums by an ulp, and with them
  everything behind them -- the mesh2grid inputs, and the state every later call of a sample starts from.)"""
  s = big if size == "big" else small
  gr = s["gr"]
  G, E1 = gr.num_grid_nodes, len(gr.g2m_senders)
  res = {}
  for shift in (0, 5, 32):
    idx = np.roll(np.arange(G), shift)                   # new grid node i = old node idx[i]
    inv = np.argsort(idx)
    eidx = np.roll(np.arange(E1), shift)
    nodes = dataclasses.replace(gr, grid_struct=gr.grid_struct[idx], g2m_senders=inv[gr.g2m_senders].astype(gr.g2m_senders.dtype),
                                m2g_receivers=inv[gr.m2g_receivers].astype(gr.m2g_receivers.dtype))
    edges = dataclasses.replace(nodes, g2m_senders=nodes.g2m_senders[eidx], g2m_receivers=nodes.g2m_receivers[eidx],
                                g2m_edge_struct=nodes.g2m_edge_struct[eidx])
    got = {}
    for name, g2 in (("nodes", nodes), ("edges", edges)):
      nd = _native(monkeypatch, s, "1", gr=g2)
      try:
        _sample(nd, s, SIG if name == "nodes" else SIG_ONE_CALL, x=s["x"][idx], noise=s["noise"][idx])
        assert nd.counter("edge_term_samples") == 1 and nd.counter("m2g_fused_sum") == 1
        e1 = nd.debug_fetch("e1").reshape(E1, -1)
        got[name] = (e1[np.argsort(eidx)] if name == "edges" else e1, nd.debug_fetch("agg2").reshape(G, -1)[inv])
      finally:
        nd.close()
    res[shift] = (got["nodes"][0], got["nodes"][1], got["edges"][0])
  for shift in (5, 32):
    for a, b in zip(res[shift], res[0]):
      np.testing.assert_array_equal(a, b)
