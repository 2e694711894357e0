"""Multivariate ensemble scores on the device (gc_ens_energy_*, gc_ens_variogram_*) against the float64
definition restated in tests/multivar_reference.py.

Energy: omega (d d) is the same three rounded double operations on both sides and d is exact, so only the order of the
n = G |group| additions differs: |device - reference| <= (n + 8) 2^-53 sum |term| (`multivar_reference.energy_tolerance`),
derived, not measured.  The node weights and the scales of the tests are dyadic, so S0 must EQUAL the reference.
Variogram: |device - reference| <= (G + M + 8) 2^-53 sum |term|; counts are integers: ==.

Sizes: the 13 x 24 grid (G = 312) with handles that know their graph only.  M in {2, 3, 8, 33, 50, 64} gives P = 3, 6, 36,
561, 1 275 and 2 080 pairs: fewer than one pair per thread (the spare threads take slices of a tile), P no multiple of 256,
and more than 8 pairs per thread.  (B, C) = (2, 6) with groups {0, 1}, {2, 3, 4} and channel 5 in none; (4, 82) with one
group over all channels and with 32 groups of interleaved channels.  Every case has more than one node-range block and a
last tile that is not full; most have only that one tile per workgroup (a block's points number at most 234).  The cases
with one group over 82 channels give a workgroup 328 points, a full tile and a partial one: at (4, 82) with M = 8 for the
sliced instance, at (1, 82) with M in {33, 50, 64} for the instances with 3 and 9 pairs per thread."""
import ctypes

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, verification
from gencast_flax_nnx_amd.verification import EnergyScores, VariogramScores
from tests import multivar_reference as R
from tests.helpers import graph_handle as _handle, small_graph as _graph

pytestmark = pytest.mark.gpu

N_LAT, N_LON = 13, 24
GROUP6 = np.array([0, 0, 1, 1, 1, -1], np.int32)
SCALE6 = np.array([1.0, 0.5, 2.0, 1.0, 0.25, 3.0])
OFFSETS = [(0, 1), (1, 0), (0, -5), (12, 0), (-3, 23)]


def _data(M, G, B, C, seed):
  """Members and truth of mixed magnitudes; node weights that are multiples of 1/8."""
  rng = np.random.default_rng(seed)
  scale = np.logspace(-2, 3, C)
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  w = (rng.integers(1, 17, G) / 8.0).astype(np.float32)
  return members, truth, w


def _push_all(nd, members, w=None):
  nd.ens_reserve(len(members))
  if w is not None:
    nd.ens_set_node_weight(w)
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _check_energy(tag, out, ref):
  d2, s0, invalid = out
  assert d2.shape == ref["d2"].shape and d2.dtype == np.float64 and s0.shape == ref["s0"].shape, f"{tag}: {d2.shape} {s0.shape}"
  tol = R.energy_tolerance(ref)
  err = np.abs(d2 - ref["d2"])
  ratio = float(np.max(err / np.maximum(tol, 1e-300)))
  print(f"{tag} D2: max |device - reference| {err.max():.3e}, worst ratio to (n + 8) 2^-53 sum|term| {ratio:.3f}")
  assert np.all(err <= tol), f"{tag}: D2 outside (n + 8) 2^-53 sum|term|"
  np.testing.assert_array_equal(s0, ref["s0"], err_msg=f"{tag}: S0 (dyadic weights and scales)")
  assert invalid == ref["invalid"], f"{tag}: invalid"


def _check_variogram(tag, out, ref, G, M):
  sums, counts = out
  assert sums.shape == ref["sums"].shape and sums.dtype == np.float64 and counts.dtype == np.uint64, f"{tag}: {sums.shape}"
  tol = R.variogram_tolerance(ref, G, M)
  err = np.abs(sums - ref["sums"])
  ratio = float(np.max(err / np.maximum(tol, 1e-300)))
  print(f"{tag}: max |device - reference| {err.max():.3e}, worst ratio to (G + M + 8) 2^-53 sum|term| {ratio:.3f}")
  assert np.all(err <= tol), f"{tag}: sums outside (G + M + 8) 2^-53 sum|term|"
  np.testing.assert_array_equal(counts, ref["counts"], err_msg=f"{tag}: counts")


# ---- 1. every M, and what a call leaves alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 8, 33, 50, 64])
def test_energy_every_member_count_matches_the_float64_definition(M):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w = _data(M, G, B, C, seed=M)
  ref = R.energy(members, truth, w, GROUP6, SCALE6)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_energy_set(2, GROUP6, SCALE6)
    before = nd.ens_score(truth)
    out = nd.ens_energy_score(None)                       # (the truth ens_score uploaded)
    assert out[0].shape == (B, 2, M * (M + 1) // 2) and out[1].shape == (B, 2)
    _check_energy(f"tiny M={M}", out, ref)
    assert nd.counter("ens_energy_invalid_points") == 0 and nd.counter("ens_energy_calls") == 1
    again = nd.ens_energy_score(None)
    assert again[0].tobytes() == out[0].tobytes() and again[1].tobytes() == out[1].tobytes() and again[2] == out[2]
    for i in range(M):                                    # the store is read, never written
      assert nd.ens_download_member(i).tobytes() == members[i].tobytes()
    after = nd.ens_score(None)
    for x, y in zip(before, after):
      assert x.tobytes() == y.tobytes()
    sc = EnergyScores.from_sums(out[0], out[1], M, ("a", "b"))
    want = R.energy_scores(ref["d2"], ref["s0"], M)
    np.testing.assert_allclose(sc.per_forecast, want["fair"], rtol=1e-9, atol=0.0)
    np.testing.assert_allclose(sc.per_forecast_ensemble, want["ensemble"], rtol=1e-9, atol=0.0)
  finally:
    nd.close()


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M", [(1, 8), (32, 33)])
def test_energy_many_channels(K, M):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 4, 82
  members, truth, w = _data(M, G, B, C, seed=100 + K)
  if K == 1:
    group = np.zeros(C, np.int32)
  else:
    group = (np.arange(C) % 32).astype(np.int32)          # interleaved channels; the last two in no group
    group[80:] = -1
  scale = 2.0 ** np.random.default_rng(5).integers(-3, 4, C)
  ref = R.energy(members, truth, w, group, scale)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_energy_set(K, group, scale)
    _check_energy(f"C=82 K={K} M={M}", nd.ens_energy_score(truth), ref)
  finally:
    nd.close()


@pytest.mark.parametrize("M", [33, 50, 64])
def test_energy_more_than_one_tile_per_workgroup(M):
  """One group over 82 channels: 100 node ranges of 4 nodes, 328 points each -- the tile loop runs twice (the LDS tile is
  reused behind the barrier, the second tile is partial) in the instances with 3 and 9 pairs per thread.  Some points are
  invalid in each tile."""
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 1, 82
  members, truth, w = _data(M, G, B, C, seed=200 + M)
  truth[::7, 0, 3] = np.nan                               # invalid points in both tiles of a block
  members[M // 2, 5::11, 0, 80] = np.inf
  group, scale = np.zeros(C, np.int32), 2.0 ** np.random.default_rng(6).integers(-3, 4, C)
  ref = R.energy(members, truth, w, group, scale)
  assert ref["invalid"] == len(range(0, G, 7)) + len(range(5, G, 11))
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_energy_set(1, group, scale)
    out = nd.ens_energy_score(truth)
    _check_energy(f"two tiles M={M}", out, ref)
    again = nd.ens_energy_score(None)
    assert again[0].tobytes() == out[0].tobytes() and again[1].tobytes() == out[1].tobytes()
  finally:
    nd.close()


# ---- 3. invalid points ----------------------------------------------------------------------------------------------------------
def test_energy_invalid_points_are_skipped():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w = _data(M, G, B, C, seed=31)
  group = np.array([0, 0, 1, 2, 2, -1], np.int32)
  truth[40:75, 1, 0:2] = np.nan                           # a block of the truth
  members[3, 100, 0, 3] = np.nan                          # single members
  members[5, 101, 0, 4] = np.inf
  members[0, 311, 1, 4] = -np.inf                         # (the last node)
  members[2, 7, 0, 5] = np.nan                            # a channel in no group: not counted anywhere
  truth[:, :, 2] = np.nan                                 # group 1 is invalid everywhere
  ref = R.energy(members, truth, w, group, SCALE6)
  assert ref["invalid"] == 35 * 2 + 3 + G * B
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_energy_set(3, group, SCALE6)
    d2, s0, invalid = nd.ens_energy_score(truth)
    _check_energy("invalid points", (d2, s0, invalid), ref)
    assert invalid == nd.counter("ens_energy_invalid_points")
    assert np.all(s0[:, 1] == 0.0) and np.all(d2[:, 1] == 0.0) and np.all(np.isfinite(d2))
    sc = EnergyScores.from_sums(d2, s0, M)
    assert np.all(np.isnan(sc.per_forecast[:, 1])) and np.all(np.isfinite(sc.per_forecast[:, [0, 2]]))
  finally:
    nd.close()


# ---- 4. variogram ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.5, 1.0, 2.0])
def test_variogram_every_offset_and_order(p):
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w = _data(M, G, B, C, seed=41)
  truth[50:60, 1, 2] = np.nan
  members[4, 0, 0, 1] = np.inf                            # a corner: partner of wrapped and of clipped pairs
  members[1, 311, 1, 5] = np.nan
  ref = R.variogram(members, truth, w, N_LAT, N_LON, OFFSETS, p)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_variogram_set(N_LAT, N_LON, OFFSETS, p)
    before = nd.ens_score(truth)
    out = nd.ens_variogram_score(None)
    assert out[0].shape == (4, B, C, len(OFFSETS)) and out[1].shape == (B, C, len(OFFSETS))
    _check_variogram(f"tiny p={p}", out, ref, G, M)
    again = nd.ens_variogram_score(None)
    assert again[0].tobytes() == out[0].tobytes() and again[1].tobytes() == out[1].tobytes()
    for i in range(M):
      assert nd.ens_download_member(i).tobytes() == members[i].tobytes()
    after = nd.ens_score(None)
    for x, y in zip(before, after):
      assert x.tobytes() == y.tobytes()
    assert nd.counter("ens_variogram_calls") == 2
  finally:
    nd.close()


def test_variogram_more_columns_than_one_tile():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 4, 82, 3
  members, truth, w = _data(M, G, B, C, seed=43)
  ref = R.variogram(members, truth, w, N_LAT, N_LON, OFFSETS, 0.5)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_variogram_set(N_LAT, N_LON, OFFSETS, 0.5)
    _check_variogram("W=328", nd.ens_variogram_score(truth), ref, G, M)
  finally:
    nd.close()


def test_variogram_a_second_column_tile_of_one_column():
  """(B, C) = (1, 257): the second column tile is one column wide, 256 node lanes for the 8 nodes of a block."""
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 1, 257, 3
  members, truth, w = _data(M, G, B, C, seed=257)
  ref = R.variogram(members, truth, w, N_LAT, N_LON, OFFSETS, 1.0)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_variogram_set(N_LAT, N_LON, OFFSETS, 1.0)
    _check_variogram("W=257", nd.ens_variogram_score(truth), ref, G, M)
  finally:
    nd.close()


def test_variogram_wraps_in_longitude_and_clips_in_latitude():
  """The truth is 1 in row 0 and in column 0 and 0 elsewhere, the members are 0: vx = 0 and vy = 1 exactly where one end of a
  pair lies on the cross, so V3 counts those pairs with their weights -- w = (row + 1) / 8 is dyadic and every expected
  value below is exact."""
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 1, 1, 2
  y = np.zeros((N_LAT, N_LON), np.float32)
  y[0, :] = 1.0
  y[:, 0] = 1.0
  truth = y.reshape(G, 1, 1)
  members = np.zeros((M, G, B, C), np.float32)
  wr = (np.arange(N_LAT) + 1) / 8.0
  w = np.repeat(wr, N_LON).astype(np.float32)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_variogram_set(N_LAT, N_LON, OFFSETS, 1.0)
    sums, counts = nd.ens_variogram_score(truth)
    _check_variogram("cross", (sums, counts), R.variogram(members, truth, w, N_LAT, N_LON, OFFSETS, 1.0), G, M)
    V0, V1, V2, V3 = (sums[k, 0, 0] for k in range(4))
    n = counts[0, 0]
    # (0, 1): every point has a partner; in each row below the first, column 0 differs from column 1 and -- through the
    # wrap -- column n_lon - 1 from column 0
    assert n[0] == G and V3[0] == 2.0 * wr[1:].sum() and V0[0] == N_LON * wr.sum()
    # (1, 0): the last row has no partner; row 0 differs from row 1 everywhere but in column 0
    assert n[1] == (N_LAT - 1) * N_LON and V3[1] == (N_LON - 1) * 0.5 * (wr[0] + wr[1])
    assert V0[1] == N_LON * 0.5 * (wr[:-1] + wr[1:]).sum()
    # (0, -5): a wrap to the left: column 0 against column n_lon - 5, column 5 against column 0
    assert n[2] == G and V3[2] == 2.0 * wr[1:].sum()
    # (12, 0): only row 0 has a partner, the last row
    assert n[3] == N_LON and V3[3] == (N_LON - 1) * 0.5 * (wr[0] + wr[12]) and V0[3] == N_LON * 0.5 * (wr[0] + wr[12])
    # (-3, 23): rows 3 .. 12 pair with rows 0 .. 9, one column to the left; row 3 meets row 0, the others the column
    assert n[4] == (N_LAT - 3) * N_LON
    assert V3[4] == (N_LON - 1) * 0.5 * (wr[3] + wr[0]) + 2.0 * (0.5 * (wr[4:] + wr[1:10])).sum()
    np.testing.assert_array_equal(V2, 0.0)
    np.testing.assert_array_equal(V1, V3)                 # (vy - 0)^2 = vy for vy in {0, 1}
  finally:
    nd.close()


# ---- 5. structure (negative controls) ---------------------------------------------------------------------------------------------
def test_energy_pairs_follow_the_slots():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w = _data(M, G, B, C, seed=51)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_energy_set(2, GROUP6, SCALE6)
    d2, s0, _ = nd.ens_energy_score(truth)
    # two slots swapped: the pair index moves with them, bit for bit (the points are added in the same order for every pair)
    a, b = 2, 6
    nd.ens_push_host(a, members[b])
    nd.ens_push_host(b, members[a])
    swapped, s0s, _ = nd.ens_energy_score(None)
    sigma = {a: b, b: a}
    moved = 0
    for (i, j) in R.pairs(M):
      i2, j2 = sorted((sigma.get(i, i), sigma.get(j, j)))
      assert np.array_equal(swapped[:, :, R.pair_index(i2, j2)], d2[:, :, R.pair_index(i, j)]), (i, j)
      moved += (i2, j2) != (i, j)
    assert moved == 2 * (M - 1) and s0s.tobytes() == s0.tobytes()      # each of the two slots against the M - 1 other fields
    assert not np.array_equal(swapped, d2)
    nd.ens_push_host(a, members[a])
    nd.ens_push_host(b, members[b])
    # one member changed at one point of group 0: only that member's row and column of the pair matrix change
    m = 5
    changed = members[m].copy()
    changed[200, 1, 1] += np.float32(3.0)
    nd.ens_push_host(m, changed)
    got, _, _ = nd.ens_energy_score(None)
    for (i, j) in R.pairs(M):
      p = R.pair_index(i, j)
      if m in (i, j):
        assert got[1, 0, p] != d2[1, 0, p], (i, j)
      else:
        assert got[1, 0, p] == d2[1, 0, p], (i, j)
    assert np.array_equal(got[0], d2[0]) and np.array_equal(got[:, 1], d2[:, 1])      # the other batch member, the other group
  finally:
    nd.close()


def test_energy_of_single_channels_gives_the_marginal_sums():
  """Single-channel groups with a = 1: the pair sums contain the spread and the error of the ensemble mean that gc_ens_score
  forms from the same store -- sum_{i<j<M} D2 / (M (M - 1)) = sums[3] (the M - 1 variance) and
  sum_i D2[i, M] / M - sum_{i<j<M} D2 / M^2 = sums[2] ((m - y)^2)."""
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w = _data(M, G, B, C, seed=53)
  truth[10:20, 0, 3] = np.nan
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_energy_set(C, np.arange(C, dtype=np.int32), np.ones(C))
    d2, s0, _ = nd.ens_energy_score(truth)
    sums, _ = nd.ens_score(None)
    n_mm = M * (M - 1) // 2
    mm, my = d2[..., :n_mm].sum(axis=-1), d2[..., n_mm:].sum(axis=-1)
    for got, want in ((mm / (M * (M - 1)), sums[..., 3]), (my / M - mm / (M * M), sums[..., 2]), (s0, sums[..., 0])):
      assert np.all(np.abs(got - want) <= 1e-9 * np.maximum(np.abs(got), np.abs(want)))
  finally:
    nd.close()


# ---- 6. plans, allocations, errors --------------------------------------------------------------------------------------------------
def test_plans_survive_reserve_and_replace_their_buffers():
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w = _data(50, G, B, C, seed=61)
  nd = _handle(gr, B, C)
  try:
    base = nd.counter("device_allocations")
    nd.ens_energy_set(2, GROUP6, SCALE6)
    nd.ens_variogram_set(N_LAT, N_LON, OFFSETS, 0.5)
    held = nd.counter("device_allocations")
    assert held > base
    for _ in range(3):                                            # replaced, not added
      nd.ens_energy_set(3, np.array([0, 0, 1, 2, 2, -1], np.int32), SCALE6)
      nd.ens_variogram_set(N_LAT, N_LON, OFFSETS[:2], 2.0)
      assert nd.counter("device_allocations") == held
    nd.ens_energy_set(2, GROUP6, SCALE6)
    nd.ens_variogram_set(N_LAT, N_LON, OFFSETS, 0.5)
    assert nd.counter("device_allocations") == held
    _push_all(nd, members[:8], w)
    _check_energy("M = 8", nd.ens_energy_score(truth), R.energy(members[:8], truth, w, GROUP6, SCALE6))
    work = nd.counter("device_allocations")
    # M from 8 to 50 through reserve and push, WITHOUT a new plan
    _push_all(nd, members)
    _check_energy("M = 50 after M = 8", nd.ens_energy_score(None), R.energy(members, truth, w, GROUP6, SCALE6))
    _check_variogram("M = 50 after M = 8", nd.ens_variogram_score(None), R.variogram(members, truth, w, N_LAT, N_LON, OFFSETS, 0.5),
                     G, 50)
    assert nd.counter("device_allocations") == work               # the work buffers were replaced, not added
    nd.ens_energy_set(1, np.zeros(C, np.int32), np.ones(C))      # a new plan: the work buffers follow it at the next call
    _check_energy("K = 1", nd.ens_energy_score(None), R.energy(members, truth, w, np.zeros(C, np.int32), np.ones(C)))
    assert nd.counter("device_allocations") == work
    assert nd.counter("ens_energy_calls") == 3 and nd.counter("ens_variogram_calls") == 1
    assert nd.counter("ens_energy_device_us") >= 0 and nd.counter("ens_variogram_device_us") >= 0
  finally:
    nd.close()


def test_state_and_argument_errors():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 3
  members, truth, w = _data(M, G, B, C, seed=71)
  lib = _lib.load_library()
  dp, ip, u64 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64)
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  nd = _handle(gr, B, C)
  P = M * (M + 1) // 2
  d2, s0 = np.empty((B, 2, P)), np.empty((B, 2))
  vs = np.empty((4, B, C, 2))
  offs = np.array([[0, 1], [1, 0]], np.int32)

  def e_set(h, K, group, scale):
    g = None if group is None else np.asarray(group, np.int32).ctypes.data_as(ip)
    a = None if scale is None else np.asarray(scale, np.float64).ctypes.data_as(dp)
    return lib.gc_ens_energy_set(h._h, K, g, a)

  def v_set(h, n_lat, n_lon, o, p):
    o = None if o is None else np.ascontiguousarray(o, np.int32)
    return lib.gc_ens_variogram_set(h._h, n_lat, n_lon, 0 if o is None else len(o), None if o is None else o.ctypes.data_as(ip), p)

  try:
    # no graph
    assert e_set(bare, 2, GROUP6, SCALE6) == _lib.GC_ERR_STATE
    assert lib.gc_ens_variogram_set(bare._h, N_LAT, N_LON, 2, offs.ctypes.data_as(ip), 0.5) == _lib.GC_ERR_STATE
    assert lib.gc_ens_energy_score(bare._h, None, d2.ctypes.data_as(dp), s0.ctypes.data_as(dp), None) == _lib.GC_ERR_STATE
    assert lib.gc_ens_variogram_score(bare._h, None, vs.ctypes.data_as(dp), None) == _lib.GC_ERR_STATE
    # the limits of the plans
    assert e_set(nd, 0, GROUP6, SCALE6) == _lib.GC_ERR_UNSUPPORTED and e_set(nd, 33, GROUP6, SCALE6) == _lib.GC_ERR_UNSUPPORTED
    assert e_set(nd, 2, None, SCALE6) == _lib.GC_ERR_INVALID_ARGUMENT and e_set(nd, 2, GROUP6, None) == _lib.GC_ERR_INVALID_ARGUMENT
    assert e_set(nd, 2, [0, 0, 1, 2, 1, -1], SCALE6) == _lib.GC_ERR_INVALID_ARGUMENT      # a group index beyond K - 1
    assert e_set(nd, 2, [0, 0, -2, 1, 1, -1], SCALE6) == _lib.GC_ERR_INVALID_ARGUMENT
    assert e_set(nd, 3, GROUP6, SCALE6) == _lib.GC_ERR_INVALID_ARGUMENT and b"empty" in lib.gc_last_error(nd._h)
    for bad in (0.0, -1.0, np.nan, np.inf):
      a = SCALE6.copy()
      a[1] = bad
      assert e_set(nd, 2, GROUP6, a) == _lib.GC_ERR_INVALID_ARGUMENT
      with pytest.raises(ValueError):
        nd.ens_energy_set(2, GROUP6, a)
    a = SCALE6.copy()
    a[5] = np.nan                                                 # the scale of a channel in no group is not read
    assert e_set(nd, 2, GROUP6, a) == _lib.GC_OK
    for K, g in ((0, GROUP6), (33, GROUP6), (3, GROUP6), (2, GROUP6[:5])):
      with pytest.raises(ValueError):
        nd.ens_energy_set(K, g, SCALE6[:len(g)])
    assert v_set(nd, N_LAT, N_LON, np.zeros((17, 2)) + 1, 0.5) == _lib.GC_ERR_UNSUPPORTED
    assert lib.gc_ens_variogram_set(nd._h, N_LAT, N_LON, 0, offs.ctypes.data_as(ip), 0.5) == _lib.GC_ERR_UNSUPPORTED
    for bad in (0.25, 3.0, np.nan):
      assert v_set(nd, N_LAT, N_LON, offs, bad) == _lib.GC_ERR_UNSUPPORTED
      with pytest.raises(ValueError):
        nd.ens_variogram_set(N_LAT, N_LON, offs, bad)
    assert lib.gc_ens_variogram_set(nd._h, N_LAT, N_LON, 2, None, 0.5) == _lib.GC_ERR_INVALID_ARGUMENT
    assert v_set(nd, N_LAT, N_LON + 1, offs, 0.5) == _lib.GC_ERR_INVALID_ARGUMENT
    for bad in ([[0, 0]], [[13, 0]], [[-13, 1]], [[0, 24]], [[1, -24]]):
      assert v_set(nd, N_LAT, N_LON, bad, 0.5) == _lib.GC_ERR_INVALID_ARGUMENT
      with pytest.raises(ValueError):
        nd.ens_variogram_set(N_LAT, N_LON, bad, 0.5)
    # before any plan
    fresh = _handle(gr, B, C)
    try:
      with pytest.raises(_lib.GencastHipError, match="ens_energy_set"):
        fresh.ens_energy_score(truth)
      with pytest.raises(_lib.GencastHipError, match="ens_variogram_set"):
        fresh.ens_variogram_score(truth)
      assert lib.gc_ens_energy_score(fresh._h, None, d2.ctypes.data_as(dp), s0.ctypes.data_as(dp), None) == _lib.GC_ERR_STATE
      assert b"gc_ens_energy_set" in lib.gc_last_error(fresh._h)
      assert lib.gc_ens_variogram_score(fresh._h, None, vs.ctypes.data_as(dp), None) == _lib.GC_ERR_STATE
      assert b"gc_ens_variogram_set" in lib.gc_last_error(fresh._h)
    finally:
      fresh.close()
    nd.ens_energy_set(2, GROUP6, SCALE6)
    nd.ens_variogram_set(N_LAT, N_LON, offs, 0.5)
    # no store; a slot unpushed; no weights; no truth
    assert lib.gc_ens_energy_score(nd._h, None, d2.ctypes.data_as(dp), s0.ctypes.data_as(dp), None) == _lib.GC_ERR_STATE
    assert b"gc_ens_reserve" in lib.gc_last_error(nd._h)
    assert lib.gc_ens_variogram_score(nd._h, None, vs.ctypes.data_as(dp), None) == _lib.GC_ERR_STATE
    nd.ens_reserve(M)
    for i in range(M - 1):
      nd.ens_push_host(i, members[i])
    for call in (nd.ens_energy_score, nd.ens_variogram_score):
      with pytest.raises(_lib.GencastHipError, match=f"slot {M - 1} has not been pushed"):
        call(truth)
    nd.ens_push_host(M - 1, members[M - 1])
    for call in (nd.ens_energy_score, nd.ens_variogram_score):
      with pytest.raises(_lib.GencastHipError, match="no node weights"):
        call(truth)
    nd.ens_set_node_weight(w)
    for call in (nd.ens_energy_score, nd.ens_variogram_score):
      with pytest.raises(_lib.GencastHipError, match="no truth"):
        call(None)
      with pytest.raises(ValueError, match="truth must be"):
        call(truth[:-1])
    assert lib.gc_ens_energy_score(nd._h, None, None, s0.ctypes.data_as(dp), None) == _lib.GC_ERR_INVALID_ARGUMENT
    assert lib.gc_ens_energy_score(nd._h, None, d2.ctypes.data_as(dp), None, None) == _lib.GC_ERR_INVALID_ARGUMENT
    assert lib.gc_ens_variogram_score(nd._h, None, None, None) == _lib.GC_ERR_INVALID_ARGUMENT
    # and the calls go through, with the optional outputs left out
    t = np.ascontiguousarray(truth)
    assert lib.gc_ens_energy_score(nd._h, t.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), d2.ctypes.data_as(dp),
                                   s0.ctypes.data_as(dp), None) == _lib.GC_OK
    assert lib.gc_ens_variogram_score(nd._h, None, vs.ctypes.data_as(dp), None) == _lib.GC_OK
    ref = R.energy(members, truth, w, GROUP6, SCALE6)
    _check_energy("C ABI", (d2, s0, 0), ref)
    _check_variogram("C ABI", (vs, nd.ens_variogram_score(None)[1]), R.variogram(members, truth, w, N_LAT, N_LON, offs.tolist(), 0.5),
                     G, M)
  finally:
    nd.close()
    bare.close()


# ---- 7. a scored store ------------------------------------------------------------------------------------------------------------
def test_scored_store_scores_both():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w = _data(M, G, B, C, seed=81)
  espec = {"n_groups": 2, "group": GROUP6, "scale": SCALE6, "names": ("uv", "rest")}
  vspec = verification.VariogramSpec(OFFSETS, 0.5).grid_plan(N_LAT, N_LON)
  nd = _handle(gr, B, C)
  try:
    store = verification.ScoredStore(nd, M, w, energy=espec, variogram=vspec)
    store.setup()
    for i, x in enumerate(members):
      nd.ens_push_host(i, x)
    store.score(truth)
    en, vg = store.score_energy(None), store.score_variogram(None)
    ref = R.energy(members, truth, w, GROUP6, SCALE6)
    want = R.energy_scores(ref["d2"], ref["s0"], M)
    assert en.names == ("uv", "rest") and en.n_forecasts == B and en.invalid == 0
    np.testing.assert_allclose(en.err, want["err"], rtol=1e-12)
    np.testing.assert_allclose(en.energy_score, want["fair"].mean(axis=0), rtol=1e-12)
    assert isinstance(vg, VariogramScores) and vg.offsets == tuple(OFFSETS) and vg.p == 0.5
    _check_variogram("store", (vg.sums, vg.counts), R.variogram(members, truth, w, N_LAT, N_LON, OFFSETS, 0.5), G, M)
    plain = verification.ScoredStore(nd, M, w)
    assert plain.score_energy(None) is None and plain.score_variogram(None) is None
  finally:
    nd.close()
