"""An ensemble scored against a climatology on the device (gc_ens_clim_score) against the float64
definition restated in tests/clim_reference.py.

Tolerance: the bound of section 8c, carried over and not tuned.  The slot-order sums of a point are the same IEEE double
operations on both sides; what differs is the order of the G additions of a column and the form of the mean absolute
difference (the gaps of the sorted sample on the device, all pairs in the reference), so per sum
|device - reference| <= (G + max(M, K)^2 + 8) 2^-53 sum |term| (`clim_reference.tolerance`).  Counts, `invalid` and A0 on
dyadic weights are integers or exact: ==.

Sizes: the 13 x 24 grid (G = 312) with handles that know their graph only.  (B, C) = (2, 3): 6 columns, 42 node lanes per
workgroup; (4, 82): W = 328 columns, more than the 256 columns of one tile and no multiple of the wave size (the second tile
is 72 wide: 3 lanes, 40 idle threads).  The (M, K) pairs cover M < K and K < M across different paddings, sizes that are no
powers of two, and the register-heaviest instance."""
import ctypes

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, geometry
from gencast_flax_nnx_amd.verification import ClimatologyScores
from tests import clim_reference as R
from tests.helpers import graph_handle as _handle, small_graph as _graph

pytestmark = pytest.mark.gpu

WORST = {}                                                 # tag -> worst |device - reference| / bound, printed by every check


def _data(M, K, G, B, C, seed, scale=None, offset=None):
  rng = np.random.default_rng(seed)
  scale = np.logspace(-2, 3, C) if scale is None else scale
  offset = np.linspace(0.0, 300.0, C) if offset is None else offset
  clim = (offset + rng.standard_normal((K, G, B, C)) * scale).astype(np.float32)
  truth = (offset + rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  members = (truth + 0.5 * rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)      # a forecast with some skill
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  return members, clim, truth, w


def _push_all(nd, fields, w=None):
  nd.ens_reserve(len(fields))
  if w is not None:
    nd.ens_set_node_weight(w)
  for i, x in enumerate(fields):
    nd.ens_push_host(i, x)


def _check(tag, out, ref, G):
  """Sums within the bound (the worst ratio of error to bound is printed first), counts and invalid exact."""
  sums, counts, invalid = out
  tol = R.tolerance(ref, G)
  assert sums.shape == ref["sums"].shape and sums.dtype == np.float64, f"{tag}: sums {sums.shape}"
  err = np.abs(sums - ref["sums"])
  ratio = np.max(err / np.maximum(tol, 1e-300), axis=(0, 1))
  WORST[tag] = float(ratio.max())
  print(f"{tag}: worst |device - reference| / bound per sum " + " ".join(f"{n}={r:.3f}" for n, r in zip(R.NAMES, ratio)))
  assert np.isfinite(sums).all(), f"{tag}: a sum is not finite"
  for k, name in enumerate(R.NAMES):
    assert np.all(err[..., k] <= tol[..., k]), f"{tag}: {name} outside (G + max(M, K)^2 + 8) 2^-53 sum|term|"
  assert counts.dtype == np.uint64
  np.testing.assert_array_equal(counts, ref["counts"], err_msg=f"{tag}: counts")
  assert invalid == ref["invalid"], f"{tag}: invalid"


# ---- 1. every padding pair ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(2, 2), (3, 8), (8, 3), (33, 5), (5, 33), (50, 30), (64, 64)])
def test_every_padding_pair_matches_the_float64_definition(M, K):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 3
  members, clim, truth, w = _data(M, K, G, B, C, seed=100 * M + K)
  ref = R.reference(members, clim, truth, w)
  nd, cl = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)                                    # the climatology handle needs neither weights nor truth
    out = nd.ens_clim_score(cl, truth)
    assert out[0].shape == (B, C, 12) and out[1].shape == (B, C)
    _check(f"tiny M={M} K={K}", out, ref, G)
    assert nd.counter("ens_clim_invalid_points") == 0 and nd.counter("ens_clim_calls") == 1
    again = nd.ens_clim_score(cl, None)                    # the truth is on the device
    assert out[0].tobytes() == again[0].tobytes() and out[1].tobytes() == again[1].tobytes() and out[2] == again[2]
    sc, want = ClimatologyScores(out[0], out[1], M, K, out[2]), R.scores(ref)
    for name, v in want.items():
      np.testing.assert_allclose(getattr(sc, name), v, rtol=1e-9, atol=1e-12, err_msg=name)
    assert np.all(sc.acc > 0.5) and np.all(sc.crpss > 0.0)  # (the members were drawn around the truth)
  finally:
    nd.close()
    cl.close()


# ---- 2. column tiling -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(8, 8), (64, 64)])
def test_more_columns_than_one_tile(M, K):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 4, 82                       # W = 328 = 256 + 72
  members, clim, truth, w = _data(M, K, G, B, C, seed=7 * M, scale=np.logspace(-2, 4, C), offset=np.linspace(-50.0, 1e5, C))
  members[1, 17, 3, 80] = np.nan                           # an invalid point in the second tile
  ref = R.reference(members, clim, truth, w)
  nd, cl = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)
    _check(f"W=328 M={M} K={K}", nd.ens_clim_score(cl, truth), ref, G)
  finally:
    nd.close()
    cl.close()


def test_a_second_column_tile_of_one_column():
  """(B, C) = (1, 257): the second column tile is one column wide, 256 node lanes for the 8 nodes of a block."""
  gr = _graph()
  G, B, C, M, K = gr.num_grid_nodes, 1, 257, 3, 3
  members, clim, truth, w = _data(M, K, G, B, C, seed=257)
  members[1, 17, 0, 256] = np.nan                          # an invalid point in the one-column tile
  ref = R.reference(members, clim, truth, w)
  nd, cl = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)
    _check("W=257", nd.ens_clim_score(cl, truth), ref, G)
  finally:
    nd.close()
    cl.close()


def test_a_width_that_is_no_multiple_of_the_wave_size():
  gr = _graph()
  G, B, C, M, K = gr.num_grid_nodes, 1, 37, 5, 3           # 6 lanes of 37 columns: lanes straddle the waves, 34 idle threads
  members, clim, truth, w = _data(M, K, G, B, C, seed=37)
  ref = R.reference(members, clim, truth, w)
  nd, cl = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)
    _check("W=37", nd.ens_clim_score(cl, truth), ref, G)
  finally:
    nd.close()
    cl.close()


# ---- 3. ties and invalid points -------------------------------------------------------------------------------------------
def test_ties_and_invalid_points():
  gr = _graph()
  G, B, C, M, K = gr.num_grid_nodes, 2, 3, 8, 5
  members, clim, truth, _ = _data(M, K, G, B, C, seed=21)
  w = (np.arange(G) % 7 + 1).astype(np.float32) / 8.0      # dyadic: their sums are exact in any order
  all_equal, two_equal, on_truth = np.array([30, 31, 250]), np.array([0, 5, 77]), np.array([11, 200, G - 1])
  members[:, all_equal] = members[0, all_equal]            # d_x = 0 there
  members[2, two_equal] = members[6, two_equal]            # duplicated values
  clim[1, two_equal] = clim[3, two_equal]
  members[3, on_truth] = truth[on_truth]                   # a member equal to y
  clim[:, 40:44] = clim[0, 40:44]                          # a climatological mean pushed K times: d_c = 0
  nan_truth, inf_member, nan_clim, shared = (3, 0, 1), (120, 1, 2), (251, 0, 0), (9, 1, 1)
  truth[nan_truth] = np.nan
  members[(5,) + inf_member] = np.inf
  clim[(4,) + nan_clim] = np.nan
  truth[shared] = np.nan                                   # all three at one point: counted as invalid once
  members[(0,) + shared] = -np.inf
  clim[(2,) + shared] = np.nan
  clim[0, 60:70, 1, 0] = np.nan                            # points invalid only through the climatology
  members[:, :, 0, 2] = np.nan                             # a column that is wholly invalid
  ref = R.reference(members, clim, truth, w)
  nd, cl = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)
    sums, counts, invalid = out = nd.ens_clim_score(cl, truth)
    _check("ties", out, ref, G)
    # what is counted, from first principles
    keep = np.ones((G, B, C), bool)
    for p in (nan_truth, inf_member, nan_clim, shared):
      keep[p] = False
    keep[60:70, 1, 0] = False
    keep[:, 0, 2] = False
    assert invalid == int((~keep).sum()) == nd.counter("ens_clim_invalid_points")
    np.testing.assert_array_equal(counts, keep.sum(0).astype(np.uint64))
    np.testing.assert_array_equal(sums[..., 0], (w.astype(np.float64)[:, None, None] * keep).sum(0))   # A0: exact
    assert not sums[0, 2].any() and counts[0, 2] == 0      # the wholly invalid column: zeros, no NaN
    # a point invalid only through the climatology adds nothing: without those nodes every sum of the column is the same
    less = np.delete(np.arange(G), np.arange(60, 70))
    part = R.reference(members[:, less], clim[:, less], truth[less], w[less])
    assert np.all(np.abs(sums[1, 0] - part["sums"][1, 0]) <= R.tolerance(part, G)[1, 0])
  finally:
    nd.close()
    cl.close()


def test_equal_members_and_equal_samples_give_zero_spread_terms():
  gr = _graph()
  G, B, C, M, K = gr.num_grid_nodes, 2, 3, 33, 2
  members, clim, truth, w = _data(M, K, G, B, C, seed=33)
  members[:] = members[0]
  clim[:] = clim[0]                                        # a plain climatological mean field, pushed twice
  nd, cl = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)
    sums, _, _ = out = nd.ens_clim_score(cl, truth)
    _check("flat", out, R.reference(members, clim, truth, w), G)
    assert not sums[..., 9].any() and not sums[..., 11].any()          # F5 == 0 and C5 == 0, exactly
  finally:
    nd.close()
    cl.close()


# ---- 4. agreement with the existing scorer --------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(3, 8), (50, 30)])
def test_agrees_with_ens_score_on_the_same_store(M, K):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 3
  members, clim, truth, _ = _data(M, K, G, B, C, seed=40 + M)
  w = (np.arange(G) % 5 + 1).astype(np.float32) / 4.0      # dyadic
  members[1, 5:40] = members[0, 5:40]
  truth[100:110] = members[M - 1, 100:110]
  truth[7, 1, 1] = np.nan                                  # skipped by both
  ref = R.reference(members, clim, truth, w)
  nd, cl = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)
    s, hist = nd.ens_score(truth)
    sums, counts, invalid = nd.ens_clim_score(cl, None)
    np.testing.assert_array_equal(sums[..., 0], s[..., 0])             # A0 == S0 on dyadic weights
    np.testing.assert_array_equal(counts, hist.sum(-1))
    assert invalid == nd.counter("ens_invalid_points") == 1
    both = ((G + M * M + 8) + (G + max(M, K) ** 2 + 8)) * 2.0 ** -53
    for mine, theirs in ((8, 4), (9, 5), (7, 2)):                      # F4 ~ S4, F5 ~ S5, A7 ~ S2
      err = np.abs(sums[..., mine] - s[..., theirs])
      print(f"M={M} K={K}: {R.NAMES[mine]} vs S{theirs}: worst error / sum of both bounds "
            f"{np.max(err / (both * ref['abs'][..., mine])):.3f}")
      assert np.all(err <= both * ref["abs"][..., mine]), R.NAMES[mine]
  finally:
    nd.close()
    cl.close()


# ---- 5. determinism: nothing else is touched ------------------------------------------------------------------------------
def test_everything_around_the_call_stays_bit_identical():
  gr = _graph()
  G, B, C, M, K = gr.num_grid_nodes, 2, 3, 8, 5
  members, clim, truth, w = _data(M, K, G, B, C, seed=55)
  nd, cl = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)
    nd.ens_order_set((0.1, 0.5))
    score0, order0 = nd.ens_score(truth), nd.ens_order_score(None)
    first = nd.ens_clim_score(cl, None)
    held, held_c = nd.counter("device_allocations"), cl.counter("device_allocations")
    for _ in range(3):
      again = nd.ens_clim_score(cl, None)
      assert again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    assert nd.counter("device_allocations") == held and cl.counter("device_allocations") == held_c
    for i in range(M):
      assert nd.ens_download_member(i).tobytes() == members[i].tobytes()
    for j in range(K):
      assert cl.ens_download_member(j).tobytes() == clim[j].tobytes()
    score1, order1 = nd.ens_score(None), nd.ens_order_score(None)
    for a, b in zip(score0 + order0[:4], score1 + order1[:4]):
      assert a.tobytes() == b.tobytes()
    for q in range(2):
      nd.ens_order_quantile(q)                             # the quantile fields are still there
    # either store reserved again: replaced, not added; the result follows the new stores
    _push_all(cl, clim[:3])
    _push_all(nd, members[:5])
    out = nd.ens_clim_score(cl, None)
    _check("re-reserved", out, R.reference(members[:5], clim[:3], truth, w), G)
    assert nd.counter("device_allocations") == held and cl.counter("device_allocations") == held_c
    assert nd.counter("ens_clim_calls") == 5 and nd.counter("ens_clim_device_us") >= 0
  finally:
    nd.close()
    cl.close()


# ---- 6. state and argument errors -----------------------------------------------------------------------------------------
def test_state_and_argument_errors():
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 3
  members, clim, truth, w = _data(3, 2, G, B, C, seed=61)
  lib = _lib.load_library()
  dp = ctypes.POINTER(ctypes.c_double)
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  nd, cl, wide, deep = _handle(gr, B, C), _handle(gr, B, C), _handle(gr, B, C + 1), _handle(gr, B + 1, C)
  other = _handle(_graph(9, 16), B, C)
  sums = np.empty((B, C, 12))
  sp = sums.ctypes.data_as(dp)

  def raw(h, c, s=sp):
    return lib.gc_ens_clim_score(h._h, None if c is None else c._h, None, s, None, None)

  try:
    assert lib.gc_ens_clim_score(None, cl._h, None, sp, None, None) == _lib.GC_ERR_INVALID_ARGUMENT
    assert raw(nd, None) == _lib.GC_ERR_INVALID_ARGUMENT and b"another handle" in lib.gc_last_error(nd._h)
    assert raw(nd, nd) == _lib.GC_ERR_INVALID_ARGUMENT and b"another handle" in lib.gc_last_error(nd._h)
    assert raw(nd, cl, None) == _lib.GC_ERR_INVALID_ARGUMENT and b"null argument" in lib.gc_last_error(nd._h)
    assert raw(bare, cl) == _lib.GC_ERR_STATE and b"gc_set_graph" in lib.gc_last_error(bare._h)
    for bad in (wide, deep, other, bare):                  # other c_out, other batch, other G, no graph at all
      assert raw(nd, bad) == _lib.GC_ERR_INVALID_ARGUMENT
      assert b"the climatology handle has other dimensions (G, batch, c_out)" in lib.gc_last_error(nd._h)
    with pytest.raises(ValueError, match="another handle"):
      nd.ens_clim_score(nd)
    with pytest.raises(TypeError):
      nd.ens_clim_score(None)
    with pytest.raises(_lib.GencastHipError, match="ens_reserve"):
      nd.ens_clim_score(cl)
    # no store on h; none on the climatology handle; unpushed slots on either; no weights; no truth
    assert raw(nd, cl) == _lib.GC_ERR_STATE and b"no member store (gc_ens_reserve)" in lib.gc_last_error(nd._h)
    nd.ens_reserve(3)
    assert raw(nd, cl) == _lib.GC_ERR_STATE and b"no member store on the climatology handle" in lib.gc_last_error(nd._h)
    cl.ens_reserve(2)
    for i in range(2):
      nd.ens_push_host(i, members[i])
    with pytest.raises(_lib.GencastHipError, match="(?<!climatology )member slot 2 has not been pushed"):
      nd.ens_clim_score(cl, truth)
    nd.ens_push_host(2, members[2])
    cl.ens_push_host(1, clim[1])
    with pytest.raises(_lib.GencastHipError, match="climatology member slot 0 has not been pushed"):
      nd.ens_clim_score(cl, truth)
    assert raw(nd, cl) == _lib.GC_ERR_STATE
    cl.ens_push_host(0, clim[0])
    with pytest.raises(_lib.GencastHipError, match="no node weights"):
      nd.ens_clim_score(cl, truth)
    nd.ens_set_node_weight(w)
    with pytest.raises(_lib.GencastHipError, match="no truth on the device"):
      nd.ens_clim_score(cl, None)
    assert raw(nd, cl) == _lib.GC_ERR_STATE
    with pytest.raises(ValueError, match="truth must be"):
      nd.ens_clim_score(cl, truth[:-1])
    assert nd.counter("ens_clim_calls") == 0
    _check("after the errors", nd.ens_clim_score(cl, truth), R.reference(members, clim, truth, w), G)
    assert raw(nd, cl) == _lib.GC_OK                       # counts and invalid may be NULL
    np.testing.assert_array_equal(sums, nd.ens_clim_score(cl, None)[0])
  finally:
    for h in (nd, cl, wide, deep, other, bare):
      h.close()


# ---- 7. full-size grids, set_graph only -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["nano", "one_degree"])
def test_full_size(case):
  if case == "nano":
    gr, M, K, hw = _graph(73, 144, mesh_size=4, k_hop=8), 50, 30, dict(latent=256, heads=4, ffw=2048)
  else:
    lat, lon = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0)
    gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=5, attention_k_hop=8)
    M, K, hw = 8, 8, dict(latent=512, heads=4, ffw=2048)
  G, B, C = gr.num_grid_nodes, 1, (32 if case == "nano" else 82)   # (nano: 1 660 pairs per point in the reference -- fewer columns)
  assert G == (10512 if case == "nano" else 65160)
  members, clim, truth, w = _data(M, K, G, B, C, seed=11, scale=np.logspace(-2, 4, C), offset=np.linspace(0.0, 1e5, C))
  clim[2, 1000, 0, C - 1] = np.nan
  ref = R.reference(members, clim, truth, w)
  nd, cl = _handle(gr, B, C, **hw), _handle(gr, B, C, **hw)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)
    out = nd.ens_clim_score(cl, truth)
    print(f"{case}: ens_clim_device_us {nd.counter('ens_clim_device_us')}")
    # the regime: loss_reduce_blocks = min(kLossMaxBlocks = 2048, ceil(G / (8 q))) -- nano: W = 32, q = 8, ceil(10512 / 64) =
    # 165; one degree: W = 82, q = 3, 2715 -> 2048 (per = 32, 11 trailing workgroups without nodes)
    assert nd.counter("ens_clim_blocks") == (165 if case == "nano" else 2048)
    _check(case, out, ref, G)
  finally:
    nd.close()
    cl.close()
