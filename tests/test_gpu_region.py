"""Regional ensemble scores on the device (gc_ens_region_*) against the float64 yardstick of
tests/region_reference.py: per region, tests/verification_reference.py on the region's node subset.

Tolerance, derived as in section 8c and not measured: |device - reference| <= (G + M^2 + 8) 2^-53 A_k per sum, A_k the
reference's absolute sum over that region (`region_reference.sum_tolerance`).  Where two DEVICE results are compared (with
gc_ens_score), each lies within its own bound of the exact value, so the two bounds add.  Histograms, `invalid`, and S0 on
dyadic weights are integers or exact sums: ==.

Sizes: the 13 x 24 grid (G = 312) with handles that know their graph only.  (B, C) = (2, 6): W = 12 columns, q = 21 node
lanes per workgroup; (4, 82): W = 328, two column tiles, one lane in the full tile."""
import ctypes

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib
from gencast_flax_nnx_amd.verification import RegionScores
from tests import region_reference as R
from tests import verification_reference as VR
from tests.helpers import graph_handle as _handle, small_graph as _graph

pytestmark = pytest.mark.gpu

N_LAT, N_LON = 13, 24
NAN_TRUTH = np.array([3, 4, 97, 98, 150, 151, 152, 300])           # nodes whose truth is NaN, in every column
U = 2.0 ** -53


def _data(M, G, B, C, seed, dyadic=True):
  """Members, truth and weights with everything the kernel has a branch for: a NaN block in the truth, a NaN and an inf in
  single members -- on nodes the regions of `_regions` list (3, 4, 150.., 300; 9, 120) and on nodes they do not (97, 98;
  99, 96) -- ties between members and between a member and the truth."""
  rng = np.random.default_rng(seed)
  scale = np.logspace(-3, 5, C)
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  w = ((np.arange(G) % 7 + 1).astype(np.float32) / 8.0 if dyadic        # dyadic: their sums are exact in any order
       else rng.uniform(0.1, 2.0, G).astype(np.float32))
  members[1, 40:44] = members[0, 40:44]                           # ties between members
  truth[50:54] = members[0, 50:54]                                # a member equal to the truth is not below it
  truth[NAN_TRUTH] = np.nan
  members[M // 2, 9, 1, 2] = np.nan
  members[0, 120, 0, 4] = np.inf
  members[M - 1, 99, 0, 1] = np.nan                               # node 99 and node 96 belong to no region of `_regions`
  members[0, 96, 1, 0] = np.inf
  return members, truth, w


def _regions(W):
  """R = 8 on the 13 x 24 grid: three latitude bands (rows 0-3, 5-7, 9-12), a box over rows 6-10 that wraps through 0
  degrees and overlaps two of them, a single-node region, a region of exactly q nodes and one of q + 1 (q: the node lanes
  of a full column tile), and an empty region.  Nodes 96-99 (and more of rows 4 and 8 where q is small) are in none."""
  q = 256 // min(256, W)
  bits = np.zeros(N_LAT * N_LON, np.uint32)
  node = np.arange(N_LAT * N_LON).reshape(N_LAT, N_LON)
  bits[node[0:4].ravel()] |= 1
  bits[node[5:8].ravel()] |= 2
  bits[node[9:13].ravel()] |= 4
  bits[node[6:11][:, [22, 23, 0, 1, 2]].ravel()] |= 8
  bits[100] |= 16
  bits[101:101 + q] |= 32
  bits[192:192 + q + 1] |= 64
  assert not bits[96:100].any() and not (bits >> 7).any()
  return bits, 8


def _push_all(nd, members, w=None):
  nd.ens_reserve(len(members))
  if w is not None:
    nd.ens_set_node_weight(w)
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _check(tag, out, ref, G, M, dyadic=True):
  """Sums within the bound (the worst ratio of error to bound is printed first), histograms and invalid exact."""
  sums, hist, invalid = out
  assert sums.shape == ref["sums"].shape and sums.dtype == np.float64, f"{tag}: sums {sums.shape}"
  tol = R.sum_tolerance(ref, G, M)
  err = np.abs(sums - ref["sums"])
  for k, name in enumerate(VR.SUM_NAMES):
    ratio = float(np.max(np.where(err[..., k] > 0, err[..., k] / np.maximum(tol[..., k], 1e-300), 0.0)))
    print(f"{tag} {name}: max |device - reference| {err[..., k].max():.3e}, worst ratio to the bound {ratio:.3f}")
  assert np.all(err <= tol), f"{tag}: sums outside (G + M^2 + 8) 2^-53 A_k"
  assert hist.dtype == np.uint64 and invalid.dtype == np.uint64
  np.testing.assert_array_equal(hist, ref["hist"], err_msg=f"{tag}: hist")
  np.testing.assert_array_equal(invalid, ref["invalid"], err_msg=f"{tag}: invalid")
  if dyadic:
    assert sums[..., 0].tobytes() == ref["sums"][..., 0].tobytes(), f"{tag}: S0 on dyadic weights"


def _check_accounting(out, members, truth, bits, n_regions):
  """What is counted, from first principles: invalid[r] and the histogram of region r see the region's points only."""
  sums, hist, invalid = out
  keep = np.isfinite(truth) & np.isfinite(members).all(0)
  for r, idx in enumerate(R.region_nodes(bits, n_regions)):
    assert int(invalid[r]) == int((~keep[idx]).sum()), r
    np.testing.assert_array_equal(hist[r].sum(-1), keep[idx].sum(0).astype(np.uint64))
    assert int(invalid[r]) + int(hist[r].sum()) == idx.size * truth.shape[1] * truth.shape[2]
  unlisted = bits == 0
  assert (~keep[unlisted]).any() and (~keep[~unlisted]).any()     # both kinds of node carry NaN / inf points
  assert np.isfinite(sums).all()


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,B,C", [(2, 2, 6), (3, 2, 6), (8, 2, 6), (17, 2, 6), (50, 2, 6), (64, 2, 6), (8, 4, 82), (50, 4, 82)])
def test_every_region_matches_the_float64_reference_on_its_nodes(M, B, C):
  gr = _graph()
  G = gr.num_grid_nodes
  members, truth, w = _data(M, G, B, C, seed=M + C)
  bits, n_regions = _regions(B * C)
  ref = R.reference(members, truth, w, bits, n_regions)
  sizes = [idx.size for idx in R.region_nodes(bits, n_regions)]
  q = 256 // min(256, B * C)
  assert sizes[4:] == [1, q, q + 1, 0] and min(sizes[:4]) > 20
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_region_set(bits, n_regions)
    out = nd.ens_region_score(truth)
    assert out[0].shape == (n_regions, B, C, 6) and out[1].shape == (n_regions, B, C, M + 1) and out[2].shape == (n_regions,)
    _check(f"W={B * C} M={M}", out, ref, G, M)
    _check_accounting(out, members, truth, bits, n_regions)
    assert not out[0][7].any() and not out[1][7].any() and out[2][7] == 0          # the empty region: zeros
    assert nd.counter("ens_region_invalid_points") == int(out[2].sum())
    again = nd.ens_region_score(None)
    for x, y in zip(out, again):
      assert x.tobytes() == y.tobytes()
    sc = RegionScores(("south", "tropics", "north", "box", "one", "q", "q1", "empty"), *out[:2], M, out[2])
    want = VR.scores({"sums": ref["sums"][1]}, M)
    for name in ("crps", "crps_ensemble", "rmse", "spread", "spread_skill_ratio"):
      np.testing.assert_allclose(getattr(sc["tropics"], name), want[name], rtol=1e-9, atol=0.0, err_msg=name)
  finally:
    nd.close()


def test_a_second_column_tile_of_one_column():
  """(B, C) = (1, 257): the second column tile is one column wide -- 256 node lanes in the pass, and in the finish 256
  lanes for the few blocks of a region.  `_data` needs B >= 2, so the data here are plain but for the NaN truth rows."""
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 1, 257, 3
  rng = np.random.default_rng(257)
  scale = np.logspace(-3, 5, C)
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  truth[NAN_TRUTH] = np.nan
  w = (np.arange(G) % 7 + 1).astype(np.float32) / 8.0
  bits, n_regions = _regions(B * C)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_region_set(bits, n_regions)
    _check("W=257 M=3", nd.ens_region_score(truth), R.reference(members, truth, w, bits, n_regions), G, M)
  finally:
    nd.close()


# ---- 2. R = 1, all nodes: gc_ens_score ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 50])
def test_one_region_of_all_nodes_is_ens_score(M):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w = _data(M, G, B, C, seed=20 + M, dyadic=False)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    before = nd.ens_score(truth)
    skipped = nd.counter("ens_invalid_points")
    nd.ens_region_set(np.ones(G, np.uint32), 1)
    sums, hist, invalid = nd.ens_region_score(None)                # (the truth ens_score uploaded)
    after = nd.ens_score(None)
    for x, y in zip(before, after):                                # gc_ens_score keeps its bytes around the call
      assert x.tobytes() == y.tobytes()
    np.testing.assert_array_equal(hist[0], before[1])
    assert int(invalid[0]) == skipped
    ref = VR.reference(members, truth, w)
    bound = 2 * VR.sum_tolerance(ref, G, M)                        # two device results: the two bounds add
    err = np.abs(sums[0] - before[0])
    print(f"M={M}: worst ratio to the added bounds {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)
    for i in range(M):                                             # the store is read, never written
      assert nd.ens_download_member(i).tobytes() == members[i].tobytes()
  finally:
    nd.close()


# ---- 3. a partition into 4 regions --------------------------------------------------------------------------------------------
def test_a_partition_adds_up_to_the_global_score():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w = _data(M, G, B, C, seed=31)
  bits = (np.uint32(1) << np.random.default_rng(3).integers(0, 4, G).astype(np.uint32)).astype(np.uint32)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    whole, whole_hist = nd.ens_score(truth)
    skipped = nd.counter("ens_invalid_points")
    nd.ens_region_set(bits, 4)
    out = nd.ens_region_score(None)
    _check("partition", out, R.reference(members, truth, w, bits, 4), G, M)
    sums, hist, invalid = out
    np.testing.assert_array_equal(hist.sum(0), whole_hist)
    assert int(invalid.sum()) == skipped
    assert sums[..., 0].sum(0).tobytes() == whole[..., 0].tobytes()                # dyadic weights: exact in any order
    ref = VR.reference(members, truth, w)
    assert np.all(np.abs(sums.sum(0) - whole) <= 2 * VR.sum_tolerance(ref, G, M) + 4 * U * ref["abs_sums"])
  finally:
    nd.close()


# ---- 4. R = 32 ----------------------------------------------------------------------------------------------------------------
def test_thirty_two_regions_with_bit_31_and_nodes_in_all_of_them():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w = _data(M, G, B, C, seed=41)
  g = np.arange(G)
  bits = (np.uint32(1) << (g % 32).astype(np.uint32)).astype(np.uint32)
  bits[g % 5 == 0] |= np.uint32(1) << np.uint32(31)
  bits[:12] = np.uint32(0xFFFFFFFF)                                # nodes 3 and 4 (NaN truth) belong to all 32 regions
  bits[90:100] = 0                                                 # and some nodes to none
  assert int(bits.max()) == 2 ** 32 - 1 and len(np.unique(bits[bits != 0])) <= 256
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_region_set(bits, 32)
    out = nd.ens_region_score(truth)
    _check("R=32", out, R.reference(members, truth, w, bits, 32), G, M)
    assert (out[2] >= 2 * B * C).all()                             # every region skips the points of nodes 3 and 4
    assert out[1][31].sum() > out[1][30].sum()                     # bit 31 carries the g % 5 == 0 nodes too
  finally:
    nd.close()


# ---- 5. atom limits -------------------------------------------------------------------------------------------------------------
def test_256_atoms_score_and_312_are_refused_with_the_old_plan_in_force():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w = _data(M, G, B, C, seed=51)
  bits = (1 + np.arange(G) % 256).astype(np.uint32)                # 256 atoms of one or two nodes: every workgroup has one or two nodes
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_region_set(bits, 9)
    out = nd.ens_region_score(truth)
    _check("256 atoms", out, R.reference(members, truth, w, bits, 9), G, M)
    many = (np.arange(G) + 1).astype(np.uint32)                    # 312 atoms
    with pytest.raises(ValueError, match="256 atoms"):
      nd.ens_region_set(many, 9)
    lib = _lib.load_library()
    assert lib.gc_ens_region_set(nd._h, 9, many.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == _lib.GC_ERR_UNSUPPORTED
    assert b"256 atoms" in lib.gc_last_error(nd._h)
    again = nd.ens_region_score(None)                              # the previous plan is in force
    for x, y in zip(out, again):
      assert x.tobytes() == y.tobytes()
  finally:
    nd.close()


# ---- 6. determinism, replacement, reserve ---------------------------------------------------------------------------------------
def test_plans_replace_each_other_survive_reserve_and_hold_a_flat_number_of_buffers():
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w = _data(50, G, B, C, seed=61)
  bits_a, R_a = _regions(B * C)
  bits_b = (np.uint32(1) << (np.arange(G) // 104).astype(np.uint32)).astype(np.uint32)      # three bands of 104 nodes
  nd = _handle(gr, B, C)
  try:
    nd.ens_region_set(bits_a, R_a)                                 # before any store: the plan is kept on the host
    _push_all(nd, members[:8], w)
    first = nd.ens_region_score(truth)
    _check("plan set before the store", first, R.reference(members[:8], truth, w, bits_a, R_a), G, 8)
    held = nd.counter("device_allocations")
    second = nd.ens_region_score(None)
    for x, y in zip(first, second):                                # the same call twice: identical bytes
      assert x.tobytes() == y.tobytes()
    nd.ens_region_set(bits_b, 3)                                   # another plan replaces the first
    assert nd.counter("device_allocations") == held
    _check("plan b", nd.ens_region_score(None), R.reference(members[:8], truth, w, bits_b, 3), G, 8)
    nd.ens_reserve(50)                                             # M = 50 after M = 8, WITHOUT a new plan
    assert nd.counter("device_allocations") == held
    for i in range(50):
      nd.ens_push_host(i, members[i])
    _check("M = 50 after M = 8", nd.ens_region_score(None), R.reference(members, truth, w, bits_b, 3), G, 50)
    assert nd.counter("device_allocations") == held
    nd.ens_region_set(bits_a, R_a)
    assert nd.counter("device_allocations") == held
    _check("plan a again", nd.ens_region_score(None), R.reference(members, truth, w, bits_a, R_a), G, 50)
    assert nd.counter("device_allocations") == held
  finally:
    nd.close()


# ---- 7. state and argument errors; 8. counters ------------------------------------------------------------------------------------
def test_state_and_argument_errors_and_counters():
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w = _data(8, G, B, C, seed=71)
  bits, n_regions = _regions(B * C)
  lib = _lib.load_library()
  up, dp, u64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  nd = _handle(gr, B, C)
  try:
    sums = np.empty((n_regions, 6, B, C))
    p_bits, p_sums = bits.ctypes.data_as(up), sums.ctypes.data_as(dp)
    assert lib.gc_ens_region_set(bare._h, n_regions, p_bits) == _lib.GC_ERR_STATE                  # no graph
    assert b"gc_set_graph" in lib.gc_last_error(bare._h)
    assert lib.gc_ens_region_score(bare._h, None, p_sums, None, None) == _lib.GC_ERR_STATE
    # gc_ens_region_set: argument errors at the C ABI (the binding raises before the call)
    assert lib.gc_ens_region_set(nd._h, 0, p_bits) == _lib.GC_ERR_UNSUPPORTED
    assert lib.gc_ens_region_set(nd._h, 33, p_bits) == _lib.GC_ERR_UNSUPPORTED
    assert b"1..32" in lib.gc_last_error(nd._h)
    assert lib.gc_ens_region_set(nd._h, n_regions, None) == _lib.GC_ERR_INVALID_ARGUMENT
    assert lib.gc_ens_region_set(nd._h, 6, p_bits) == _lib.GC_ERR_INVALID_ARGUMENT                 # bit 6 is set on nodes 192..
    assert b"node 192 has a bit at or above n_regions" in lib.gc_last_error(nd._h)
    # before any plan
    with pytest.raises(_lib.GencastHipError, match="ens_region_set"):
      nd.ens_region_score(truth)
    assert lib.gc_ens_region_score(nd._h, None, p_sums, None, None) == _lib.GC_ERR_STATE
    assert b"gc_ens_region_set" in lib.gc_last_error(nd._h)
    nd.ens_region_set(bits, n_regions)
    # no store; a slot unpushed; no weights; no truth
    assert lib.gc_ens_region_score(nd._h, None, p_sums, None, None) == _lib.GC_ERR_STATE
    assert b"gc_ens_reserve" in lib.gc_last_error(nd._h)
    nd.ens_reserve(8)
    for i in range(7):
      nd.ens_push_host(i, members[i])
    with pytest.raises(_lib.GencastHipError, match="slot 7 has not been pushed"):
      nd.ens_region_score(truth)
    nd.ens_push_host(7, members[7])
    with pytest.raises(_lib.GencastHipError, match="no node weights"):
      nd.ens_region_score(truth)
    nd.ens_set_node_weight(w)
    with pytest.raises(_lib.GencastHipError, match="no truth"):
      nd.ens_region_score(None)
    assert lib.gc_ens_region_score(nd._h, None, None, None, None) == _lib.GC_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError, match="truth must be"):
      nd.ens_region_score(truth[:-1])
    assert nd.counter("ens_region_calls") == 0
    out = nd.ens_region_score(truth)
    ref = R.reference(members, truth, w, bits, n_regions)
    _check("after the errors", out, ref, G, 8)
    # hist and invalid may be NULL
    assert lib.gc_ens_region_score(nd._h, None, p_sums, None, None) == _lib.GC_OK
    assert np.ascontiguousarray(np.moveaxis(sums, 1, -1)).tobytes() == out[0].tobytes()
    # counters
    assert nd.counter("ens_region_calls") == 2 and nd.counter("ens_region_device_us") >= 0
    assert nd.counter("ens_region_invalid_points") == int(ref["invalid"].sum())
    before = nd.counter("ens_scores")
    nd.ens_region_score(None)
    assert nd.counter("ens_region_calls") == 3 and nd.counter("ens_scores") == before
  finally:
    nd.close()
    bare.close()
