"""Ensemble order statistics on the device (gc_ens_order_*) against the float64 definition restated in
tests/order_reference.py.

Quantile fields: the host hands the device lo, hi and f, and every operation is an IEEE double operation on both sides, so
a field must EQUAL the reference (NaN positions included; the sign of a zero is not asserted).  Sums: w alpha is the same
double product on both sides and only the order of the G additions differs, so |device - reference| <= (G + 8) 2^-53
sum |term| per sum (`order_reference.sum_tolerance`), derived as in tests/test_gpu_verification.py, not measured.  Counts
and `invalid` are integers: ==.

Sizes: the 13 x 24 grid (G = 312) with handles that know their graph only.  (B, C) = (2, 6): 12 columns, up to 21 node
lanes per workgroup; (4, 82): W = 328 columns, more than one column tile and no multiple of one -- at M = 64 the
accumulators of a workgroup fill its LDS and the tiles narrow to 110 columns of one lane.  M in {2, 3, 8, 33, 50, 64}
covers every padded size of the sorting network."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import DerivedSpec, _lib, geometry, verification
from gencast_flax_nnx_amd.verification import EnsembleScores, OrderScores
from tests import derive_reference as DR
from tests import order_reference as R
from tests.helpers import graph_handle as _handle, small_graph as _graph

pytestmark = pytest.mark.gpu

PROBS = (0.0, 0.1, 0.5, 0.9, 1.0)


def _data(M, G, B, C, seed, scale=None):
  rng = np.random.default_rng(seed)
  scale = np.logspace(-3, 5, C) if scale is None else scale
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  return members, truth, w


def _push_all(nd, members, w=None):
  nd.ens_reserve(len(members))
  if w is not None:
    nd.ens_set_node_weight(w)
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _check_fields(tag, nd, ref):
  for q in range(ref["fields"].shape[0]):
    np.testing.assert_array_equal(nd.ens_order_quantile(q), ref["fields"][q], err_msg=f"{tag}: quantile field {q}")


def _check(tag, out, ref, G):
  """Sums within the bound (the worst ratio of error to bound is printed first), counts and invalid exact."""
  bins, extra, pinball, counts, invalid = out
  tol = R.sum_tolerance(ref, G)
  worst = 0.0
  for name, got in (("bins", bins), ("extra", extra), ("pinball", pinball)):
    assert got.shape == ref[name].shape and got.dtype == np.float64, f"{tag}: {name} {got.shape}"
    if got.size == 0:
      continue
    err = np.abs(got - ref[name])
    ratio = float(np.max(err / np.maximum(tol[name], 1e-300)))
    worst = max(worst, ratio)
    print(f"{tag} {name}: max |device - reference| {err.max():.3e}, worst ratio to (G + 8) 2^-53 sum|term| {ratio:.3f}")
  for name, got in (("bins", bins), ("extra", extra), ("pinball", pinball)):
    assert np.all(np.abs(got - ref[name]) <= tol[name]), f"{tag}: {name} outside (G + 8) 2^-53 sum|term|"
  assert counts.dtype == np.uint64
  np.testing.assert_array_equal(counts, ref["counts"], err_msg=f"{tag}: counts")
  assert invalid == ref["invalid"], f"{tag}: invalid"
  return worst


# ---- 1. every M ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 8, 33, 50, 64])
def test_every_member_count_matches_the_float64_definition(M):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w = _data(M, G, B, C, seed=M)
  ref = R.reference(members, truth, w, PROBS)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_order_set(PROBS)
    before = nd.ens_score(truth)
    out = nd.ens_order_score(None)                        # (the truth ens_score uploaded)
    assert out[0].shape == (B, C, M + 1, 2) and out[1].shape == (B, C, 3) and out[2].shape == (B, C, len(PROBS))
    assert out[3].shape == (B, C, len(PROBS) + 1)
    _check(f"tiny M={M}", out, ref, G)
    _check_fields(f"tiny M={M}", nd, ref)
    np.testing.assert_array_equal(nd.ens_order_quantile(0), members.min(axis=0))
    np.testing.assert_array_equal(nd.ens_order_quantile(len(PROBS) - 1), members.max(axis=0))
    assert nd.counter("ens_order_invalid_points") == 0 and nd.counter("ens_order_calls") == 1
    again = nd.ens_order_score(None)
    for x, y in zip(out[:4], again[:4]):
      assert x.tobytes() == y.tobytes()
    assert again[4] == out[4]
    _check_fields(f"tiny M={M}, second call", nd, ref)
    for i in range(M):                                    # the store is read, never written
      assert nd.ens_download_member(i).tobytes() == members[i].tobytes()
    after = nd.ens_score(None)
    for x, y in zip(before, after):
      assert x.tobytes() == y.tobytes()
    sc = OrderScores(*out[:4], M, PROBS)
    want = R.scores(ref, M)
    for name in ("reliability", "crps_potential", "crps_ensemble", "bin_width", "bin_frequency"):
      np.testing.assert_allclose(getattr(sc, name), want[name], rtol=1e-9, atol=0.0, err_msg=name)
  finally:
    nd.close()


# ---- 2. column tiling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [8, 64])
def test_more_columns_than_one_tile(M):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 4, 82
  members, truth, w = _data(M, G, B, C, seed=100 + M)
  ref = R.reference(members, truth, w, PROBS)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_order_set(PROBS)
    _check(f"W=328 M={M}", nd.ens_order_score(truth), ref, G)
    _check_fields(f"W=328 M={M}", nd, ref)
  finally:
    nd.close()


def test_two_equal_width_tiles_of_one_lane():
  """(B, C) = (1, 257): two column tiles of 129 and 128 columns, one node lane in the first and two in the second."""
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 1, 257, 3
  members, truth, w = _data(M, G, B, C, seed=257)
  ref = R.reference(members, truth, w, PROBS)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_order_set(PROBS)
    _check("W=257", nd.ens_order_score(truth), ref, G)
    _check_fields("W=257", nd, ref)
  finally:
    nd.close()


# ---- 3. ties and invalid points ---------------------------------------------------------------------------------------------
def test_ties_and_invalid_points():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, _ = _data(M, G, B, C, seed=21)
  w = (np.arange(G) % 7 + 1).astype(np.float32) / 8.0             # dyadic: their sums are exact in any order
  probs = (0.0, 0.25, 0.5, 1.0)
  two_equal, on_member, on_quantile, all_equal = np.array([0, 5, 77]), np.array([11, 200, G - 1]), np.array([20, 21, 99]), \
      np.array([30, 31, 250])
  nan_truth = np.array([3, 4, 150, 151, 152, 300])
  members[2, two_equal] = members[6, two_equal]
  truth[on_member] = members[3][on_member]
  members[:, all_equal] = members[0, all_equal]
  truth[all_equal[0]] = members[0, all_equal[0]]                  # the truth on a zero-width ensemble, too
  truth[nan_truth] = np.nan
  members[5, [9, 120], 1, 2] = np.nan
  members[5, 251, 1, 2] = np.inf
  members[6, 9, 0, 4] = -np.inf
  members[:, :, 1, 5] = np.nan                                    # a column that is wholly invalid
  members[:, 60:64, 0, 0] = np.float32(0.0)                       # members and truth of +-0.0
  members[::2, 60:64, 0, 0] = np.float32(-0.0)
  truth[60:62, 0, 0] = np.float32(-0.0)
  truth[62:64, 0, 0] = np.float32(0.0)
  fields = R.quantile_fields(members, probs)
  truth[on_quantile] = fields[1][on_quantile]                     # equal to the p = 0.25 field: not counted as below it
  truth[on_quantile, 1, 5] = np.float32(1.0)                      # (that column has no quantile: keep the truth finite)
  ref = R.reference(members, truth, w, probs)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_order_set(probs)
    out = nd.ens_order_score(truth)
    _check("ties", out, ref, G)
    _check_fields("ties", nd, ref)
    bins, extra, pinball, counts, invalid = out
    # what is counted, from first principles
    bad_member = np.zeros((G, B, C), bool)
    bad_member[[9, 120, 251], 1, 2] = True
    bad_member[9, 0, 4] = True
    bad_member[:, 1, 5] = True
    keep = ~bad_member
    keep[nan_truth] = False
    assert invalid == int((~keep).sum()) == nd.counter("ens_order_invalid_points")
    np.testing.assert_array_equal(counts[..., -1], keep.sum(0).astype(np.uint64))
    np.testing.assert_array_equal(extra[..., 0], (w.astype(np.float64)[:, None, None] * keep).sum(0))
    q1 = nd.ens_order_quantile(1)
    np.testing.assert_array_equal(np.isnan(q1), bad_member)       # NaN truth: the quantile is finite; a bad member: NaN
    assert np.isfinite(q1[nan_truth][~bad_member[nan_truth]]).all()
    # a truth equal to the quantile value is not below it
    below = (truth < fields[1]) & keep
    np.testing.assert_array_equal(counts[..., 1], below.sum(0).astype(np.uint64))
    assert not below[on_quantile][:, :, :5].any()
    # the wholly invalid column: zeros, no NaN
    assert np.isfinite(bins).all() and np.isfinite(extra).all() and np.isfinite(pinball).all()
    assert not bins[1, 5].any() and not extra[1, 5].any() and not pinball[1, 5].any() and not counts[1, 5].any()
    # a truth on a member is in no outlier bin; all members equal: every interior bin has zero width there
    sc = OrderScores(bins, extra, pinball, counts, M, probs)
    with np.errstate(invalid="ignore", divide="ignore"):
      assert np.isfinite(sc.reliability[keep.any(0)]).all()
  finally:
    nd.close()


# ---- 4. agreement with the existing scorer ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 50])
def test_crps_agrees_with_ens_score_on_the_same_store(M):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w = _data(M, G, B, C, seed=40 + M)
  members[1, 5:40] = members[0, 5:40]                             # ties between members
  truth[100:110] = members[M - 1, 100:110]
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_order_set(())
    sums, hist = nd.ens_score(truth)
    bins, extra, pinball, counts, _ = nd.ens_order_score(None)
    a = OrderScores(bins, extra, pinball, counts, M, ()).crps_ensemble
    b = EnsembleScores(sums, hist, M).crps_ensemble
    print(f"M={M}: max relative difference of the two ensemble CRPS {np.max(np.abs(a - b) / np.abs(b)):.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-9, atol=0.0)
    s0 = (w.astype(np.float64)[:, None, None] * np.ones((G, B, C))).sum(0)
    bound = ((G + 8) + (G + M * M + 8)) * 2.0 ** -53 * s0
    assert np.all(np.abs(extra[..., 0] - sums[..., 0]) <= bound)
    np.testing.assert_array_equal(counts[..., -1], hist.sum(-1))
  finally:
    nd.close()


# ---- 5. fields without truth and without weights ----------------------------------------------------------------------------
def test_fields_need_neither_truth_nor_weights():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 33
  members, truth, w = _data(M, G, B, C, seed=51)
  members[4, 17, 1, 3] = np.nan
  ref = R.reference(members, truth, w, PROBS)
  nd, scored = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members)                                        # no weights, no truth
    nd.ens_order_set(PROBS)
    nd.ens_order_fields()
    _check_fields("fields only", nd, ref)
    assert nd.counter("ens_order_calls") == 1
    with pytest.raises(_lib.GencastHipError, match="no node weights"):
      nd.ens_order_score(truth)
    _push_all(scored, members, w)
    scored.ens_order_set(PROBS)
    scored.ens_order_score(truth)
    for q in range(len(PROBS)):
      assert scored.ens_order_quantile(q).tobytes() == nd.ens_order_quantile(q).tobytes()
    # Q = 0: the sums alone
    scored.ens_order_set(())
    out = scored.ens_order_score(None)
    _check("Q = 0", out, R.reference(members, truth, w, ()), G)
    assert out[2].shape == (B, C, 0) and out[3].shape == (B, C, 1)
    with pytest.raises(ValueError, match="outside"):
      scored.ens_order_quantile(0)
    scored.ens_order_fields()                                     # nothing to form: still a call
  finally:
    nd.close()
    scored.close()


# ---- 6. state and argument errors -------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
  import ctypes
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w = _data(50, G, B, C, seed=61)
  lib = _lib.load_library()
  dp = ctypes.POINTER(ctypes.c_double)
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  nd = _handle(gr, B, C)
  try:
    half = np.array([0.5])
    assert lib.gc_ens_order_set(bare._h, 1, half.ctypes.data_as(dp)) == _lib.GC_ERR_STATE        # no graph
    assert lib.gc_ens_order_fields(bare._h) == _lib.GC_ERR_STATE
    # gc_ens_order_set: argument errors at the C ABI (the binding raises before the call)
    assert lib.gc_ens_order_set(nd._h, 9, np.zeros(9).ctypes.data_as(dp)) == _lib.GC_ERR_UNSUPPORTED
    assert lib.gc_ens_order_set(nd._h, -1, None) == _lib.GC_ERR_UNSUPPORTED
    assert lib.gc_ens_order_set(nd._h, 1, None) == _lib.GC_ERR_INVALID_ARGUMENT
    for bad in (np.nan, -0.25, 1.5, np.inf):
      assert lib.gc_ens_order_set(nd._h, 2, np.array([0.5, bad]).ctypes.data_as(dp)) == _lib.GC_ERR_INVALID_ARGUMENT
    for bad in ([0.5, np.nan], [-0.1], [1.01], np.zeros(9), np.zeros((2, 2))):
      with pytest.raises(ValueError):
        nd.ens_order_set(bad)
    # before any setting
    with pytest.raises(_lib.GencastHipError, match="ens_order_set"):
      nd.ens_order_score(truth)
    with pytest.raises(_lib.GencastHipError, match="ens_order_set"):
      nd.ens_order_quantile(0)
    bins, extra = np.empty((B, C, 9, 2)), np.empty((B, C, 3))
    assert lib.gc_ens_order_score(nd._h, None, bins.ctypes.data_as(dp), extra.ctypes.data_as(dp), None, None, None) == _lib.GC_ERR_STATE
    assert b"gc_ens_order_set" in lib.gc_last_error(nd._h)
    base = nd.counter("device_allocations")
    nd.ens_order_set((0.5,))
    held = nd.counter("device_allocations")
    assert held == base + 1
    for _ in range(3):                                            # replaced, not added
      nd.ens_order_set((0.25, 0.5, 0.75))
      assert nd.counter("device_allocations") == held
    nd.ens_order_set((0.5,))
    assert nd.counter("device_allocations") == held
    # no store; a slot unpushed; no weights; no truth
    assert lib.gc_ens_order_fields(nd._h) == _lib.GC_ERR_STATE and b"gc_ens_reserve" in lib.gc_last_error(nd._h)
    nd.ens_reserve(8)
    for i in range(7):
      nd.ens_push_host(i, members[i])
    with pytest.raises(_lib.GencastHipError, match="slot 7 has not been pushed"):
      nd.ens_order_fields()
    with pytest.raises(_lib.GencastHipError, match="slot 7 has not been pushed"):
      nd.ens_order_score(truth)
    nd.ens_push_host(7, members[7])
    with pytest.raises(_lib.GencastHipError, match="no node weights"):
      nd.ens_order_score(truth)
    nd.ens_set_node_weight(w)
    with pytest.raises(_lib.GencastHipError, match="no truth"):
      nd.ens_order_score(None)
    with pytest.raises(_lib.GencastHipError, match="no quantile fields"):
      nd.ens_order_quantile(0)                                    # nothing ran yet
    assert lib.gc_ens_order_score(nd._h, None, None, extra.ctypes.data_as(dp), None, None, None) == _lib.GC_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError, match="truth must be"):
      nd.ens_order_score(truth[:-1])
    out8 = nd.ens_order_score(truth)
    _check("M = 8", out8, R.reference(members[:8], truth, w, (0.5,)), G)
    for q in (-1, 1):
      with pytest.raises(ValueError, match="outside"):
        nd.ens_order_quantile(q)
    assert lib.gc_ens_order_download(nd._h, 0, None) == _lib.GC_ERR_INVALID_ARGUMENT
    # a new setting and a new store each invalidate the fields
    nd.ens_order_set((0.5,))
    with pytest.raises(_lib.GencastHipError, match="no quantile fields"):
      nd.ens_order_quantile(0)
    nd.ens_order_fields()
    nd.ens_order_quantile(0)
    # M from 8 to 50 through reserve and push, WITHOUT a new setting: lo, hi and f follow the current M
    work = nd.counter("device_allocations")
    nd.ens_reserve(50)
    with pytest.raises(_lib.GencastHipError, match="no quantile fields"):
      nd.ens_order_quantile(0)
    for i in range(50):
      nd.ens_push_host(i, members[i])
    ref50 = R.reference(members, truth, w, (0.5,))
    _check("M = 50 after M = 8", nd.ens_order_score(None), ref50, G)
    _check_fields("M = 50 after M = 8", nd, ref50)
    assert nd.counter("device_allocations") == work               # the work buffers were replaced, not added
    assert nd.counter("ens_order_calls") == 3
  finally:
    nd.close()
    bare.close()


# ---- 7. full-size grids, set_graph only -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["nano", "one_degree"])
def test_full_size(case):
  if case == "nano":
    gr, M, hw = _graph(73, 144, mesh_size=4, k_hop=8), 50, dict(latent=256, heads=4, ffw=2048)
  else:
    lat, lon = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0)
    gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=5, attention_k_hop=8)
    M, hw = 8, dict(latent=512, heads=4, ffw=2048)
  G, B, C = gr.num_grid_nodes, 1, 82
  assert G == (10512 if case == "nano" else 65160)
  members, truth, w = _data(M, G, B, C, seed=11, scale=np.logspace(-2, 4, C))
  probs = (0.1, 0.5, 0.9)
  ref = R.reference(members, truth, w, probs)
  nd = _handle(gr, B, C, **hw)
  try:
    _push_all(nd, members, w)
    nd.ens_order_set(probs)
    out = nd.ens_order_score(truth)
    print(f"{case}: ens_order_device_us {nd.counter('ens_order_device_us')}")
    # the regime: ord_blocks = min(ceil(G / (8 q)), min(1024, 2 * kOrdCuCount * per_cu)), W = 82, Q = 3.  nano, M = 50: a thread's
    # accumulators take 880 bytes, so 167 threads get a set (q = 2) and one workgroup fits a CU: ceil(10512 / 16) = 657 -> 512.
    # One degree, M = 8: 208 bytes, 256 threads (q = 3), three workgroups per CU: ceil(65160 / 24) = 2715 -> 1024.
    assert nd.counter("ens_order_blocks") == (512 if case == "nano" else 1024)
    _check(case, out, ref, G)
    _check_fields(case, nd, ref)
  finally:
    nd.close()


# ---- 8. a derived view --------------------------------------------------------------------------------------------------------
def test_a_derived_view_scores_the_derived_members():
  """Wind speed from two components, max-pooled, through `ScoredStore(plan=..., order=...)`.  The components are small
  multiples of 1/8, so u u + v v is exact in double and the norm is one correctly rounded square root on either side: the
  derived members of tests/derive_reference.py are then the device's, bit for bit (asserted), and full of ties."""
  from gencast_flax_nnx_amd import datasets
  n_lat, n_lon, B, M = 13, 24, 2, 8
  gr = _graph(n_lat, n_lon)
  G = gr.num_grid_nodes
  lat, lon = np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)
  dims = ("batch", "time", "lat", "lon")
  zeros = np.zeros((B, 1, n_lat, n_lon), np.float32)
  template0 = datasets.Dataset({name: datasets.Variable(dims, zeros) for name in ("t2m", "u10", "v10")},
                               {"lat": lat, "lon": lon})
  spec = DerivedSpec([("norm2", "wind10", "u10", "v10"), ("copy", "t2m")], pool="max", r_lat=1, r_lon=np.full(n_lat, 2))
  plan = spec.plan(template0)
  rng = np.random.default_rng(81)
  members = (rng.integers(-40, 41, (M, G, B, 3)) / 8.0).astype(np.float32)
  truth = (rng.integers(-40, 41, (G, B, 3)) / 8.0).astype(np.float32)
  members[3, 100, 1, 1] = np.nan                                  # a hole: the pooling skips it, the centre goes NaN
  w = verification.node_weights(template0)
  d_members, d_truth = DR.apply(members, plan), DR.apply(truth, plan)
  probs = (0.1, 0.5, 0.9)
  ref = R.reference(d_members, d_truth, w, probs)
  src, dst = _handle(gr, B, 3), _handle(gr, B, 2)
  try:
    _push_all(src, members)
    view = verification.ScoredStore(dst, M, w, plan=plan, source=src, order=probs)
    view.setup()
    view.score(truth)                                             # fills the view: members and truth, device to device
    got = view.score_order(None)
    for i in range(M):
      np.testing.assert_array_equal(dst.ens_download_member(i), d_members[i])
    _check("derived view", (got.bins, got.extra, got.pinball, got.counts, dst.counter("ens_order_invalid_points")), ref, G)
    assert got.n_members == M and got.probs == probs
    for q, f in enumerate(view.quantile_fields()):
      np.testing.assert_array_equal(f, ref["fields"][q])
    assert verification.ScoredStore(dst, M, w, plan=plan, source=src).score_order(None) is None
  finally:
    src.close()
    dst.close()
