"""Threshold-weighted CRPS on the device (gc_ens_tail_*) against the float64 definition restated in
tests/tail_reference.py.

Tolerance, derived and not measured: the per-point sums have at most M (M - 1) / 2 non-negative terms on either side, and the
node sums differ only in order, so |device - reference| <= (G + M (M - 1) / 2 + 8) 2^-53 sum |term| per sum
(`tail_reference.sum_tolerance`).  Counts and `invalid` are integers: ==.  Where two DEVICE results are compared (the
identities with gc_ens_score), each lies within its own bound of the exact value, so the bounds add.

Sizes: the 13 x 24 grid (G = 312) with handles that know their graph only.  (B, C) = (2, 6): 12 columns, 21 node lanes per
workgroup, two node-range blocks; (4, 82): W = 328 columns, two column tiles of 164 and one lane.  M in {2, 3, 4, 8, 16, 17,
33, 50, 64} covers every instance of the sorting network, padded and exactly full."""
import ctypes

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, verification
from gencast_flax_nnx_amd.verification import TailScores
from tests import tail_reference as R
from tests import verification_reference as VR
from tests.helpers import graph_handle as _handle, small_graph as _graph

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
NAN_TRUTH = np.array([3, 4, 150, 151, 152, 300])                  # nodes whose truth is NaN, in every column
ON_MEMBER, ON_TRUTH = np.array([11, 200, 311]), np.array([20, 21, 99])


def _directions(T):
  return tuple(+1 if t % 2 == 0 else -1 for t in range(T))


def _data(M, G, B, C, T, seed, dyadic=False):
  """Members, truth, weights and T threshold fields with everything the kernel has a branch for: a NaN block in the truth, a
  NaN and an inf in single members, a NaN threshold in channel 1 of the last t, thresholds bit-equal to a member and to the
  truth."""
  rng = np.random.default_rng(seed)
  scale = np.logspace(-3, 5, C)
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  w = ((np.arange(G) % 7 + 1).astype(np.float32) / 8.0 if dyadic        # dyadic: their sums are exact in any order
       else rng.uniform(0.1, 2.0, G).astype(np.float32))
  offset = np.linspace(-1.0, 1.5, T)[:, None, None, None]
  thr = ((rng.standard_normal((T, G, B, C)) * 0.5 + offset) * scale).astype(np.float32)
  thr[0, ON_MEMBER] = members[1, ON_MEMBER]
  thr[0, ON_TRUTH] = truth[ON_TRUTH]
  thr[T - 1, ON_MEMBER] = members[0, ON_MEMBER]
  members[1, 40:44] = members[0, 40:44]                           # ties between members
  truth[NAN_TRUTH] = np.nan
  members[M // 2, 9, 1, 2] = np.nan
  members[0, 120, 0, 4] = np.inf
  thr[T - 1, :, :, 1] = np.nan
  return members, truth, w, thr


def _push_all(nd, members, w=None):
  nd.ens_reserve(len(members))
  if w is not None:
    nd.ens_set_node_weight(w)
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _check(tag, out, ref, G, M):
  """Sums within the bound (the worst ratio of error to bound is printed first), counts and invalid exact."""
  sums, counts, invalid = out
  assert sums.shape == ref["sums"].shape and sums.dtype == np.float64, f"{tag}: sums {sums.shape}"
  tol = R.sum_tolerance(ref, G, M)
  err = np.abs(sums - ref["sums"])
  worst = 0.0
  for k, name in enumerate(("S0", "S1", "S2", "S3")):
    ratio = float(np.max(err[..., k] / np.maximum(tol[..., k], 1e-300)))
    worst = max(worst, ratio)
    print(f"{tag} {name}: max |device - reference| {err[..., k].max():.3e}, worst ratio to the bound {ratio:.3f}")
  assert np.all(err <= tol), f"{tag}: sums outside (G + M (M - 1) / 2 + 8) 2^-53 sum|term|"
  assert counts.dtype == np.uint64 and invalid.dtype == np.uint64
  np.testing.assert_array_equal(counts, ref["counts"], err_msg=f"{tag}: counts")
  np.testing.assert_array_equal(invalid, ref["invalid"], err_msg=f"{tag}: invalid")
  return worst


def _check_accounting(out, members, truth, thr, w, dyadic):
  """What is counted, from first principles: only (t = T - 1, c = 1) loses points to the NaN threshold."""
  sums, counts, invalid = out
  T, G, B, C = thr.shape
  keep = np.isfinite(truth) & np.isfinite(members).all(0)
  assert int((~keep).sum()) == NAN_TRUTH.size * B * C + 2
  for t in range(T):
    want = keep.copy()
    if t == T - 1:
      want[:, :, 1] = False
    np.testing.assert_array_equal(counts[t], want.sum(0).astype(np.uint64))
    assert int(invalid[t]) == int((~want).sum())
    if dyadic:                                                    # S0 and S3 are sums of dyadic numbers: exact in any order
      y, th = np.where(want, truth, 0), np.where(want, thr[t], 0)
      o = ((y > th) if t % 2 == 0 else (y < th)) & want
      np.testing.assert_array_equal(sums[t, ..., 0], (w.astype(np.float64)[:, None, None] * want).sum(0))
      np.testing.assert_array_equal(sums[t, ..., 3], (w.astype(np.float64)[:, None, None] * o).sum(0))
  assert int(invalid[T - 1]) == int((~keep).sum()) + int(keep[:, :, 1].sum()) and not counts[T - 1, :, 1].any()
  assert not sums[T - 1, :, 1].any() and np.isfinite(sums).all()


# ---- 1. every M ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 4, 8, 16, 17, 33, 50, 64])
def test_every_member_count_matches_the_float64_definition(M):
  gr = _graph()
  G, B, C, T = gr.num_grid_nodes, 2, 6, 3
  members, truth, w, thr = _data(M, G, B, C, T, seed=M, dyadic=True)
  dirs = _directions(T)
  ref = R.reference(members, truth, w, thr, dirs)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_tail_set(thr, dirs)
    before = nd.ens_score(truth)
    out = nd.ens_tail_score(None)                         # (the truth ens_score uploaded)
    assert out[0].shape == (T, B, C, 4) and out[1].shape == (T, B, C) and out[2].shape == (T,)
    _check(f"tiny M={M}", out, ref, G, M)
    _check_accounting(out, members, truth, thr, w, dyadic=True)
    assert nd.counter("ens_tail_invalid_points") == int(out[2].sum()) and nd.counter("ens_tail_calls") == 1
    again = nd.ens_tail_score(None)
    for x, y in zip(out, again):
      assert x.tobytes() == y.tobytes()
    for i in range(M):                                    # the store is read, never written
      assert nd.ens_download_member(i).tobytes() == members[i].tobytes()
    after = nd.ens_score(None)
    for x, y in zip(before, after):
      assert x.tobytes() == y.tobytes()
    sc = TailScores(out[0], out[1], M, dirs, out[2])
    want = R.scores(ref, M)
    ok = ref["sums"][..., 0] > 0
    for name in ("twcrps", "twcrps_ensemble", "abs_error", "pair_distance", "base_rate"):
      np.testing.assert_allclose(getattr(sc, name)[ok], want[name][ok], rtol=1e-9, atol=0.0, err_msg=name)
      assert np.isnan(getattr(sc, name)[~ok]).all()
  finally:
    nd.close()


# ---- 2. every T, mixed directions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,M", [(1, 8), (3, 17), (8, 17), (8, 64)])
def test_every_threshold_count(T, M):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w, thr = _data(M, G, B, C, T, seed=10 * T + M)
  dirs = _directions(T)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_tail_set(thr, dirs)
    out = nd.ens_tail_score(truth)
    _check(f"T={T} M={M}", out, R.reference(members, truth, w, thr, dirs), G, M)
    _check_accounting(out, members, truth, thr, w, dyadic=False)
  finally:
    nd.close()


# ---- 3. column tiling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,T", [(8, 8), (64, 2)])
def test_more_columns_than_one_tile(M, T):
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 4, 82
  members, truth, w, thr = _data(M, G, B, C, T, seed=100 + M)
  dirs = _directions(T)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_tail_set(thr, dirs)
    out = nd.ens_tail_score(truth)
    _check(f"W=328 M={M} T={T}", out, R.reference(members, truth, w, thr, dirs), G, M)
    _check_accounting(out, members, truth, thr, w, dyadic=False)
  finally:
    nd.close()


def test_two_equal_width_tiles_of_one_lane():
  """(B, C) = (1, 257): two column tiles of 129 and 128 columns, one node lane in the first and two in the second.  `_data`
  needs B >= 2, so the data here are plain: no special points but the NaN truth rows."""
  gr = _graph()
  G, B, C, M, T = gr.num_grid_nodes, 1, 257, 3, 2
  rng = np.random.default_rng(257)
  scale = np.logspace(-3, 5, C)
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  truth[NAN_TRUTH] = np.nan
  thr = (rng.standard_normal((T, G, B, C)) * 0.5 * scale).astype(np.float32)
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  dirs = _directions(T)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_tail_set(thr, dirs)
    _check("W=257", nd.ens_tail_score(truth), R.reference(members, truth, w, thr, dirs), G, M)
  finally:
    nd.close()


# ---- 4. identities on the device ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 50])
def test_identities_with_ens_score_on_the_same_store(M):
  """t0 = -FLT_MAX upper: nothing clamps, so S1 and S2 are gc_ens_score's sums 4 and 5.  t1 = +FLT_MAX upper: everything
  clamps to one value, S1 = S2 = S3 = 0.0 exactly.  t2 / t3: the upper and the lower tail at one finite threshold add up to
  the plain sums.  Two device results each lie within their own bound of the exact value, so the bounds add: the tail's
  (G + M (M - 1) / 2 + 8) 2^-53 sum|term| per tail result, gc_ens_score's (G + M^2 + 8) 2^-53 sum|term|
  (tests/verification_reference.py)."""
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  rng = np.random.default_rng(40 + M)
  scale = np.logspace(-3, 5, C)
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  members[1, 5:40] = members[0, 5:40]                             # ties between members
  truth[100:110] = members[M - 1, 100:110]
  finite = (rng.standard_normal((G, B, C)) * 0.7 * scale).astype(np.float32)
  finite[60:70] = members[0, 60:70]
  thr = np.stack([np.full((G, B, C), -FLT_MAX, np.float32), np.full((G, B, C), FLT_MAX, np.float32), finite, finite])
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_tail_set(thr, (+1, +1, +1, -1))
    plain, hist = nd.ens_score(truth)
    sums, counts, invalid = nd.ens_tail_score(None)
    assert not invalid.any()
    for t in range(4):
      np.testing.assert_array_equal(counts[t], hist.sum(-1))
    u = 2.0 ** -53
    f_tail, f_plain = (G + M * (M - 1) // 2 + 8) * u, (G + M * M + 8) * u
    for k_tail, k_plain in ((1, 4), (2, 5), (0, 0)):
      err = np.abs(sums[0, ..., k_tail] - plain[..., k_plain])
      bound = (f_tail + f_plain) * np.abs(plain[..., k_plain])
      print(f"M={M} -FLT_MAX sum {k_tail}: worst ratio to the bound {np.max(err / bound):.3f}")
      assert np.all(err <= bound)
    assert sums[0, ..., 3].tobytes() == sums[0, ..., 0].tobytes()         # every truth is above -FLT_MAX
    assert not sums[1, ..., 1:].any() and not np.signbit(sums[1, ..., 1:]).any()    # == 0.0, exactly
    np.testing.assert_array_equal(sums[1, ..., 0], sums[0, ..., 0])
    for k_tail, k_plain in ((1, 4), (2, 5)):
      both = sums[2, ..., k_tail] + sums[3, ..., k_tail]
      err = np.abs(both - plain[..., k_plain])
      bound = (2 * f_tail + f_plain + u) * np.abs(plain[..., k_plain])
      print(f"M={M} upper + lower sum {k_tail}: worst ratio to the bound {np.max(err / bound):.3f}")
      assert np.all(err <= bound)
    # the two base rates and the ties: y > thr, y < thr and y == thr partition the weight
    ties = (w.astype(np.float64)[:, None, None] * (truth == finite)).sum(0)
    np.testing.assert_allclose(sums[2, ..., 3] + sums[3, ..., 3] + ties, sums[2, ..., 0], rtol=(3 * G + 8) * u, atol=0.0)
  finally:
    nd.close()


# ---- 5. controls: the test can fail ----------------------------------------------------------------------------------------------
def test_controls_slot_order_one_changed_value_and_a_flipped_direction():
  gr = _graph()
  G, B, C, M, T = gr.num_grid_nodes, 2, 6, 8, 2
  members, truth, w, thr = _data(M, G, B, C, T, seed=71)
  thr[T - 1, :, :, 1] = thr[0, :, :, 1]                           # (no NaN threshold here: every column counts)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_tail_set(thr, (+1, -1))
    base = nd.ens_tail_score(truth)
    # two member slots swapped: the sort undoes it, every byte is the same
    nd.ens_push_host(2, members[5])
    nd.ens_push_host(5, members[2])
    swapped = nd.ens_tail_score(None)
    for x, y in zip(base, swapped):
      assert x.tobytes() == y.tobytes()
    # one member changed at one point: that column's sums change, no other column's
    g, b, c = 77, 1, 3
    changed = members[5].copy()
    changed[g, b, c] += np.float32(50.0 * np.logspace(-3, 5, C)[c])
    nd.ens_push_host(2, changed)
    one = nd.ens_tail_score(None)
    mask = np.zeros((T, B, C, 4), bool)
    mask[:, b, c, 1:3] = True                                     # S1 and S2 of both tails' column (b, c)
    differs = one[0] != base[0]
    assert differs[:, b, c, 1:3].any() and not differs[~mask].any()
    assert one[1].tobytes() == base[1].tobytes() and one[2].tobytes() == base[2].tobytes()
    want = members.copy()
    want[2], want[5] = changed, members[2]
    _check("one changed value", one, R.reference(want, truth, w, thr, (+1, -1)), G, M)
    # a flipped direction changes the result
    nd.ens_tail_set(thr, (+1, +1))
    flipped = nd.ens_tail_score(None)
    assert flipped[0][0].tobytes() == one[0][0].tobytes()
    assert (flipped[0][1, ..., 1:] != one[0][1, ..., 1:]).any(axis=-1).all()
    _check("flipped direction", flipped, R.reference(want, truth, w, thr, (+1, +1)), G, M)
  finally:
    nd.close()


# ---- 6. nothing else on the handle is touched -------------------------------------------------------------------------------------
def test_scores_and_event_tables_are_untouched_and_the_two_settings_are_independent():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w, thr = _data(M, G, B, C, 3, seed=81)
  ethr = thr[:2].copy()                                           # the events: T = 2, other directions
  wq, _ = verification.quantize_node_weights(w)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    nd.ens_event_set(ethr, (-1, +1), wq)
    score0, event0 = nd.ens_score(truth), nd.ens_event_score(None)
    nd.ens_tail_set(thr, (+1, -1, +1))
    tail0 = nd.ens_tail_score(None)
    score1, event1 = nd.ens_score(None), nd.ens_event_score(None)
    for before, after in ((score0, score1), (event0, event1)):
      for x, y in zip(before, after):
        assert x.tobytes() == y.tobytes()
    for i in range(M):
      assert nd.ens_download_member(i).tobytes() == members[i].tobytes()
    # a new event setting does not reach the tails, nor the other way round
    nd.ens_event_set(thr[:1] * np.float32(2.0), (+1,), wq)
    tail1 = nd.ens_tail_score(None)
    for x, y in zip(tail0, tail1):
      assert x.tobytes() == y.tobytes()
    nd.ens_event_set(ethr, (-1, +1), wq)
    nd.ens_tail_set(thr[:1], (-1,))
    nd.ens_tail_score(None)
    for x, y in zip(event0, nd.ens_event_score(None)):
      assert x.tobytes() == y.tobytes()
  finally:
    nd.close()


# ---- 7. state and argument errors, buffers ---------------------------------------------------------------------------------------
def test_state_and_argument_errors():
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth, w, thr = _data(50, G, B, C, 3, seed=61)
  dirs = (+1, -1, +1)
  lib = _lib.load_library()
  fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
  dp, up = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  nd = _handle(gr, B, C)
  try:
    thr9 = np.zeros((9, G, B, C), np.float32)
    d9 = np.ones(9, np.int32)
    sums = np.empty((3, B, C, 4))
    assert lib.gc_ens_tail_set(bare._h, 1, thr9.ctypes.data_as(fp), d9.ctypes.data_as(ip)) == _lib.GC_ERR_STATE      # no graph
    assert lib.gc_ens_tail_score(bare._h, None, sums.ctypes.data_as(dp), None, None) == _lib.GC_ERR_STATE
    # gc_ens_tail_set: argument errors at the C ABI (the binding raises before the call)
    assert lib.gc_ens_tail_set(nd._h, 9, thr9.ctypes.data_as(fp), d9.ctypes.data_as(ip)) == _lib.GC_ERR_UNSUPPORTED
    assert lib.gc_ens_tail_set(nd._h, 0, thr9.ctypes.data_as(fp), d9.ctypes.data_as(ip)) == _lib.GC_ERR_UNSUPPORTED
    assert lib.gc_ens_tail_set(nd._h, 1, None, d9.ctypes.data_as(ip)) == _lib.GC_ERR_INVALID_ARGUMENT
    assert lib.gc_ens_tail_set(nd._h, 1, thr9.ctypes.data_as(fp), None) == _lib.GC_ERR_INVALID_ARGUMENT
    d0 = np.array([1, 0], np.int32)
    assert lib.gc_ens_tail_set(nd._h, 2, thr9.ctypes.data_as(fp), d0.ctypes.data_as(ip)) == _lib.GC_ERR_INVALID_ARGUMENT
    assert b"direction 1 is zero" in lib.gc_last_error(nd._h)
    # before any setting
    with pytest.raises(_lib.GencastHipError, match="ens_tail_set"):
      nd.ens_tail_score(truth)
    assert lib.gc_ens_tail_score(nd._h, None, sums.ctypes.data_as(dp), None, None) == _lib.GC_ERR_STATE
    assert b"gc_ens_tail_set" in lib.gc_last_error(nd._h)
    base = nd.counter("device_allocations")
    nd.ens_tail_set(thr[:1], dirs[:1])
    held = nd.counter("device_allocations")
    assert held == base + 1
    for _ in range(3):                                            # replaced, not added
      nd.ens_tail_set(thr, dirs)
      assert nd.counter("device_allocations") == held
    nd.ens_tail_set(thr[:2], dirs[:2])
    nd.ens_tail_set(thr, dirs)
    assert nd.counter("device_allocations") == held
    # no store; a slot unpushed; no weights; no truth
    assert lib.gc_ens_tail_score(nd._h, None, sums.ctypes.data_as(dp), None, None) == _lib.GC_ERR_STATE
    assert b"gc_ens_reserve" in lib.gc_last_error(nd._h)
    nd.ens_reserve(8)
    for i in range(7):
      nd.ens_push_host(i, members[i])
    with pytest.raises(_lib.GencastHipError, match="slot 7 has not been pushed"):
      nd.ens_tail_score(truth)
    nd.ens_push_host(7, members[7])
    with pytest.raises(_lib.GencastHipError, match="no node weights"):
      nd.ens_tail_score(truth)
    nd.ens_set_node_weight(w)
    with pytest.raises(_lib.GencastHipError, match="no truth"):
      nd.ens_tail_score(None)
    assert lib.gc_ens_tail_score(nd._h, None, None, None, None) == _lib.GC_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError, match="truth must be"):
      nd.ens_tail_score(truth[:-1])
    assert nd.counter("ens_tail_calls") == 0
    out8 = nd.ens_tail_score(truth)
    ref8 = R.reference(members[:8], truth, w, thr, dirs)
    _check("M = 8", out8, ref8, G, 8)
    # counts and invalid may be NULL
    alone = np.empty((3, B, C, 4))
    assert lib.gc_ens_tail_score(nd._h, None, alone.ctypes.data_as(dp), None, None) == _lib.GC_OK
    assert alone.tobytes() == out8[0].tobytes()
    # M from 8 to 50 through reserve and push, WITHOUT a new setting: the thresholds survive gc_ens_reserve
    work = nd.counter("device_allocations")
    nd.ens_reserve(50)
    for i in range(50):
      nd.ens_push_host(i, members[i])
    _check("M = 50 after M = 8", nd.ens_tail_score(None), R.reference(members, truth, w, thr, dirs), G, 50)
    assert nd.counter("device_allocations") == work               # the work buffers do not depend on M
    # another T: the work buffers are made again by the scoring call, replaced and not added
    nd.ens_tail_set(thr[:2], dirs[:2])
    out2 = nd.ens_tail_score(None)
    _check("T = 2 after T = 3", out2, R.reference(members, truth, w, thr[:2], dirs[:2]), G, 50)
    assert nd.counter("device_allocations") == work
    assert nd.counter("ens_tail_calls") == 4 and nd.counter("ens_tail_device_us") >= 0
    assert nd.counter("ens_tail_invalid_points") == int(out2[2].sum())
  finally:
    nd.close()
    bare.close()
