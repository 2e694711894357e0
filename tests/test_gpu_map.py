"""Score maps on the device (gc_ens_map_*) against tests/map_reference.py: the planes BYTE FOR BYTE,
the counts and the event planes with ==.  Graph-only handles on the 13 x 24 grid (G = 312) but for the one case above the
block cap, on the 1.5 degree grid of tests/test_gpu_mid_grid.py."""
import functools

import numpy as np
import pytest

from gencast_flax_nnx_amd import verification
from gencast_flax_nnx_amd.verification import EventMaps, EventScores, ScoreMaps, quantize_node_weights
from tests import event_reference as ER
from tests import helpers
from tests import map_reference as R
from tests import verification_reference as VR
from tests.helpers import graph_handle

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _graph(n_lat=13, n_lon=24):
  return helpers.small_graph(n_lat, n_lon)


G = 13 * 24


def _fields(M, B, C, seed, g=G, offset=0.0, spread=1.0):
  """(members [M, g, B, C], truth [g, B, C]) float32: channels over six decades."""
  rng = np.random.default_rng(seed)
  scale = np.logspace(-2, 4, C).astype(np.float32) if offset == 0.0 else np.ones(C, np.float32)
  members = (np.float32(offset) + np.float32(spread) * rng.standard_normal((M, g, B, C), dtype=np.float32)) * scale
  truth = (np.float32(offset) + np.float32(spread) * rng.standard_normal((g, B, C), dtype=np.float32)) * scale
  return members, truth


def _push(nd, members, reserve=True):
  if reserve:
    nd.ens_reserve(len(members))
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _accumulate(nd, dates, slot=0):
  """Every date into `slot`; -> the invalid-point counter after each."""
  invalid = []
  for k, (members, truth) in enumerate(dates):
    _push(nd, members, reserve=k == 0)
    nd.ens_map_accumulate(slot, truth)
    invalid.append(nd.counter("ens_map_invalid_points"))
  return invalid


def _same(tag, got, want):
  """The bytes; what differs is printed first."""
  got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
  assert got.shape == want.shape and got.dtype == want.dtype, f"{tag}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
  if got.tobytes() != want.tobytes():
    bad = np.argwhere(got.view(np.uint64 if got.dtype == np.float64 else got.dtype) != want.view(np.uint64 if want.dtype == np.float64 else want.dtype))
    raise AssertionError(f"{tag}: {len(bad)} of {got.size} values differ, first at {bad[:5].tolist()}: "
                         f"{got[tuple(bad[0])]!r} against {want[tuple(bad[0])]!r}")


def _check(nd, slot, dates, channels=None, tag=""):
  sums, counts, _, n = nd.ens_map_download(slot)
  ref_sums, ref_counts, ref_invalid = R.reference(dates, channels)
  _same(f"{tag} counts", counts, ref_counts)
  _same(f"{tag} sums", sums, ref_sums)
  assert n[0] == len(dates) and n[1] == 0
  return sums, counts, ref_invalid


# ---- 1. byte for byte -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 8, 33, 50, 64])
def test_three_dates_into_one_slot_byte_for_byte(M):
  """Every padded size of the register sort (2, 4, 8, 64) and the member counts that are no power of two; three dates, so the
  planes are a fold and not one addition."""
  B, C = 2, 3
  dates = [_fields(M, B, C, seed=100 * M + k) for k in range(3)]
  dates[1][0][M - 1, 5, 1, 2] = np.nan
  dates[2][1][G - 1, 0, 0] = np.nan
  nd = graph_handle(_graph(), B, C)
  try:
    nd.ens_map_set(None, 1)
    assert nd.counter("ens_map_bytes") == (6 * 8 + 3 * 4) * G * B * C
    invalid = _accumulate(nd, dates)
    sums, counts, ref_invalid = _check(nd, 0, dates, tag=f"M={M}")
    assert invalid == ref_invalid == [0, 1, 1]
    assert counts[0].max() == 3 and counts[0, 5, 1, 2] == 2 and counts[0, G - 1, 0, 0] == 2
    assert nd.counter("ens_map_calls") == 3 and nd.counter("ens_map_blocks") == (G + 41) // 42     # q = 256 // 6 node lanes
  finally:
    nd.close()


# ---- 2. channel subsets and column tiling ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,channels", [(2, 3, [1]), (2, 3, [0, 2]), (4, 82, [0, 3, 40, 41, 81]), (1, 257, None)])
def test_channel_subsets_and_more_than_one_column_tile(B, C, channels):
  """A NaN truth, a NaN member and an infinite member at points of the LAST selected column (and, at 257 columns, of the
  second column tile), and the same at unselected columns: those change nothing and are not counted as skipped."""
  M = 4
  members, truth = _fields(M, B, C, seed=B * C)
  sel = list(range(C)) if channels is None else channels
  last = sel[-1]
  truth[10, B - 1, last] = np.nan
  members[1, 20, B - 1, last] = np.nan
  members[M - 1, G - 1, B - 1, last] = np.inf
  planted = 3
  others = [c for c in range(C) if c not in sel]
  if others:
    truth[11, 0, others[0]] = np.nan
    members[0, 21, B - 1, others[-1]] = np.nan
    members[2, 0, 0, others[0]] = -np.inf
  nd = graph_handle(_graph(), B, C)
  try:
    nd.ens_map_set(channels, 1)
    invalid = _accumulate(nd, [(members, truth)])
    _, counts, ref_invalid = _check(nd, 0, [(members, truth)], channels, tag=f"B={B} C={C}")
    assert invalid == ref_invalid == [planted]
    assert int(counts[0].sum()) == G * B * len(sel) - planted
    if others:                                              # the same store without the values planted outside the selection
      clean_m, clean_t = _fields(M, B, C, seed=B * C)
      clean_t[..., sel], clean_m[..., sel] = truth[..., sel], members[..., sel]
      before = nd.ens_map_download(0)
      nd.ens_map_reset(0)
      assert _accumulate(nd, [(clean_m, clean_t)]) == [planted]
      after = nd.ens_map_download(0)
      assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
  finally:
    nd.close()


def test_bad_plans_are_refused_with_a_message_each():
  nd = graph_handle(_graph(), 2, 3)
  try:
    for channels, word in (([0, 3], "outside"), ([-1], "outside"), ([1, 0], "not above"), ([1, 1], "not above"), ([0, 1, 2, 2], "n_channels")):
      with pytest.raises(ValueError, match=word):
        nd.ens_map_set(channels, 1)
    for slots in (0, 129):
      with pytest.raises(ValueError, match="n_slots must be in 1..128"):
        nd.ens_map_set(None, slots)
    for T in (-1, 9):
      with pytest.raises(ValueError, match="n_event_thresholds must be in 0..8"):
        nd.ens_map_set(None, 1, T)
    nd.ens_map_set(None, 2)
    for slot in (-1, 2):
      with pytest.raises(ValueError, match="slot outside"):
        nd.ens_map_download(slot)
    with pytest.raises(ValueError, match="slot outside"):
      nd.ens_map_reset(-2)
  finally:
    nd.close()


# ---- 3. slots --------------------------------------------------------------------------------------------------------------
def test_slots_are_separate_and_reset_clears_one():
  M, B, C = 5, 2, 3
  dates = [_fields(M, B, C, seed=40 + k) for k in range(4)]
  dates[1][1][77, 1, 1] = np.nan                              # a NaN truth on one of slot 0's dates
  nd = graph_handle(_graph(), B, C)
  try:
    nd.ens_map_set(None, 3)
    _accumulate(nd, dates[:3], slot=0)
    nd.ens_map_accumulate(2, dates[3][1])                     # (the members of the third date are still in the store)
    _, counts, _ = _check(nd, 0, dates[:3], tag="slot 0")
    assert counts[0, 77, 1, 1] == 2 and int((counts[0] != 3).sum()) == 1
    sums1, counts1, _, n1 = nd.ens_map_download(1)
    assert not sums1.any() and not counts1.any() and not n1.any() and not np.signbit(sums1).any()
    two = [(dates[2][0], dates[3][1])]
    _check(nd, 2, two, tag="slot 2")
    nd.ens_map_reset(0)
    sums0, counts0, _, n0 = nd.ens_map_download(0)
    assert not sums0.any() and not counts0.any() and not n0.any()
    _check(nd, 2, two, tag="slot 2 after reset(0)")
    nd.ens_map_reset()
    assert not nd.ens_map_download(2)[0].any()
  finally:
    nd.close()


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------
def test_ties_between_members_and_with_the_truth():
  M, B, C = 8, 2, 3
  dates = []
  for k in range(2):
    members, truth = _fields(M, B, C, seed=60 + k)
    scale = np.logspace(-2, 4, C).astype(np.float32)
    members = np.round(members / scale * 2).astype(np.float32) / 2 * scale       # a grid of half a standard deviation
    truth = np.round(truth / scale * 2).astype(np.float32) / 2 * scale
    dates.append((members, truth))
  members, truth = dates[0]
  tie_truth = (members == truth[None]).any(axis=0)
  tie_members = (np.diff(np.sort(members, axis=0), axis=0) == 0).any(axis=0)
  assert tie_truth.mean() > 0.05 and tie_members.mean() > 0.05
  nd = graph_handle(_graph(), B, C)
  try:
    nd.ens_map_set(None, 1)
    _accumulate(nd, dates)
    _, counts, _ = _check(nd, 0, dates, tag="ties")
    assert counts[1].sum() > 0 and counts[2].sum() > 0
    # a truth equal to the lowest member: no member is below it (r == 0); equal to the highest: not all M are below it
    low, high = truth == members.min(axis=0), (truth == members.max(axis=0)) & (dates[1][1] <= dates[1][0].max(axis=0))
    assert low.any() and (counts[1][low] >= 1).all() and high.any() and (counts[2][high] == 0).all()
  finally:
    nd.close()


# ---- 5. a common offset ------------------------------------------------------------------------------------------------------
def test_members_with_a_common_offset():
  M, B, C = 50, 2, 3
  dates = [_fields(M, B, C, seed=70 + k, offset=1e4) for k in range(2)]
  assert all(abs(float(m.mean()) - 1e4) < 1.0 for m, _ in dates)
  nd = graph_handle(_graph(), B, C)
  try:
    nd.ens_map_set(None, 1)
    _accumulate(nd, dates)
    sums, counts, _ = _check(nd, 0, dates, tag="offset")
    assert (counts[0] == 2).all() and (sums[4] > 0.0).all()
    crps = ScoreMaps(sums, counts, M).crps
    assert (crps > 0.0).all() and float(crps.max()) < 10.0    # (of unit spread: not of the size of the offset)
  finally:
    nd.close()


# ---- 6. against gc_ens_score ---------------------------------------------------------------------------------------------------
def test_weighted_plane_sums_equal_the_column_sums_of_ens_score():
  """Dyadic node weights, so w * plane value is exact and the two sides differ in the order of the G additions of a column and
  in the form of ae and d alone: (G + M^2 + 8) 2^-53 A_k, A_k from the reference (section 8c's own bound)."""
  M, B, C = 8, 2, 3
  members, truth = _fields(M, B, C, seed=81)
  truth[5, 0, 1] = np.nan
  members[3, 100, 1, 2] = np.nan
  w = (2.0 ** np.random.default_rng(3).integers(-3, 3, G)).astype(np.float32)
  ref = VR.reference(members, truth, w)
  tol = VR.sum_tolerance(ref, G, M)
  nd = graph_handle(_graph(), B, C)
  try:
    _push(nd, members)
    nd.ens_set_node_weight(w)
    nd.ens_map_set(None, 1)
    nd.ens_map_accumulate(0, truth)
    col_sums, hist = nd.ens_score(None)
    sums, counts, _, _ = nd.ens_map_download(0)
    reg = ScoreMaps(sums, counts, M).region(w)
    for k in range(6):
      for name, got in (("map", reg.sums[..., k]), ("gc_ens_score", col_sums[..., k])):
        err = np.abs(got - ref["sums"][..., k])
        print(f"S{k} {name}: worst error / bound {float(np.max(err / np.maximum(tol[..., k], 1e-300))):.3f}")
        assert np.all(err <= tol[..., k]), f"S{k} of {name}"
      assert np.all(np.abs(reg.sums[..., k] - col_sums[..., k]) <= tol[..., k])
    assert np.array_equal(counts[0].sum(axis=0, dtype=np.uint64), hist.sum(axis=-1))
    assert np.array_equal(counts[1].sum(axis=0, dtype=np.uint64), hist[..., 0])
    assert np.array_equal(counts[2].sum(axis=0, dtype=np.uint64), hist[..., M])
    assert np.array_equal(reg.valid_points, hist.sum(axis=-1))
  finally:
    nd.close()


# ---- 7. event planes -----------------------------------------------------------------------------------------------------------
def test_event_planes_over_three_dates():
  M, B, C, T = 9, 2, 3, 2
  events_ref = np.zeros((T, 5, G, B, C), np.uint32)
  tables, dates = [], []
  nd = graph_handle(_graph(), B, C)
  try:
    for k in range(3):
      members, truth, w, thr, _ = ER.data(M, G, B, C, seed=90 + k, T=3)
      thr, d = thr[1:3], np.array([+1, -1], np.int32)         # an upper and a lower event
      truth[30 + k, 1, 0] = np.nan
      if k == 0:
        wq, scale = quantize_node_weights(w)
        nd.ens_event_set(thr, d, wq)
        nd.ens_map_set(None, 2, T)
        assert nd.counter("ens_map_bytes") == 2 * (6 * 8 + 3 * 4 + T * 5 * 4) * G * B * C
      _push(nd, members, reserve=k == 0)
      ref = ER.tables(members, truth, thr, d, wq)
      weighted, counts, invalid = nd.ens_event_score(truth)
      np.testing.assert_array_equal(weighted, ref["weighted"])
      nd.ens_map_accumulate_events(1)
      nd.ens_map_accumulate(1)                                # the truth already there
      R.accumulate_events(events_ref, ref["code"])
      tables.append(EventScores(weighted, counts, M, d, scale, invalid))
      dates.append((members, truth))
    sums, counts, events, n = nd.ens_map_download(1)
    assert events.dtype == np.uint32 and np.array_equal(events, events_ref) and n.tolist() == [3, 3]
    ref_sums, ref_counts, _ = R.reference(dates)
    _same("sums beside the events", sums, ref_sums)
    _same("counts beside the events", counts, ref_counts)
    assert np.array_equal(events[:, 0], np.broadcast_to(counts[0], events[:, 0].shape))     # (no NaN thresholds here)
    empty = nd.ens_map_download(0)
    assert not empty[2].any() and empty[3].tolist() == [0, 0]
    maps = EventMaps(events, M, d)
    merged = EventScores.merge(tables)
    got = maps.region(wq)["brier"]
    ulps = np.abs(got - merged.brier) / np.spacing(merged.brier)
    print(f"brier of the planes against the tables': worst {float(ulps.max()):.2f} ulp")
    assert np.all(ulps <= 8.0)
  finally:
    nd.close()


# ---- 8. leaves its neighbours alone ----------------------------------------------------------------------------------------------
def _neighbours(nd, M):
  return ([nd.ens_download_member(i).tobytes() for i in range(M)] + [a.tobytes() for a in nd.ens_download_fields()]
          + [nd.ens_event_codes(0).tobytes(), nd.ens_order_quantile(0).tobytes()] + [a.tobytes() for a in nd.ens_score(None)])


def _sequence(members, truth, thr, wq, w):
  """One fixed sequence of calls on a fresh handle -> (the neighbours before, after, the planes, allocations seen)."""
  M, _, B, C = members.shape
  nd = graph_handle(_graph(), B, C)
  try:
    _push(nd, members)
    nd.ens_set_node_weight(w)
    nd.ens_event_set(thr, (+1,), wq)
    nd.ens_order_set([0.5])
    nd.ens_score(truth, want_fields=True)
    nd.ens_event_score(None)
    nd.ens_order_score(None)
    fresh = nd.counter("device_allocations")
    nd.ens_map_set([0, 2], 2, 1)
    allocs = [nd.counter("device_allocations")]
    before = _neighbours(nd, M)
    nd.ens_map_accumulate(0)
    nd.ens_map_accumulate_events(0)
    nd.ens_map_accumulate(1, truth)
    after = _neighbours(nd, M)
    planes = [a.tobytes() for a in nd.ens_map_download(0)[:3]]
    nd.ens_map_set([0, 2], 2, 1)
    nd.ens_map_set(None, 3, 0)
    allocs.append(nd.counter("device_allocations"))
    assert not nd.ens_map_download(0)[0].any()                # a repeated set zeroes
    nd.ens_reserve(M)                                         # the accumulators are not the store's
    allocs.append(nd.counter("device_allocations"))
    return before, after, planes, allocs, fresh
  finally:
    nd.close()


def test_an_accumulate_changes_nothing_else_and_repeats_to_the_byte():
  M, B, C = 6, 2, 3
  members, truth, w, thr, _ = ER.data(M, G, B, C, seed=5, T=1)
  truth[9, 0, 2] = np.nan
  wq, _ = quantize_node_weights(w)
  before, after, planes, allocs, fresh = _sequence(members, truth, thr, wq, w)
  assert before == after
  assert allocs[0] == allocs[1] == allocs[2] == fresh + 5     # sums, counts, events, the skipped words, the channel list
  again = _sequence(members, truth, thr, wq, w)
  assert again[2] == planes and again[1] == after


# ---- 10. above the block cap -----------------------------------------------------------------------------------------------------
def test_above_the_block_cap_on_the_one_and_a_half_degree_grid():
  """121 x 240, G = 29 040; (B, C) = (6, 4) with two channels selected: Ws = 12 selected columns, q = 256 // 12 = 21 node lanes,
  ceil(29040 / 21) = 1383 workgroups wanted, kMapMaxBlocks = 1024 given: the workgroups stride by 1024 * 21 = 21 504 nodes and
  the nodes from there on are reached by a second step.  NaNs at the first and last node, on either side of the stride and
  in an unselected channel."""
  n_lat, n_lon = 121, 240
  g, M, B, C, channels = n_lat * n_lon, 8, 6, 4, [1, 3]
  members, truth = _fields(M, B, C, seed=29, g=g)
  planted = [0, 21503, 21504, 25000, g - 1]
  truth[planted, 0, 1] = np.nan
  members[5, planted, B - 1, 3] = np.nan
  members[0, planted, 2, 0] = np.nan                          # not selected
  nd = graph_handle(_graph(n_lat, n_lon), B, C)
  try:
    nd.ens_map_set(channels, 1)
    invalid = _accumulate(nd, [(members, truth)])
    assert nd.counter("ens_map_blocks") == 1024               # map_blocks: the cap, not ceil(29040 / 21) = 1383
    sums, counts, _, _ = nd.ens_map_download(0)
    ref_sums, ref_counts, ref_invalid = R.reference([(members, truth)], channels)
    _same("1.5 degree counts", counts, ref_counts)
    _same("1.5 degree sums", sums, ref_sums)
    assert invalid == ref_invalid == [2 * len(planted)]
    assert int(counts[0].sum()) == g * B * 2 - 2 * len(planted) and counts[0, 21504:].sum() > 0
  finally:
    nd.close()
