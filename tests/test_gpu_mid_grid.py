"""Every ensemble unit on a grid where its node-range block cap bites: the 1.5 degree grid, 121 x 240, G = 29 040 nodes,
against the unit's own float64 reference (tests/*_reference.py) inside the unit's existing, derived bound (DESIGN.md
section 8t).  The small-grid tests (G = 312, 165) are careful about columns, members, NaN placement and ties; at those sizes
no pass reaches its workgroup cap, no grid-stride loop takes a second step and the fractions sums are never cut by their
byte budget.  Here they are, and every case ASSERTS the regime it ran in through the `<prefix>_blocks` counters: when a cap
is moved, the assertion fails and says that the case has to move with it.

Default shape (B, C, M) = (2, 82, 3): W = 164 columns, one node lane (q = 1) in a 256-wide column tile -- the smallest W at
which the 2048 and the 1024 caps bite at this G.  Below a cap a workgroup walks per = ceil(G / blocks) >= 8 q nodes; above it
per grows, blocks * per overshoots G by whole workgroups and the trailing ones have an empty node range:
  2048 workgroups (loss_reduce_blocks):  per = ceil(29040 / 2048) = 15, ceil(29040 / 15) = 1936 working, 112 empty;
  1024 (tail_blocks; energy at B K = 2):  per = 29, 1002 working, 22 empty;
  256 (fss_blocks; energy at B K = 8):    per = 114, 255 working, 1 empty.

Inputs that make a wrong node range visible: node weights uniform in [0.1, 2), so a node dropped or counted twice moves S0
by 0.1 or more where the bound is about G 2^-53 S0; and one NaN member value and one NaN truth value at each of the nodes of
`PLANTED` -- the first and the last node, the first node of the last non-empty workgroup of every geometry above, and nodes
that only the second step of a grid-stride loop reaches.  The invalid-point counters and the counts are integers: ==.

The references run on all columns but where a docstring states a subset.  No tuning variable is set."""
import functools
import time

import numpy as np
import pytest

from gencast_flax_nnx_amd import BandSpec, DerivedSpec, SphericalAnalysis, losses
from gencast_flax_nnx_amd.verification import efi_table, quantize_node_weights, quantize_row_weights
from oracle import gencast_oracle as O
from tests import band_reference as BR
from tests import derive_expr_reference as XR
from tests import derive_reference as DR
from tests import efi_reference as FR
from tests import event_reference as ER
from tests import feature_reference as TR
from tests import fss_reference as SR
from tests import helpers
from tests import multivar_reference as MR
from tests import region_reference as RR
from tests import tail_reference as LR
from tests import window_reference as WR
from tests.helpers import graph_handle as _handle

pytestmark = pytest.mark.gpu

N_LAT, N_LON = 121, 240
G = N_LAT * N_LON                                           # 29 040
B, C, M = 2, 82, 3
W = B * C                                                   # 164: q = 256 // 164 = 1
# 0 and G - 1; 15 * 1935, 29 * 1001, 114 * 254, 171 * 169, 227 * 127: the first node of the last non-empty workgroup at
# per = 15 (2048 workgroups), 29 (1024), 114 (256), 171 (170: the event table pass below) and 227 (128: the EFI table pass);
# 21 * 1024 = 21504 and 25000: reached by the second step of a grid-stride loop of 1024 workgroups with 21 node lanes (W = 12)
PLANTED = np.array([0, 21504, 25000, 28829, 28899, 28956, 29025, 29029, G - 1])
NAN_MEMBER, NAN_TRUTH = (1, 0, 3), (1, 80)                  # (slot, b, c) of the NaN member value, (b, c) of the NaN truth value
ROW = 60                                                    # the latitude row of the planted NaN row and the lone finite value


@functools.lru_cache(maxsize=None)
def _graph():
  gr = helpers.small_graph(N_LAT, N_LON)
  assert gr.num_grid_nodes == G
  return gr


def _latlon():
  return np.linspace(-90, 90, N_LAT), np.arange(N_LON) * (360.0 / N_LON)


def _plant(members, truth):
  members[NAN_MEMBER[0], PLANTED, NAN_MEMBER[1], NAN_MEMBER[2]] = np.nan
  truth[PLANTED, NAN_TRUTH[0], NAN_TRUTH[1]] = np.nan


@functools.lru_cache(maxsize=None)
def _data():
  """(members [M, G, B, C], truth [G, B, C], w [G]) float32, shared and read-only: channels over eight decades, ties between
  members and with the truth, the planted NaNs."""
  rng = np.random.default_rng(2904)
  scale = np.logspace(-3, 5, C).astype(np.float32)
  members = rng.standard_normal((M, G, B, C), dtype=np.float32) * scale
  truth = rng.standard_normal((G, B, C), dtype=np.float32) * scale
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  members[1, 40:44] = members[0, 40:44]                     # ties between members
  truth[50:54] = members[0, 50:54]                          # a member equal to the truth is not below it
  _plant(members, truth)
  for a in (members, truth, w):
    a.setflags(write=False)
  return members, truth, w


def _keep(members, truth):
  return np.isfinite(truth) & np.isfinite(members).all(0)


def _push_all(nd, members, w=None):
  nd.ens_reserve(len(members))
  if w is not None:
    nd.ens_set_node_weight(w)
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _within(tag, got, ref, tol):
  """|got - ref| <= tol everywhere; the worst ratio is printed first."""
  assert got.shape == ref.shape and got.dtype == np.float64, f"{tag}: {got.shape} {got.dtype}"
  err = np.abs(got - ref)
  print(f"{tag}: max |device - reference| {err.max():.3e}, worst ratio to the bound {float(np.max(err / np.maximum(tol, 1e-300))):.3f}")
  assert np.all(err <= tol), f"{tag}: outside the bound at {np.argwhere(err > tol)[:5].tolist()}"


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _timed:
  """Prints the wall time of a case (what DESIGN.md section 8t records)."""

  def __init__(self, tag):
    self.tag = tag

  def __enter__(self):
    self.t0 = time.perf_counter()

  def __exit__(self, *exc):
    print(f"{self.tag}: {time.perf_counter() - self.t0:.2f} s wall")


# ---- tail: the 1024 cap -------------------------------------------------------------------------------------------------------
def test_tail_above_its_1024_workgroup_cap():
  """T = 2, one upper and one lower tail.  tail_blocks = node_blocks(G, q = 1, 1024) = min(ceil(29040 / 8), 1024): per = 29,
  1002 working workgroups, 22 with an empty node range."""
  members, truth, w = _data()
  rng = np.random.default_rng(7)
  scale = np.logspace(-3, 5, C).astype(np.float32)
  thr = (rng.standard_normal((2, G, B, C), dtype=np.float32) * np.float32(0.5) + np.float32([[[[0.6]]], [[[-0.6]]]])) * scale
  thr[0, PLANTED[3]] = members[0, PLANTED[3]]               # a threshold bit-equal to a member
  dirs = (+1, -1)
  with _timed("tail"):
    ref = LR.reference(members, truth, w, thr, dirs)
    nd = _handle(_graph(), B, C)
    try:
      _push_all(nd, members, w)
      nd.ens_tail_set(thr, dirs)
      sums, counts, invalid = nd.ens_tail_score(truth)
      assert nd.counter("ens_tail_blocks") == 1024          # tail_blocks: the cap, not ceil(G / 8) = 3630
      np.testing.assert_array_equal(counts, ref["counts"], err_msg="counts")
      np.testing.assert_array_equal(invalid, ref["invalid"], err_msg="invalid")
      keep = _keep(members, truth)
      assert int((~keep).sum()) == 2 * PLANTED.size
      for t in range(2):                                    # from first principles: every point is counted or skipped, once
        np.testing.assert_array_equal(counts[t], keep.sum(0).astype(np.uint64))
        assert int(invalid[t]) == 2 * PLANTED.size
      assert nd.counter("ens_tail_invalid_points") == 2 * 2 * PLANTED.size
      _within("tail", sums, ref["sums"], LR.sum_tolerance(ref, G, M))
      again = nd.ens_tail_score(None)
      assert again[0].tobytes() == sums.tobytes() and again[1].tobytes() == counts.tobytes()
    finally:
      nd.close()


# ---- region: the plan's base capped at 2048 ----------------------------------------------------------------------------------
def _region_bits():
  """R = 3: rows 0-59, rows 40-120 but row 60, and the last node alone; row 60 is in no region.  Four atoms: bits 1 (rows
  0-39, 9600 nodes), 3 (rows 40-59, 4800), 2 (rows 61-120 less the last node, 14399), 6 (the last node)."""
  row = np.arange(G) // N_LON
  bits = np.zeros(G, np.uint32)
  bits[row < 60] |= 1
  bits[(row >= 40) & (row != ROW)] |= 2
  bits[G - 1] |= 4
  return bits, 3


def test_region_plan_with_its_base_capped_at_2048():
  """28 800 listed nodes: base = loss_reduce_blocks(28800, B, C) = min(2048, ceil(28800 / 8) = 3600) = 2048, per =
  ceil(28800 / 2048) = 15, and every atom of n_a nodes gets ceil(n_a / 15) table entries: 640 + 320 + 960 + 1 = 1921."""
  members, truth, w = _data()
  bits, R = _region_bits()
  with _timed("region"):
    ref = RR.reference(members, truth, w, bits, R)
    nd = _handle(_graph(), B, C)
    try:
      _push_all(nd, members, w)
      nd.ens_region_set(bits, R)
      sums, hist, invalid = nd.ens_region_score(truth)
      assert nd.counter("ens_region_blocks") == 1921        # 9600 / 15 + 4800 / 15 + ceil(14399 / 15) + 1
      np.testing.assert_array_equal(hist, ref["hist"], err_msg="hist")
      np.testing.assert_array_equal(invalid, ref["invalid"], err_msg="invalid")
      keep = _keep(members, truth)
      for r, idx in enumerate(RR.region_nodes(bits, R)):    # the histogram of a region sees the region's points, each once
        np.testing.assert_array_equal(hist[r].sum(-1), keep[idx].sum(0).astype(np.uint64))
        assert int(invalid[r]) == int((~keep[idx]).sum()) and int(invalid[r]) + int(hist[r].sum()) == idx.size * W
      assert [int(v) for v in invalid] == [2 * 1, 2 * 8, 2]  # PLANTED: node 0 | all but node 0 | the last node
      assert nd.counter("ens_region_invalid_points") == int(invalid.sum())
      _within("region", sums, ref["sums"], RR.sum_tolerance(ref, G, M))
    finally:
      nd.close()


# ---- events: the cap 1024 / (T tiles) ----------------------------------------------------------------------------------------
def test_event_tables_with_two_column_tiles_above_their_cap():
  """M = 9, not 3: a column's bins take (2 (M + 1) + 1) 12 = 252 bytes of the 40 KB of kEvtTableLds, so 162 columns fit a tile
  and W = 164 is cut into evt_tiles = 2 tiles of 82 (q = 3 node lanes); at M = 3 everything fits one tile.  T = 3:
  evt_node_blocks = node_blocks(G, 3, kEvtMaxWorkgroups / (T tiles) = 1024 / 6 = 170) = min(ceil(29040 / 24) = 1210, 170) = 170,
  per = 171, far above 8 q = 24.  Everything is an integer: ==."""
  M9, T = 9, 3
  with _timed("events"):
    members, truth, w, thr, d = ER.data(M9, G, B, C, seed=9, T=T)
    _plant(members, truth)
    thr[T - 1, PLANTED[4], 0, 7] = np.nan                   # a NaN threshold: not counted for that t alone
    wq, _ = quantize_node_weights(w)
    ref = ER.tables(members, truth, thr, d, wq)
    nd = _handle(_graph(), B, C)
    try:
      _push_all(nd, members)
      nd.ens_event_set(thr, d, wq)
      weighted, counts, invalid = nd.ens_event_score(truth)
      assert nd.counter("ens_event_blocks") == 170          # evt_node_blocks: 1024 // (3 thresholds * 2 tiles)
      np.testing.assert_array_equal(weighted, ref["weighted"], err_msg="weighted")
      np.testing.assert_array_equal(counts, ref["counts"], err_msg="counts")
      np.testing.assert_array_equal(invalid, ref["invalid"], err_msg="invalid")
      assert [int(v) for v in invalid] == [2 * PLANTED.size, 2 * PLANTED.size, 2 * PLANTED.size + 1]
      assert nd.counter("ens_event_invalid_points") == int(invalid.sum())
      for t in range(T):
        code = nd.ens_event_codes(t)
        np.testing.assert_array_equal(code, ref["code"][t], err_msg=f"code bytes of threshold {t}")
        skipped = (code == 255).sum(axis=0).astype(np.uint64)
        np.testing.assert_array_equal(counts[t].sum(axis=(-1, -2)) + skipped, np.full(skipped.shape, G, np.uint64))
    finally:
      nd.close()


# ---- EFI: the table pass above its cap, the index pass at 2048 ---------------------------------------------------------------
EFI_CHANNELS = np.array([0, 3, 17, 40, 41, 63, 80, 81])


def test_efi_table_pass_above_its_cap_and_index_pass_at_2048():
  """K = 3 samples, T = 2 events, E = 32 bins.  Table pass: a column's bins take (2 E + 1) 12 = 780 bytes of kEfiTableLds = 40 KB,
  52 columns fit, W = 164 is cut into 4 tiles of 41 (q = 6): efi_table_blocks = node_blocks(G, 6, kEfiMaxWorkgroups / (T tiles)
  = 1024 / 8 = 128) = min(ceil(29040 / 48) = 605, 128) = 128, per = 227.  Index pass: loss_reduce_blocks = 2048, 112 workgroups
  without nodes; gc_ens_efi_fields runs it alone.
  The device runs on all 164 columns.  The reference (its tables are filled point by point) runs on the 16 columns
  (b, c), b in {0, 1}, c in EFI_CHANNELS = {0, 3, 17, 40, 41, 63, 80, 81}: the first and the last column of every 41-wide tile
  of the table pass (c = 0, 40, 41, 81 in either b) and so of the one 256-wide tile of the index pass, and both columns
  that carry planted NaNs (c = 3, 80)."""
  members, truth, w = _data()
  rng = np.random.default_rng(33)
  scale = np.logspace(-3, 5, C).astype(np.float32)
  clim = rng.standard_normal((3, G, B, C), dtype=np.float32) * scale
  clim[2, PLANTED[3], 1, 17] = np.nan                       # a NaN sample, at the first node of the table pass's last workgroup
  wq, _ = quantize_node_weights(w)
  ranks, dirs, E, K = (2, 1), (+1, -1), 32, 3
  cs = EFI_CHANNELS
  with _timed("efi"):
    ref = FR.reference(members[..., cs], clim[..., cs], truth[..., cs], w, ranks, dirs, E, wq)
    nd, cl = _handle(_graph(), B, C), _handle(_graph(), B, C)
    try:
      _push_all(nd, members, w)
      _push_all(cl, clim)
      nd.ens_efi_set(ranks, dirs, E, wq)
      sums, weighted, counts, invalid = nd.ens_efi_score(cl, efi_table(K), truth)
      assert nd.counter("ens_efi_blocks") == 128            # efi_table_blocks: 1024 // (2 events * 4 tiles)
      assert invalid == 2 * PLANTED.size + 1 == nd.counter("ens_efi_invalid_points")     # over ALL columns
      assert ref["invalid"] == invalid                      # (the subset holds every column with an invalid point)
      efi, obs = nd.ens_efi_field(0), nd.ens_efi_field(1)
      assert int(np.isnan(efi).sum()) == invalid and int(np.isnan(obs).sum()) == invalid
      assert _bits(efi[..., cs]).tobytes() == _bits(ref["efi"]).tobytes(), "EFI field"
      assert _bits(obs[..., cs]).tobytes() == _bits(ref["observed"]).tobytes(), "observed index"
      np.testing.assert_array_equal(weighted[:, :, cs], ref["weighted"], err_msg="weighted")
      np.testing.assert_array_equal(counts[:, :, cs], ref["counts"], err_msg="counts")
      keep = _keep(members, truth) & np.isfinite(clim).all(0)
      for t in range(2):                                    # every column, from first principles: each valid point in one bin
        np.testing.assert_array_equal(counts[t].sum(axis=(-1, -2)), keep.sum(0).astype(np.uint64))
      _within("efi", sums[:, cs], ref["sums"], FR.tolerance(ref, G))
      # the index pass alone
      nd.ens_efi_fields(cl, efi_table(K))
      assert nd.counter("ens_efi_blocks") == 2048           # loss_reduce_blocks: kLossMaxBlocks, not ceil(G / 8) = 3630
      alone = nd.ens_efi_field(0)
      assert _bits(alone[..., cs]).tobytes() == _bits(FR.fields_only(members[..., cs], clim[..., cs])).tobytes()
      fin = np.isfinite(members).all(0) & np.isfinite(clim).all(0)
      np.testing.assert_array_equal(np.isnan(alone), ~fin)
      assert _bits(alone[keep]).tobytes() == _bits(efi[keep]).tobytes()
    finally:
      nd.close()
      cl.close()


# ---- variogram: 2048 ------------------------------------------------------------------------------------------------------------
def test_variogram_at_the_2048_workgroup_cap():
  """loss_reduce_blocks = 2048, per = 15, 112 workgroups without nodes.  Offsets across the wrap and across many rows, p = 0.5."""
  members, truth, w = _data()
  offsets = [(0, 1), (1, 0), (-3, 239), (60, 7)]
  with _timed("variogram"):
    ref = MR.variogram(members, truth, w, N_LAT, N_LON, offsets, 0.5)
    nd = _handle(_graph(), B, C)
    try:
      _push_all(nd, members, w)
      nd.ens_variogram_set(N_LAT, N_LON, offsets, 0.5)
      sums, counts = nd.ens_variogram_score(truth)
      assert nd.counter("ens_variogram_blocks") == 2048     # loss_reduce_blocks: kLossMaxBlocks
      np.testing.assert_array_equal(counts, ref["counts"], err_msg="counts")
      _within("variogram", sums, ref["sums"], MR.variogram_tolerance(ref, G, M))
    finally:
      nd.close()


# ---- energy: 2048 / (B K) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,blocks", [(1, 1024), (4, 256)])
def test_energy_above_its_cap_with_many_tiles_per_workgroup(K, blocks):
  """mv_energy_blocks = min(tiles, kMvMaxWorkgroups / (B K), G).  K = 1, one group over all 82 channels: 2048 / 2 = 1024
  node ranges of per = 29 nodes, 29 * 82 = 2378 points, ten tiles of 256 a workgroup (the last partial), 22 workgroups with
  no points at all.  K = 4, interleaved groups of 22, 20, 20 and 19 channels and channel 81 in none: 2048 / 8 = 256 node ranges
  of 114 nodes, up to 2508 points, ten tiles, one empty workgroup per (b, k).
  D2 within `energy_tolerance`.  The weights are uniform here, not dyadic, so S0 is held to the same derived bound and not to
  equality: its n = G |group| terms w a[c] are the same doubles on both sides (the scales are powers of two) and only the
  order of the additions differs, (n + 8) 2^-53 S0 -- a dropped node moves it by 0.1 / 8 at least, ten orders more."""
  members, truth, w = _data()
  if K == 1:
    group = np.zeros(C, np.int32)
  else:
    group = (np.arange(C) % 4).astype(np.int32)
    group[C - 1] = -1
    group[3] = 0                                            # (both planted columns in a group)
  scale = 2.0 ** np.random.default_rng(5).integers(-3, 4, C)
  with _timed(f"energy K={K}"):
    ref = MR.energy(members, truth, w, group, scale)
    assert ref["invalid"] == 2 * PLANTED.size
    nd = _handle(_graph(), B, C)
    try:
      _push_all(nd, members, w)
      nd.ens_energy_set(K, group, scale)
      d2, s0, invalid = nd.ens_energy_score(truth)
      assert nd.counter("ens_energy_blocks") == blocks      # mv_energy_blocks: 2048 // (B * K)
      assert invalid == ref["invalid"] == nd.counter("ens_energy_invalid_points")
      _within(f"energy K={K} D2", d2, ref["d2"], MR.energy_tolerance(ref))
      _within(f"energy K={K} S0", s0, ref["s0"], (ref["n"][None, :] + 8.0) * 2.0 ** -53 * ref["s0"])
      again = nd.ens_energy_score(None)
      assert again[0].tobytes() == d2.tobytes() and again[1].tobytes() == s0.tobytes()
    finally:
      nd.close()


# ---- fractions sums: the byte budget cuts the columns ----------------------------------------------------------------------------
FSS_COLUMNS = np.array([0, 2, 3, 4, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 162, 163])


def test_fss_chunks_cut_by_the_byte_budget():
  """S = 8 scales: a column of the work buffer takes 8 (S + 1) G = 2 090 880 bytes, kFssWorkBudget = 256 MiB holds 128 of them,
  so fss_chunk = 128 columns (four row tiles of 32), not the kFssMaxChunk = 256 every small grid gets: two chunks, the second with 36
  live columns of 128.  Column pass: fss_blocks = node_blocks(G, q = 256 / 128 = 2, kFssMaxBlocks = 256) = min(1815, 256) = 256,
  per = 114, one workgroup without nodes.  T = 1: the reference takes 3 s a threshold, and nothing here depends on T.
  The device runs on all 164 columns; so does the check of the code bytes.  The reference of the sums and fields runs on the
  16 columns FSS_COLUMNS (flat index b C + c): the first and the last column of every 32-wide row tile of either chunk (0, 31, 32, 63, 64, 95, 96, 127
  | 128, 159, 160, 163 -- so of either chunk too), the columns of the planted NaN row (2), the lone counted point (4) and the
  planted NaNs (3 = (0, 3), 162 = (1, 80))."""
  T, S = 1, 8
  members, truth, w = _data()
  truth = truth.copy()
  truth[ROW * N_LON:(ROW + 1) * N_LON, 0, 2] = np.nan       # one whole latitude row
  lone = truth[ROW * N_LON + 5, 0, 4]
  truth[:, 0, 4] = np.nan                                   # a counted centre, its whole window otherwise not counted
  truth[ROW * N_LON + 5, 0, 4] = lone
  scale = np.logspace(-3, 5, C)
  thr = np.ascontiguousarray(np.broadcast_to((np.array([-0.5])[:, None] * scale)[:, None, None, :], (T, G, B, C))).astype(np.float32)
  d = np.array([-1], np.int32)
  lat, lon = _latlon()
  cap = (N_LON - 1) // 2
  r_lats = np.array([0, 1, 2, 3, 5, 8, 13, 120], np.int32)
  r_lons = np.stack([np.zeros(N_LAT, np.int32), np.ones(N_LAT, np.int32), DerivedSpec.window(lat, lon, 500.0)[1],
                     np.full(N_LAT, 3, np.int32), DerivedSpec.window(lat, lon, 1500.0)[1], np.full(N_LAT, 8, np.int32),
                     np.full(N_LAT, 20, np.int32), np.full(N_LAT, cap, np.int32)]).astype(np.int32)
  row_wq = quantize_row_weights(losses.normalized_latitude_weights(lat))
  wq, _ = quantize_node_weights(w)
  with _timed("fss"):
    nd = _handle(_graph(), B, C)
    try:
      _push_all(nd, members)
      nd.ens_event_set(thr, d, wq)
      nd.ens_fss_set(r_lats, r_lons, row_wq)
      nd.ens_event_score(truth)
      code = np.stack([nd.ens_event_codes(t) for t in range(T)])
      np.testing.assert_array_equal(code, ER.tables(members, truth, thr, d, wq)["code"])
      sub = code.reshape(T, G, W)[:, :, FSS_COLUMNS]
      ref = SR.separable(sub, M, N_LAT, N_LON, r_lats, r_lons, row_wq, wq)
      sums = nd.ens_fss_score()
      assert nd.counter("ens_fss_chunks") == 2              # per threshold; fss_chunk: 256 MiB // (8 * 9 * 29040) = 128 columns of 164
      assert nd.counter("ens_fss_blocks") == 256            # fss_blocks: kFssMaxBlocks, not ceil(G / 16) = 1815
      assert sums.shape == (T, S, B, C, 4) and np.isfinite(sums).all()
      got = sums.reshape(T, S, W, 4)[:, :, FSS_COLUMNS]
      assert (ref["sums"] >= 0.0).all()
      _within("fss", got, ref["sums"], SR.bound(ref["sums"], G))
      for t, s in ((0, 0), (0, 2), (0, 4), (0, 7)):  # fields: ==, NaN pattern included
        prob, obs = nd.ens_fss_fields(t, s)
        np.testing.assert_array_equal(prob.reshape(G, W)[:, FSS_COLUMNS], ref["prob"][t, s], err_msg=f"prob t={t} s={s}")
        np.testing.assert_array_equal(obs.reshape(G, W)[:, FSS_COLUMNS], ref["obs"][t, s], err_msg=f"obs t={t} s={s}")
        assert (np.isnan(prob) == (code[t] == 255)).all() and (np.isnan(obs) == (code[t] == 255)).all()
        c = int(code[t, ROW * N_LON + 5, 0, 4])              # the lone centre sees itself only
        assert prob[ROW * N_LON + 5, 0, 4] == np.float32((c & 127) / M) and obs[ROW * N_LON + 5, 0, 4] == np.float32(c >> 7)
      assert (code[:, :, 0, 4] != 255).sum() == T
    finally:
      nd.close()


# ---- derive and derive-expr: the second trip of the grid-stride walk --------------------------------------------------------------
C_SRC, C_D = 12, 6                                          # W = B c_d = 12 derived columns: q = 21 node lanes


def _derive_fields(seed):
  """[M + 1, G, B, C_SRC]: M members, then the truth; the planted NaNs (channel 3 of slot 1, channel 11 of the truth), a NaN
  latitude row and a lone finite value in row 60, a constant channel."""
  members, truth = DR.data(M, G, B, C_SRC, seed)
  f = np.concatenate([members, truth[None]])
  f[1, PLANTED, 0, 3] = np.nan
  f[M, PLANTED, 1, C_SRC - 1] = np.nan
  f[:, ROW * N_LON:(ROW + 1) * N_LON, 0, 2] = np.nan        # one whole latitude row
  f[:, :, 0, 4] = np.nan                                    # a finite centre, every neighbour NaN
  f[:, ROW * N_LON + 5, 0, 4] = np.float32(2.5)
  f[:, :, B - 1, 5] = np.float32(7.25)                      # a constant field
  f[2, 21504 + 17, 1, 0] = np.inf
  return f


def _derived(dst, src, fields):
  _push_all(src, fields[:-1])
  dst.ens_derive(src, fields[-1])
  return np.stack([dst.ens_download_member(i) for i in range(len(fields) - 1)])


def test_derive_takes_a_second_grid_stride_trip():
  """launch_ens_derive: drv_point_blocks = min(1024, ceil(G / q)) with q = 256 / 12 = 21: ceil(29040 / 21) = 1383 > 1024, so
  the workgroups walk n += 1024 * 21 and the nodes from 21504 on are reached by a second step.  COPY moves the bits, NORM2 is
  within one float32 ulp (tests/test_gpu_derive.py).  The truth is checked through a slot, the fields rotated by one."""
  f = _derive_fields(seed=12)
  plan = dict(c_src=C_SRC, op=np.array([1, 0, 1, 0, 0, 1], np.int32), src_a=np.array([0, 3, 5, 11, 4, 2], np.int32),
              src_b=np.array([1, 0, 2, 0, 0, 9], np.int32),
              affine=np.array([[3.7, -12.5, 0.9, 4.0], [1, 0, 1, 0], [1e-3, 250.0, 41.0, -3e4], [1, 0, 1, 0], [1, 0, 1, 0],
                               [2.5, 0.0, -2.5, 1e-7]]), pool=0, n_lat=N_LAT, n_lon=N_LON)
  with _timed("derive"):
    src, dst = _handle(_graph(), B, C_SRC), _handle(_graph(), B, C_D)
    try:
      dst.ens_derive_set(**plan)
      dst.ens_reserve(M)
      for fields in (f, np.roll(f, -1, axis=0)):
        got = _derived(dst, src, fields)
        assert dst.counter("ens_derive_blocks") == 1024     # drv_point_blocks: the cap, not ceil(29040 / 21) = 1383
        ref = DR.apply(fields[:M], plan)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
        np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref))
        for j in np.flatnonzero(plan["op"] == 0):           # the copy channels: the bits
          np.testing.assert_array_equal(_bits(got[..., j]), _bits(fields[:M][..., plan["src_a"][j]]))
        ok = np.isfinite(ref)
        err = np.abs(got[ok].astype(np.float64) - ref[ok].astype(np.float64))
        assert np.all(err <= np.spacing(np.abs(ref[ok]))), "NORM2 beyond one float32 ulp"
        assert np.isnan(got[:, 21504:]).sum() == np.isnan(ref[:, 21504:]).sum() > 0     # NaNs the second trip must carry
    finally:
      src.close()
      dst.close()


def test_derive_expr_takes_a_second_grid_stride_trip():
  """launch_ens_derive_expr, the same geometry (1024 workgroups of 21 node lanes for 1383 node groups), with c_d = 6: copy,
  norm2, a sum of 37 terms, a norm of two lists, vorticity and divergence (both poles: the pole pass runs too), within the
  bound tests/derive_expr_reference.py computes from the inputs."""
  lat, lon = _latlon()
  rng = np.random.default_rng(12)
  scale, loc = rng.uniform(0.5, 2.0, C_SRC), rng.uniform(-1.0, 1.0, C_SRC)
  long_list = [(float(rng.uniform(-2.0, 2.0)), (5 * t + 2) % C_SRC, (3 * t + 1) % C_SRC if t % 2 else -1) for t in range(37)]
  wt = [float(v) for v in rng.uniform(0.1, 3.0, 5)]
  qu = [(wt[k], 2 + k, (7 + k) % C_SRC) for k in range(5)]
  qv = [(wt[k], 2 + k, (1 + 2 * k) % C_SRC) for k in range(5)]
  channels = [("copy", C_SRC - 1), ("norm2", 0, 1, (3.7, -12.5, 0.9, 4.0)), ("sum", long_list), ("norm", qu, qv),
              ("vorticity", 5, 6), ("divergence", 5, 6)]
  plan = XR.raw_plan(C_SRC, channels, N_LAT, N_LON, scale=scale, loc=loc, lat=lat, lon=lon)
  assert plan["pole_row"].sum() == 2
  members, truth = DR.data(M, G, B, C_SRC, 21)
  f = np.concatenate([members, truth[None]])
  f[1, PLANTED, 0, 3] = np.nan
  f[M, PLANTED, 1, C_SRC - 1] = np.nan
  f[0, ROW * N_LON:(ROW + 1) * N_LON, 0, 5] = np.nan        # u: one whole latitude row
  f[1, 1 * N_LON + 5, B - 1, 6] = np.nan                    # v: next to the first pole
  f[2, 25000, 0, 6] = -np.inf                               # v: in the interior, in the second trip
  with _timed("derive-expr"):
    ref, bound = XR.derive(f, plan)
    src, dst = _handle(_graph(), B, C_SRC), _handle(_graph(), B, C_D)
    try:
      dst.ens_derive_set(**plan)
      dst.ens_reserve(M)
      got = _derived(dst, src, f)
      assert dst.counter("ens_derive_blocks") == 1024       # drv_point_blocks: the cap, not ceil(29040 / 21) = 1383
      worst = [XR.within(got[..., j], ref[:M][..., j], bound[:M][..., j]) for j in range(1, C_D)]
      print(f"derive-expr: largest error / bound per channel {[f'{x:.2g}' for x in worst]}")
      np.testing.assert_array_equal(_bits(got[..., 0]), _bits(f[:M][..., C_SRC - 1]))
      rot = np.roll(f, -1, axis=0)                          # the former truth lies in the last slot now
      got = _derived(dst, src, rot)
      for j in range(1, C_D):
        XR.within(got[M - 1][..., j], ref[M][..., j], bound[M][..., j])
      np.testing.assert_array_equal(_bits(got[M - 1][..., 0]), _bits(f[M][..., C_SRC - 1]))
    finally:
      src.close()
      dst.close()


@pytest.mark.parametrize("pool", [DR.MAX, DR.MEAN])
def test_pooling_at_240_longitudes(pool):
  """Values only (the pooling passes have no cap): a copy plan of 6 channels (W = 12), r_lat = 2, r_lon the 500 km window -- 5
  columns at the equator, whole rows at the poles.  Row kernels at n_lon = 240: a row tile of 16 columns is staged by 256
  threads, 15 longitudes each; the column kernel runs over 29 040 * 12 points of each of the four fields.  MAX is ==, MEAN
  within `derive_reference.mean_bound`; the separable restatement is the yardstick (tests/test_derive.py holds it to the
  direct one)."""
  lat, lon = _latlon()
  r_lon = DerivedSpec.window(lat, lon, 500.0)[1]
  assert r_lon[0] == r_lon[-1] == (N_LON - 1) // 2 and r_lon[N_LAT // 2] == 2
  rw = np.asarray(losses.normalized_latitude_weights(lat), np.float64)
  f = _derive_fields(seed=30 + pool)[..., :C_D]
  plan = dict(c_src=C_D, op=np.zeros(C_D, np.int32), src_a=np.arange(C_D, dtype=np.int32), src_b=np.zeros(C_D, np.int32),
              affine=np.tile([1.0, 0.0, 1.0, 0.0], (C_D, 1)), pool=pool, n_lat=N_LAT, n_lon=N_LON, r_lat=2, r_lon=r_lon, row_weight=rw)
  with _timed(f"pool {pool}"):
    ref = DR.apply(f, plan, separable=True)
    src, dst = _handle(_graph(), B, C_D), _handle(_graph(), B, C_D)
    try:
      dst.ens_derive_set(**plan)
      dst.ens_reserve(M)
      for fields, want in ((f, ref[:M]), (np.roll(f, -1, axis=0), np.roll(ref, -1, axis=0)[:M])):   # rotated: the truth in a slot
        got = _derived(dst, src, fields)
        np.testing.assert_array_equal(np.isnan(got), ~np.isfinite(fields[:M]))
        assert np.all(got[:, ROW * N_LON + 5, 0, 4] == np.float32(2.5))          # every neighbour NaN: the centre itself
        if pool == DR.MAX:
          np.testing.assert_array_equal(got, want)
          assert np.all(got[:, :, B - 1, 5] == np.float32(7.25))
        else:
          bound = DR.mean_bound(fields[:M], want, N_LON)
          ok = np.isfinite(want)
          err = np.abs(got.astype(np.float64) - want)
          print(f"mean: worst error / bound {float((err[ok] / bound[ok]).max()):.3g}")
          assert np.all(err[ok] <= bound[ok])
    finally:
      src.close()
      dst.close()


# ---- gc_ens_push_state: the 1024 cap of launch_ens_state ----------------------------------------------------------------------------
def test_push_state_takes_a_second_grid_stride_trip():
  """launch_ens_state at W = B c_out = 12: min(1024, ceil(G / 21) = 1383) = 1024 workgroups that walk n += 1024 * 21 -- the
  nodes from 21504 on are written by a second step.  A gather, no arithmetic: the member is bit for bit the conditioning
  channels (or, where state_src < 0, the sample's) it was gathered from.  (No counter: the entry keeps no Meter.)  The
  handle needs weights and a sample for this entry; the tiny model of tests/helpers.py on this grid provides them."""
  with _timed("push_state"):
    gr, dims, params, x, _ = helpers.tiny_setup(batch=B, n_lat=N_LAT, n_lon=N_LON, layers=1)
    assert gr.num_grid_nodes == G and dims.c_out == C_D
    nd = helpers.make_native(gr, dims, params, B)
    try:
      slots = np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32)
      nd.set_noisy_slots(slots)
      x[PLANTED, 0, 3] = np.float32(-0.0)                   # a value whose bits a float comparison would not tell apart
      nd.upload_cond(x)
      nd.upload_noise(np.random.default_rng(5).standard_normal((G, B, dims.c_out)).astype(np.float32))
      nd.sample_resident(np.asarray(O.noise_schedule(80.0, 0.03, 3, 7.0), np.float32), skip_dead_call=True, want_stats=False)
      sample = nd.download_sample()
      state_src = np.array([0, 3, -1, 7, -1, 13], np.int32)
      nd.ens_reserve(2)
      nd.ens_push_state(1, state_src)
      got = nd.ens_download_member(1)
      want = np.where(state_src >= 0, x[..., np.maximum(state_src, 0)], sample)
      np.testing.assert_array_equal(_bits(got), _bits(want))
      assert np.ptp(got[21504:], axis=0).min() > 0          # (the second trip's nodes hold data, not one value)
    finally:
      nd.close()


# ---- band, window, feature: no cap of their own; each right once above 312 nodes ---------------------------------------------------
def test_band_view_at_121_by_240():
  """lmax = 12, three bands read by three source channels (c_d = 9), M = 2: `band_reference.check`, the derived bound of
  tests/test_gpu_band.py."""
  L, c_src, Mb = 12, 6, 2
  with _timed("band"):
    sa = SphericalAnalysis(*_latlon(), L)
    atabs, stabs = sa.device_tables(), sa.synthesis_tables()
    response, complement = BandSpec({"low": (0, 3), "mid": (4, 8), "high": dict(l=(0, 3), complement=True)}, taper=1).responses(L)
    plan = dict(c_src=c_src, response=response, complement=complement, src_channel=np.tile(np.array([0, 3, 5], np.int32), 3),
                band=np.repeat(np.arange(3, dtype=np.int32), 3), legendre_synthesis=stabs[0], cos_s=stabs[1], sin_s=stabs[2])
    rng = np.random.default_rng(17)
    scale = np.logspace(-3, 5, c_src)
    members = ((rng.standard_normal((Mb, G, B, c_src)) + 0.5) * scale).astype(np.float32)
    truth = ((rng.standard_normal((G, B, c_src)) + 0.5) * scale).astype(np.float32)
    ref = [BR.band_fields(x, N_LAT, N_LON, response, complement, plan["src_channel"], plan["band"], atabs, stabs)
           for x in list(members) + [truth]]
    src, dst = _handle(_graph(), B, c_src), _handle(_graph(), B, 9)
    try:
      _push_all(src, members)
      dst.spec_set_tables(*atabs)
      dst.ens_band_set(**plan)
      dst.ens_reserve(Mb)
      dst.ens_band(src, truth)
      assert dst.counter("ens_band_invalid_columns") == 0
      assert dst.counter("ens_band_blocks") == (G * B * 3 + 255) // 256     # the gather: one thread per value of the 3 distinct source channels
      for i in range(Mb):
        BR.check(dst.ens_download_member(i), ref[i][0], ref[i][1], f"121x240 member {i}")
      src.ens_push_host(0, truth)                           # the band truth has no download of its own: read back as a member
      dst.ens_band(src)
      BR.check(dst.ens_download_member(0), ref[Mb][0], ref[Mb][1], "121x240 truth")
    finally:
      src.close()
      dst.close()


@pytest.mark.parametrize("kind", ["mean", "max"])
def test_window_emit_at_29040_nodes(kind):
  """L = 3 of 4 pushes (the ring wraps), (B, C, M) = (2, 6, 2): the same IEEE operations in the same order as
  tests/window_reference.py, so bit equality (a NaN matches any NaN)."""
  Lw, n, Cw, Mw = 3, 4, 6, 2
  rng = np.random.default_rng(41)
  f = (rng.standard_normal((n, Mw + 1, G, B, Cw)) * np.logspace(-2, 3, Cw)).astype(np.float32)
  f[n - 1, 1, PLANTED, 0, 3] = np.nan
  f[1, 0, PLANTED, 1, 5] = np.nan
  f[0, :, PLANTED, 0, 0] = np.inf                           # (pushed out of the window by the fourth push)
  f[:, :, :, 0, 2] = rng.integers(-2, 3, (n, Mw + 1, G)).astype(np.float32)      # ties
  code, coef = WR.coefficients(kind, Lw)
  with _timed(f"window {kind}"):
    want = WR.window(WR.last(list(f), Lw), code, coef)
    src, win = _handle(_graph(), B, Cw), _handle(_graph(), B, Cw)
    try:
      src.ens_reserve(Mw)
      win.ens_reserve(Mw)
      win.ens_window_set(code, Lw, coef)
      for i in range(n):
        for m in range(Mw):
          src.ens_push_host(m, f[i, m])
        win.ens_window_push(src, f[i, Mw])
      win.ens_window_emit()
      got = np.stack([win.ens_download_member(m) for m in range(Mw)])
      assert WR.same_bits(got, want[:Mw]), f"{int((_bits(got) != _bits(want[:Mw])).sum())} of {got.size} words differ"
      assert np.isnan(got).sum() == 2 * PLANTED.size and not np.isinf(got).any()
      assert win.counter("ens_window_emits") == 1 and win.counter("ens_window_pushes") == n
    finally:
      src.close()
      win.close()


def test_feature_detection_at_121_by_240():
  """One minimum detector (r_lat = 1, r_lon = 2, a ring one wider, depth 0.5, a strike window) on a smooth field with ties,
  scattered NaNs and planted lows at j = 0, j = n_lon - 1 and in a pole row; (B, c_src, M) = (1, 2, 2).  Everything is a
  comparison: integer equality of counts and nodes, the bits of the values, == on the strike fields.  The gather has
  ceil(G / 256) = 114 workgroups (its grid-stride cap of 1024 needs more than 262 144 nodes)."""
  Bf, Cf, Mf = 1, 2, 2
  rng = np.random.default_rng(77)
  x = rng.standard_normal((N_LAT, N_LON, Mf + 1, Bf, Cf))
  for _ in range(2):
    x = (x + np.roll(x, 1, 0) + np.roll(x, -1, 0) + np.roll(x, 1, 1) + np.roll(x, -1, 1)) / 5.0
  f = np.moveaxis((np.round(x * 24.0) / 4.0).astype(np.float32).reshape(G, Mf + 1, Bf, Cf), 0, 1).copy()
  f[rng.integers(0, Mf + 1, 40), rng.integers(0, G, 40), 0, 1] = np.nan
  f[1, PLANTED, 0, 1] = np.nan
  f[:, 0 * N_LON + 5, :, 1] = np.float32(-50.0)             # a centre in a pole row
  f[:, ROW * N_LON + 0, :, 1] = np.float32(-40.0)           # a centre at j = 0
  f[:, (N_LAT - 3) * N_LON + N_LON - 1, :, 1] = np.float32(-45.0)     # a centre at j = n_lon - 1
  det = dict(channel=1, direction=-1, threshold=0.25, r_lat=1, r_lon=np.full(N_LAT, 2), ring_lat=2, ring_lon=np.full(N_LAT, 3),
             depth=0.5, strike_lat=1, strike_lon=np.full(N_LAT, 2))
  plan = TR.plan_of(Cf, N_LAT, N_LON, [det], max_centres=1024)
  with _timed("feature"):
    r_count, r_node, r_value, r_strike = TR.apply(f, plan)
    assert r_count.min() >= 3 and r_count.max() <= 1024
    src, dst = _handle(_graph(), Bf, Cf), _handle(_graph(), Bf, 1)
    try:
      dst.ens_reserve(Mf)
      dst.ens_feature_set(**plan)
      _push_all(src, f[:Mf])
      dst.ens_feature(src, f[Mf])
      assert dst.counter("ens_feature_blocks") == 114       # min(ceil(29040 / 256), 1024)
      count, node, value = dst.ens_feature_centres()
      got = np.stack([dst.ens_download_member(i) for i in range(Mf)])
      np.testing.assert_array_equal(count, r_count)
      np.testing.assert_array_equal(node, r_node)
      np.testing.assert_array_equal(_bits(value), _bits(r_value))
      np.testing.assert_array_equal(got, r_strike[:Mf])
    finally:
      src.close()
      dst.close()
