"""The Extreme Forecast Index on the device (gc_ens_efi_*) against the float64 definition restated
in tests/efi_reference.py.

What is exact: both fields (byte for byte, NaNs included), the integer tables, the counts and `invalid` -- the device does
the reference's IEEE operations in the reference's order.  The six column sums: both sides hold identical per-point doubles
and only the order of the G additions differs, so |device - reference| <= (G + 8) 2^-53 sum |term| (`efi_reference.tolerance`:
the bound of section 8c, derived, not tuned); the worst ratio is printed.

Sizes: the 13 x 24 grid (G = 312) with handles that know their graph only.  (B, C) = (2, 3): 6 columns, 42 node lanes per
workgroup.  The (M, K) pairs cover every padded size of K (2, 4, 8, 32, 64), K < M and M < K, and sizes that are no power of
two.  W = 328 = 256 + 72: two column tiles of the index pass and seven of the table pass; W = 257: a one-column tile."""
import ctypes

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib
from gencast_flax_nnx_amd.verification import EfiScores, efi_table, quantize_node_weights
from tests import efi_reference as R
from tests.helpers import graph_handle as _handle, small_graph as _graph

pytestmark = pytest.mark.gpu


def _data(M, K, G, B, C, seed, grid=None):
  """Members drawn around the truth, samples around the climate; `grid`: every value rounded to multiples of it, so that
  members, samples and truth coincide often (precipitation-like ties)."""
  rng = np.random.default_rng(seed)
  scale, offset = np.logspace(-2, 3, C), np.linspace(0.0, 300.0, C)
  clim = offset + rng.standard_normal((K, G, B, C)) * scale
  truth = offset + rng.standard_normal((G, B, C)) * scale
  members = truth + 0.7 * rng.standard_normal((M, G, B, C)) * scale
  if grid is not None:
    clim, truth, members = (np.round((x - offset) / (grid * scale)) * (grid * scale) + offset for x in (clim, truth, members))
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  return members.astype(np.float32), clim.astype(np.float32), truth.astype(np.float32), w


def _push_all(nd, fields, w=None):
  nd.ens_reserve(len(fields))
  if w is not None:
    nd.ens_set_node_weight(w)
  for i, x in enumerate(fields):
    nd.ens_push_host(i, x)


def _same_bytes(a, b, what):
  assert a.dtype == b.dtype and a.shape == b.shape, what
  assert a.tobytes() == b.tobytes(), f"{what}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} values differ"


def _check(tag, nd, out, ref, G):
  """Fields byte for byte, tables and invalid exact, sums within the bound (the worst ratio is printed first)."""
  sums, weighted, counts, invalid = out
  tol = R.tolerance(ref, G)
  err = np.abs(sums - ref["sums"])
  ratio = np.max(err / np.maximum(tol, 1e-300), axis=(0, 1))
  print(f"{tag}: worst |device - reference| / bound per sum " + " ".join(f"{n}={r:.3f}" for n, r in zip(R.NAMES, ratio)))
  _same_bytes(nd.ens_efi_field(0), ref["efi"], f"{tag}: EFI field")
  _same_bytes(nd.ens_efi_field(1), ref["observed"], f"{tag}: observed index")
  np.testing.assert_array_equal(weighted, ref["weighted"], err_msg=f"{tag}: weighted")
  np.testing.assert_array_equal(counts, ref["counts"], err_msg=f"{tag}: counts")
  assert invalid == ref["invalid"] == nd.counter("ens_efi_invalid_points"), f"{tag}: invalid"
  assert np.isfinite(sums).all(), f"{tag}: a sum is not finite"
  for k, name in enumerate(R.NAMES):
    assert np.all(err[..., k] <= tol[..., k]), f"{tag}: {name} outside (G + 8) 2^-53 sum|term|"


def _run(tag, members, clim, truth, w, ranks, dirs, E, B, C, gr=None, check=True):
  gr = _graph() if gr is None else gr
  G, K = gr.num_grid_nodes, len(clim)
  wq, _ = quantize_node_weights(w)
  nd, cl = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)                                    # the climatology handle needs neither weights nor truth
    nd.ens_efi_set(ranks, dirs, E, wq)
    out = nd.ens_efi_score(cl, efi_table(K), truth)
    ref = R.reference(members, clim, truth, w, ranks, dirs, E, wq)
    if check:
      _check(tag, nd, out, ref, G)
    return out, ref, nd.ens_efi_field(0), nd.ens_efi_field(1)
  finally:
    nd.close()
    cl.close()


# ---- 1. every padding of K, members streamed past ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(2, 2), (3, 8), (8, 3), (33, 5), (5, 33), (50, 30), (64, 64)])
def test_every_member_and_sample_count_matches_the_definition(M, K):
  G, B, C = 312, 2, 3
  members, clim, truth, w = _data(M, K, G, B, C, seed=100 * M + K)
  hi, lo = int(np.ceil(0.9 * K - 1e-9)), int(np.floor(0.1 * K + 1e-9))
  out, ref, efi, _ = _run(f"M={M} K={K}", members, clim, truth, w, (hi, lo), (+1, -1), 20, B, C)
  sc = EfiScores(out[0], out[1], out[2], M, K, (hi, lo), (+1, -1), quantize_node_weights(w)[1], out[3])
  assert np.all(np.abs(efi) <= 1.0) and sc.sums.shape == (B, C, 6)
  assert np.all(sc.correlation > 0.3)                      # (the members were drawn around the truth)
  assert np.all(sc.roc_area[(ref["counts"][:, :, :, 1].sum(-1) > 0) & (ref["counts"][:, :, :, 0].sum(-1) > 0)] > 0.5)


# ---- 2. ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(8, 8), (5, 33)])
def test_values_on_a_coarse_grid_tie_often(M, K):
  G, B, C = 312, 2, 3
  members, clim, truth, w = _data(M, K, G, B, C, seed=9 + M, grid=0.5)
  assert (members[0] == clim[0]).mean() > 0.05 and (truth == clim[1]).mean() > 0.05
  _, ref, _, _ = _run(f"ties M={M} K={K}", members, clim, truth, w, (K // 2, K // 2), (+1, -1), 8, B, C)
  assert (ref["le_y"] != ref["lt_y"]).mean() > 0.3         # the truth ties with a sample at many points


# ---- 3. column tiling, and a NaN of each kind in the last tile ------------------------------------------------------------
@pytest.mark.parametrize("B,C,M,K", [(4, 82, 8, 8), (1, 257, 3, 3)])
def test_more_columns_than_one_tile_with_invalid_points_in_the_last(B, C, M, K):
  G = 312
  members, clim, truth, w = _data(M, K, G, B, C, seed=7 * C)
  members[1, 17, B - 1, C - 1] = np.nan                    # one of each in the last column tile
  clim[2, 100, B - 1, C - 2 if C == 82 else C - 1] = np.nan
  truth[311, B - 1, C - 1] = np.nan
  members[0, 5, 0, 0] = np.inf                             # an infinite member ranks above the padding too: not counted
  clim[0, 6, 0, 1] = -np.inf
  out, ref, efi, obs = _run(f"W={B * C}", members, clim, truth, w, (K - 1, 1), (+1, -1), 20, B, C)
  assert out[3] == 5
  for g, b, c in ((17, B - 1, C - 1), (311, B - 1, C - 1), (5, 0, 0), (6, 0, 1)):
    assert np.isnan(efi[g, b, c]) and np.isnan(obs[g, b, c])
  assert np.isnan(efi).sum() == 5


# ---- 4. the extremes of T and E ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ranks,dirs,E", [((), (), 2), ((0, 1, 7, 8), (-1, +1, -1, +1), 32), ((4,), (+1,), 2), ((), (), 32)])
def test_no_events_four_events_two_bins_thirty_two_bins(ranks, dirs, E):
  G, B, C, M, K = 312, 2, 3, 5, 8
  members, clim, truth, w = _data(M, K, G, B, C, seed=E + len(ranks))
  out, ref, _, _ = _run(f"T={len(ranks)} E={E}", members, clim, truth, w, ranks, dirs, E, B, C)
  assert out[1].shape == (len(ranks), B, C, 2, E)
  for t in range(len(ranks)):
    assert out[2][t].sum() == G * B * C                    # every point lands in one bin of every event


# ---- 5. the truth-free entry, invariances, determinism -----------------------------------------------------------------------
def test_truth_free_entry_invariances_and_determinism():
  gr = _graph()
  G, B, C, M, K = gr.num_grid_nodes, 2, 3, 8, 5
  members, clim, truth, w = _data(M, K, G, B, C, seed=55)
  clim[1, 40, 1, 2] = np.nan
  truth[7, 0, 0] = np.nan                                  # the truth-free entry does not look at it
  wq, _ = quantize_node_weights(w)
  a = efi_table(K)
  nd, cl = _handle(gr, B, C), _handle(gr, B, C)
  try:
    _push_all(nd, members, w)
    _push_all(cl, clim)
    nd.ens_efi_set((4, 1), (+1, -1), 20, wq)
    first = nd.ens_efi_score(cl, a, truth)
    efi, obs = nd.ens_efi_field(0), nd.ens_efi_field(1)
    held, held_c = nd.counter("device_allocations"), cl.counter("device_allocations")
    again = nd.ens_efi_score(cl, a, None)                  # the truth is on the device
    for x, y in zip(first[:3], again[:3]):
      assert x.tobytes() == y.tobytes()
    assert first[3] == again[3] == 2 and nd.ens_efi_field(0).tobytes() == efi.tobytes()
    assert nd.counter("device_allocations") == held and cl.counter("device_allocations") == held_c
    # the truth-free entry: the same EFI bytes wherever the truth is finite, and a value where only the truth is not
    nd.ens_efi_fields(cl, a)
    free = nd.ens_efi_field(0)
    _same_bytes(free, R.fields_only(members, clim), "truth-free EFI")
    keep = np.isfinite(truth)
    assert free[keep].tobytes() == efi[keep].tobytes() and np.isfinite(free[7, 0, 0]) and np.isnan(free[40, 1, 2])
    with pytest.raises(_lib.GencastHipError, match="no observed index on the device"):
      nd.ens_efi_field(1)
    assert nd.counter("ens_efi_calls") == 3 and nd.counter("ens_efi_device_us") >= 0
    for i in range(M):
      assert nd.ens_download_member(i).tobytes() == members[i].tobytes()
    # an increasing map of everything changes nothing; negating everything negates both fields
    for f, sign in ((4.0, 1.0), (-1.0, -1.0)):
      _push_all(nd, members * np.float32(f))
      _push_all(cl, clim * np.float32(f))
      with pytest.raises(_lib.GencastHipError, match="no index fields on the device"):
        nd.ens_efi_field(0)                                # the store was reserved again: the old fields are not of it
      nd.ens_efi_score(cl, a, truth * np.float32(f))
      # (the NaN of a skipped point keeps its bits; a zero stays +0: the sum of the negated terms starts from +0 as well)
      flip = lambda x: x if sign > 0 else np.where(np.isnan(x), x, np.float32(0.0) - x)
      _same_bytes(nd.ens_efi_field(0), flip(efi), f"EFI of {f} x")
      _same_bytes(nd.ens_efi_field(1), flip(obs), f"observed index of {f} x")
  finally:
    nd.close()
    cl.close()


# ---- 6. state and argument errors ----------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
  gr = _graph()
  G, B, C, M, K = gr.num_grid_nodes, 2, 3, 3, 4
  members, clim, truth, w = _data(M, K, G, B, C, seed=61)
  wq, _ = quantize_node_weights(w)
  a = efi_table(K)
  lib = _lib.load_library()
  dp, i32, u32 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  nd, cl, wide = _handle(gr, B, C), _handle(gr, B, C), _handle(gr, B, C + 1)
  sums = np.empty((B, C, 6))
  sp, ap = sums.ctypes.data_as(dp), a.ctypes.data_as(dp)
  one, wqp = np.array([1], np.int32), wq.ctypes.data_as(u32)

  def raw(h, c, table=ap, s=sp):
    return lib.gc_ens_efi_score(h._h, None if c is None else c._h, table, None, s, None, None, None)

  def err(h=nd):
    return lib.gc_last_error(h._h)

  try:
    # gc_ens_efi_set
    assert lib.gc_ens_efi_set(bare._h, 0, None, None, 20, None) == _lib.GC_ERR_STATE and b"gc_set_graph" in err(bare)
    for T, E, msg in ((5, 20, b"n_events must be in 0..4"), (-1, 20, b"n_events"), (0, 1, b"n_bins must be in 2..32"), (0, 33, b"n_bins")):
      assert lib.gc_ens_efi_set(nd._h, T, one.ctypes.data_as(i32), one.ctypes.data_as(i32), E, wqp) == _lib.GC_ERR_INVALID_ARGUMENT
      assert msg in err()
    assert lib.gc_ens_efi_set(nd._h, 1, one.ctypes.data_as(i32), one.ctypes.data_as(i32), 20, None) == _lib.GC_ERR_INVALID_ARGUMENT
    assert b"null argument" in err()
    zero = np.array([0], np.int32)
    assert lib.gc_ens_efi_set(nd._h, 1, one.ctypes.data_as(i32), zero.ctypes.data_as(i32), 20, wqp) == _lib.GC_ERR_INVALID_ARGUMENT
    assert b"direction 0 is zero" in err()
    with pytest.raises(ValueError, match="node_weight_q"):
      nd.ens_efi_set((1,), (+1,), 20, None)
    # the handles
    assert lib.gc_ens_efi_score(None, cl._h, ap, None, sp, None, None, None) == _lib.GC_ERR_INVALID_ARGUMENT
    assert raw(nd, None) == _lib.GC_ERR_INVALID_ARGUMENT and b"another handle" in err()
    assert raw(nd, nd) == _lib.GC_ERR_INVALID_ARGUMENT and b"another handle" in err()
    assert raw(nd, cl, None) == _lib.GC_ERR_INVALID_ARGUMENT and b"null argument" in err()
    assert raw(bare, cl) == _lib.GC_ERR_STATE and b"gc_set_graph" in err(bare)
    for bad in (wide, bare):
      assert raw(nd, bad) == _lib.GC_ERR_INVALID_ARGUMENT
      assert b"the climatology handle has other dimensions (G, batch, c_out)" in err()
    assert raw(nd, cl) == _lib.GC_ERR_STATE and b"no member store (gc_ens_reserve)" in err()
    with pytest.raises(_lib.GencastHipError, match="ens_reserve"):
      nd.ens_efi_fields(cl, a)
    nd.ens_reserve(M)
    assert raw(nd, cl) == _lib.GC_ERR_STATE and b"no member store on the climatology handle" in err()
    cl.ens_reserve(K)
    for i in range(M - 1):
      nd.ens_push_host(i, members[i])
    assert raw(nd, cl) == _lib.GC_ERR_STATE and b"member slot 2 has not been pushed" in err() and b"climatology" not in err()
    nd.ens_push_host(M - 1, members[M - 1])
    for j in range(1, K):
      cl.ens_push_host(j, clim[j])
    with pytest.raises(_lib.GencastHipError, match="climatology member slot 0 has not been pushed"):
      nd.ens_efi_fields(cl, a)
    cl.ens_push_host(0, clim[0])
    # the table: antisymmetric to the bit and non-decreasing
    off = a.copy()
    off[K] = np.nextafter(off[K], 1.0)                     # one unit in the last place from antisymmetric
    for bad in (off, -a, np.where(np.arange(K + 1) == 1, np.nan, a), np.zeros(K + 1) + 0.1):
      bad = np.ascontiguousarray(bad)
      assert raw(nd, cl, bad.ctypes.data_as(dp)) == _lib.GC_ERR_INVALID_ARGUMENT
      assert b"the table is not antisymmetric and non-decreasing" in err()
    with pytest.raises(ValueError, match="table must have shape"):
      nd.ens_efi_fields(cl, a[:-1])
    # no setting; no weights; no truth
    with pytest.raises(_lib.GencastHipError, match="ens_efi_set has not been called"):
      nd.ens_efi_score(cl, a, truth)
    assert raw(nd, cl) == _lib.GC_ERR_STATE and b"no events and bins (gc_ens_efi_set)" in err()
    nd.ens_efi_set((), (), 20)
    with pytest.raises(_lib.GencastHipError, match="no node weights"):
      nd.ens_efi_score(cl, a, truth)
    nd.ens_set_node_weight(w)
    with pytest.raises(_lib.GencastHipError, match="no truth on the device"):
      nd.ens_efi_score(cl, a, None)
    with pytest.raises(ValueError, match="truth must be"):
      nd.ens_efi_score(cl, a, truth[:-1])
    # downloads
    with pytest.raises(_lib.GencastHipError, match="no index fields on the device"):
      nd.ens_efi_field(0)
    with pytest.raises(ValueError, match="which must be 0"):
      nd.ens_efi_field(2)
    assert nd.counter("ens_efi_calls") == 0
    out = nd.ens_efi_score(cl, a, truth)                   # T = 0: sums and fields alone
    ref = R.reference(members, clim, truth, w, (), (), 20)
    _check("after the errors", nd, out, ref, G)
    assert raw(nd, cl) == _lib.GC_OK                       # weighted, counts and invalid may be NULL at T = 0
    assert sums.tobytes() == out[0].tobytes()
    nd.ens_efi_set((1,), (+1,), 20, wq)
    assert raw(nd, cl) == _lib.GC_ERR_INVALID_ARGUMENT and b"null argument" in err()   # T > 0 needs `weighted`
  finally:
    for h in (nd, cl, wide, bare):
      h.close()
