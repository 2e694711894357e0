"""Derived and pooled ensemble fields on the device (gc_ens_derive_*) against the definition restated
in tests/derive_reference.py.  COPY, MAX and MIN are exact: ==.  NORM2 is one rounding of a double result that may differ
from NumPy's by a few 2^-53: one float32 ulp.  MEAN carries the bound of a double prefix sum, computed from the inputs.

Sizes: the 13 x 24 grid (G = 312) and the 11 x 15 grid (G = 165, odd everything), handles with set_graph only.
(B, C) = (2, 6): one partial row tile of 16 columns, with M + 1 = 10 fields, so the intermediate is used in two chunks;
(1, 82) and (4, 82): three and eleven row tiles of 32 columns, the last one partial; (1, 7) on the odd grid: a tile of 8.
r_lat in {0, 1, 3, 12} (12 covers the whole column), r_lon all 0, all 2, a 2500 km window (whole rows at the poles), and
all (n_lon - 1) // 2 -- the whole row everywhere; at 24 longitudes that is a window of 23, at 15 of 15 = n_lon.

The derived TRUTH has no download of its own: it is checked once per shape by running the call again with the fields
rotated, so that the former truth lies in a slot, and through the scorers of the destination (truth = None)."""
import functools

import numpy as np
import pytest

from gencast_flax_nnx_amd import DerivedSpec, _lib, losses
from gencast_flax_nnx_amd.verification import quantize_node_weights
from tests import derive_reference as R
from tests import event_reference as ER
from tests import helpers
from tests.helpers import graph_handle as _handle

pytestmark = pytest.mark.gpu

GRIDS = {"even": (13, 24), "odd": (11, 15)}
SHAPES = [("even", 2, 6, 9), ("even", 1, 82, 2), ("even", 4, 82, 2), ("odd", 1, 7, 2)]      # grid, B, C, M
R_LATS = (0, 1, 3, 12)


@functools.lru_cache(maxsize=None)
def _grid(which):
  from gencast_flax_nnx_amd import geometry
  n_lat, n_lon = GRIDS[which]
  lat, lon = np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=2, attention_k_hop=2)
  assert gr.num_grid_nodes == n_lat * n_lon
  return gr, lat, lon, np.asarray(losses.normalized_latitude_weights(lat), np.float64)


def _push_all(nd, members):
  nd.ens_reserve(len(members))
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _r_lon_cases(which):
  _, lat, lon, _ = _grid(which)
  n_lat, n_lon = GRIDS[which]
  cap = (n_lon - 1) // 2
  by_radius = DerivedSpec.window(lat, lon, 2500.0)[1]
  assert by_radius[0] == by_radius[-1] == cap and by_radius.min() < cap          # the pole rows are capped, the others not
  return [np.zeros(n_lat, np.int32), np.full(n_lat, 2, np.int32), by_radius, np.full(n_lat, cap, np.int32)]


def _copy_plan(which, c, pool=0, r_lat=0, r_lon=None):
  n_lat, n_lon = GRIDS[which]
  return dict(c_src=c, op=np.zeros(c, np.int32), src_a=np.arange(c, dtype=np.int32), src_b=np.zeros(c, np.int32),
              affine=np.tile([1.0, 0.0, 1.0, 0.0], (c, 1)), pool=pool, n_lat=n_lat, n_lon=n_lon, r_lat=r_lat,
              r_lon=r_lon, row_weight=_grid(which)[3] if pool else None)


def _fields(which, B, C, M, seed):
  """[M + 1, G, B, C]: M members, then the truth, with every kind of non-finite input the pooling must skip."""
  n_lat, n_lon = GRIDS[which]
  G = n_lat * n_lon
  members, truth = R.data(M, G, B, C, seed)
  f = np.concatenate([members, truth[None]])
  rng = np.random.default_rng(seed + 100)
  n = 40
  f[rng.integers(0, M + 1, n), rng.integers(0, G, n), rng.integers(0, B, n), 0] = np.nan             # scattered NaN
  f[rng.integers(0, M + 1, n), rng.integers(0, G, n), rng.integers(0, B, n), 1] = np.inf             # +inf and -inf are
  f[rng.integers(0, M + 1, n), rng.integers(0, G, n), rng.integers(0, B, n), 1] = -np.inf            # skipped, never winners
  f[:, 4 * n_lon:5 * n_lon, 0, 2] = np.nan                  # one whole latitude row
  f[:, :, B - 1, 3] = np.nan                                # one whole (b, c) column
  f[:, :, 0, 4] = np.nan                                    # a finite centre, every neighbour NaN
  f[:, 6 * n_lon + 5, 0, 4] = np.float32(2.5)
  f[:, :, B - 1, 5] = np.float32(7.25)                      # a constant field
  f[0, 2 * n_lon + 3, 0, C - 1] = np.nan                    # a NaN centre with finite neighbours
  return f


def _run(dst, src, fields):
  """One derive of (members = fields[:-1], truth = fields[-1]) -> the destination's members [M, G, B, c_d]."""
  _push_all(src, fields[:-1])
  dst.ens_derive(src, fields[-1])
  return np.stack([dst.ens_download_member(i) for i in range(len(fields) - 1)])


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. copy, no pool -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,c_src,src_a", [(2, 6, [4, 0, 2, 0, 5]), (4, 82, list(range(82)))])
def test_copy_without_pooling_moves_the_bits(B, c_src, src_a):
  gr = _grid("even")[0]
  G, M, c_d = gr.num_grid_nodes, 3, len(src_a)
  members, truth = R.data(M, G, B, c_src, seed=c_src)
  f = np.concatenate([members, truth[None]])
  f[1, 7, 0, 0] = np.uint32(0x7FC12345).view(np.float32)      # a NaN with a payload of its own
  f[2, 100, B - 1, 4] = np.nan
  f[0, 5, 0, 2] = np.inf
  f[M, 9, 0, 0] = -np.inf
  f[M, 200, B - 1, 5] = np.nan
  plan = dict(c_src=c_src, op=np.zeros(c_d, np.int32), src_a=np.asarray(src_a, np.int32), src_b=np.full(c_d, -7, np.int32),
              affine=np.full((c_d, 4), np.nan), pool=0, n_lat=13, n_lon=24)                 # src_b and affine are ignored
  src, dst = _handle(gr, B, c_src), _handle(gr, B, c_d)
  try:
    dst.ens_derive_set(**plan)
    dst.ens_reserve(M)
    got = _run(dst, src, f)
    np.testing.assert_array_equal(_bits(got), _bits(f[:M][..., src_a]))
    assert np.isnan(got).sum() == np.isnan(f[:M][..., src_a]).sum() > 0 and np.isinf(got).any()
    rot = np.roll(f, -1, axis=0)                              # the former truth lies in the last slot now
    got = _run(dst, src, rot)
    np.testing.assert_array_equal(_bits(got), _bits(rot[:M][..., src_a]))
    assert dst.counter("ens_derive_calls") == 2
    print(f"copy ({B}, {c_src}) -> {c_d}: ens_derive_device_us {dst.counter('ens_derive_device_us')}")
  finally:
    src.close()
    dst.close()


# ---- 2. norm2, no pool ------------------------------------------------------------------------------------------------------
def test_norm2_without_pooling_is_within_one_float32_ulp():
  gr = _grid("even")[0]
  G, B, c_src, M = gr.num_grid_nodes, 2, 6, 3
  members, truth = R.data(M, G, B, c_src, seed=11)
  f = np.concatenate([members, truth[None]])
  f[0, 3, 0, 0] = np.nan
  f[1, 4, 1, 1] = np.inf
  f[2, 5, 0, 5] = -np.inf
  f[M, 6, 1, 2] = np.nan
  plan = dict(c_src=c_src, op=np.array([1, 1, 0, 1], np.int32), src_a=np.array([0, 5, 3, 4], np.int32),
              src_b=np.array([1, 2, 0, 4], np.int32),
              affine=np.array([[3.7, -12.5, 0.9, 4.0], [1e-3, 250.0, 41.0, -3e4], [1, 0, 1, 0], [2.5, 0.0, -2.5, 1e-7]]),
              pool=0, n_lat=13, n_lon=24)
  src, dst = _handle(gr, B, c_src), _handle(gr, B, 4)
  try:
    dst.ens_derive_set(**plan)
    dst.ens_reserve(M)
    for fields in (f, np.roll(f, -1, axis=0)):
      got = _run(dst, src, fields)
      ref = R.apply(fields[:M], plan)
      assert ref.dtype == np.float32
      np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
      np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref))
      ok = np.isfinite(ref)
      assert (~ok).sum() >= 3 and not np.isneginf(got).any()
      err = np.abs(got[ok].astype(np.float64) - ref[ok].astype(np.float64))
      ulp = np.spacing(np.abs(ref[ok]))                        # (the copy channel between the norms is signed, and exact)
      print(f"norm2: max error {float((err / ulp).max()):.3g} ulp, {int((err > 0).sum())} of {err.size} differ")
      assert np.all(err <= ulp)
      np.testing.assert_array_equal(_bits(got[..., 2]), _bits(fields[:M][..., 3]))      # the copy channel between them
  finally:
    src.close()
    dst.close()


# ---- 3. MAX and MIN: == ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [R.MAX, R.MIN])
@pytest.mark.parametrize("which,B,C,M", SHAPES)
def test_max_and_min_equal_the_definition(which, B, C, M, pool):
  gr = _grid(which)[0]
  n_lat, n_lon = GRIDS[which]
  f = _fields(which, B, C, M, seed=C + M)
  src, dst = _handle(gr, B, C), _handle(gr, B, C)
  try:
    dst.ens_reserve(M)
    _push_all(src, f[:M])
    truth = f[M]
    for r_lat in R_LATS:
      for r_lon in _r_lon_cases(which):
        plan = _copy_plan(which, C, pool, r_lat, r_lon)
        dst.ens_derive_set(**plan)
        dst.ens_derive(src, truth)
        truth = None                                          # uploaded once: it stays in the source
        got = np.stack([dst.ens_download_member(i) for i in range(M)])
        ref = R.apply(f[:M], plan)
        np.testing.assert_array_equal(got, ref, err_msg=f"pool {pool} r_lat {r_lat} r_lon {r_lon.tolist()}")
        np.testing.assert_array_equal(np.isnan(got), ~np.isfinite(f[:M]))
        assert np.all(got[:, 6 * n_lon + 5, 0, 4] == np.float32(2.5))           # every neighbour NaN: the centre itself
        assert np.all(got[:, :, B - 1, 5] == np.float32(7.25))
    # the truth, through a slot: the fields rotated by one, the widest of the capped windows
    plan = _copy_plan(which, C, pool, 3, _r_lon_cases(which)[2])
    dst.ens_derive_set(**plan)
    rot = np.roll(f, -1, axis=0)
    np.testing.assert_array_equal(_run(dst, src, rot)[M - 1], R.apply(f[M], plan))
    print(f"{which} ({B}, {C}) M={M} pool {pool}: ens_derive_device_us {dst.counter('ens_derive_device_us')}")
  finally:
    src.close()
    dst.close()


def test_norm2_followed_by_pooling_pools_the_device_own_norm():
  gr = _grid("even")[0]
  B, c_src, M = 2, 6, 3
  f = _fields("even", B, c_src, M, seed=5)
  base = dict(c_src=c_src, op=np.array([1, 0, 1], np.int32), src_a=np.array([0, 2, 4], np.int32), src_b=np.array([1, 0, 5], np.int32),
              affine=np.array([[3.7, -12.5, 0.9, 4.0], [1, 0, 1, 0], [1e2, 1.0, 1e-2, -1.0]]), n_lat=13, n_lon=24)
  src, dst = _handle(gr, B, c_src), _handle(gr, B, 3)
  try:
    dst.ens_reserve(M)
    dst.ens_derive_set(pool=0, **base)
    d = _run(dst, src, f)                                     # the device's own pool = NONE output of the plan
    for pool in (R.MAX, R.MIN):
      for r_lat, r_lon in ((1, _r_lon_cases("even")[1]), (3, _r_lon_cases("even")[2])):
        dst.ens_derive_set(pool=pool, r_lat=r_lat, r_lon=r_lon, row_weight=_grid("even")[3], **base)
        dst.ens_derive(src)
        got = np.stack([dst.ens_download_member(i) for i in range(M)])
        ref = np.moveaxis(R.pool_direct(np.moveaxis(d, 1, 0), pool, 13, 24, r_lat, r_lon, _grid("even")[3]), 0, 1)
        np.testing.assert_array_equal(got, ref)
  finally:
    src.close()
    dst.close()


# ---- 4. MEAN ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,B,C,M", SHAPES)
def test_mean_is_within_the_bound_of_a_double_prefix_sum(which, B, C, M):
  gr = _grid(which)[0]
  n_lat, n_lon = GRIDS[which]
  f = _fields(which, B, C, M, seed=2 * C + M)
  src, dst = _handle(gr, B, C), _handle(gr, B, C)
  worst = 0.0
  try:
    dst.ens_reserve(M)
    _push_all(src, f[:M])
    truth = f[M]
    for r_lat in R_LATS:
      for r_lon in _r_lon_cases(which):
        plan = _copy_plan(which, C, R.MEAN, r_lat, r_lon)
        dst.ens_derive_set(**plan)
        dst.ens_derive(src, truth)
        truth = None
        got = np.stack([dst.ens_download_member(i) for i in range(M)])
        # (the separable restatement where the direct one takes seconds: tests/test_derive.py holds them to 1e-15 of each other)
        ref = R.apply(f[:M], plan, separable=B * C * M > 300)
        bound = R.mean_bound(f[:M], ref, n_lon)               # from the reference's own inputs
        np.testing.assert_array_equal(np.isnan(got), ~np.isfinite(f[:M]))
        ok = np.isfinite(ref)
        err = np.abs(got.astype(np.float64) - ref)
        assert np.all(err[ok] <= bound[ok]), (r_lat, r_lon.tolist(), float((err[ok] / bound[ok]).max()))
        worst = max(worst, float((err[ok] / bound[ok]).max()))
        assert np.all(np.abs(got[:, :, B - 1, 5].astype(np.float64) - 7.25) <= bound[:, :, B - 1, 5])   # the constant field
        assert np.all(got[:, 6 * n_lon + 5, 0, 4] == np.float32(2.5))
    plan = _copy_plan(which, C, R.MEAN, 3, _r_lon_cases(which)[2])
    dst.ens_derive_set(**plan)
    rot = np.roll(f, -1, axis=0)
    got, ref = _run(dst, src, rot)[M - 1], R.apply(f[M], plan)
    ok = np.isfinite(ref)
    assert np.all(np.abs(got.astype(np.float64) - ref)[ok] <= R.mean_bound(f[M], ref, n_lon)[ok])
    print(f"{which} ({B}, {C}) M={M} mean: worst error / bound {worst:.3g}, ens_derive_device_us {dst.counter('ens_derive_device_us')}")
  finally:
    src.close()
    dst.close()


# ---- 5. into the scorers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,M", [(2, 6, 8), (1, 82, 3)])
def test_the_scorers_of_the_destination_see_the_derived_store(B, C, M):
  gr = _grid("even")[0]
  G, T = gr.num_grid_nodes, 3
  members, truth, w, thr, d = ER.data(M, G, B, C, seed=M, T=T)
  members[1, 17, 0, 2] = np.nan
  truth[40, B - 1, 1] = np.nan
  wq, _ = quantize_node_weights(w)
  plan = _copy_plan("even", C, R.MAX, 1, _r_lon_cases("even")[2])
  src, dst, third = (_handle(gr, B, C) for _ in range(3))
  try:
    _push_all(src, members)
    dst.ens_reserve(M)
    dst.ens_derive_set(**plan)
    dst.ens_derive(src, truth)
    _push_all(third, R.apply(members, plan))
    for h in (dst, third):
      h.ens_set_node_weight(w)
      h.ens_event_set(thr, d, wq)
    a = dst.ens_score(None, want_fields=True) + dst.ens_event_score(None) + dst.ens_download_fields()
    b = third.ens_score(R.apply(truth, plan), want_fields=True) + third.ens_event_score(None) + third.ens_download_fields()
    for x, y in zip(a, b):
      assert x.tobytes() == y.tobytes()
    for t in range(T):
      assert dst.ens_event_codes(t).tobytes() == third.ens_event_codes(t).tobytes()
    assert a[2].sum() > 0 and dst.counter("ens_invalid_points") == third.counter("ens_invalid_points") > 0
  finally:
    for h in (src, dst, third):
      h.close()


# ---- 6. state -------------------------------------------------------------------------------------------------------------------
def test_state_determinism_and_ownership():
  gr = _grid("even")[0]
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  members, truth, w, thr, d = ER.data(M, G, B, C, seed=61, T=2)
  wq, _ = quantize_node_weights(w)
  src, dst = _handle(gr, B, C), _handle(gr, B, C)
  cases = _r_lon_cases("even")
  try:
    _push_all(src, members)
    src.ens_set_node_weight(w)
    before = src.ens_score(truth)
    dst.ens_reserve(M)
    dst.ens_set_node_weight(w)
    dst.ens_event_set(thr, d, wq)
    dst.ens_derive_set(**_copy_plan("even", C, R.MEAN, 3, cases[2]))
    dst.ens_derive(src)                                        # the truth of the source's ens_score
    first = [dst.ens_download_member(i) for i in range(M)] + list(dst.ens_score(None))
    dst.ens_event_score(None)
    dst.ens_event_codes(0)
    dst.ens_derive(src)
    with pytest.raises(_lib.GencastHipError, match="no event codes"):      # the codes were of the store before
      dst.ens_event_codes(0)
    with pytest.raises(_lib.GencastHipError, match="no mean / variance"):
      dst.ens_download_fields()
    second = [dst.ens_download_member(i) for i in range(M)] + list(dst.ens_score(None))
    for x, y in zip(first, second):
      assert x.tobytes() == y.tobytes()
    dst.ens_event_score(None)
    dst.ens_event_codes(0)
    # the source: members and scores as they were
    for i in range(M):
      np.testing.assert_array_equal(src.ens_download_member(i), members[i])
    for x, y in zip(before, src.ens_score(None)):
      assert x.tobytes() == y.tobytes()
    # the plan survives gc_ens_reserve; a slot of the new store counts as pushed after the call
    dst.ens_reserve(M)
    dst.ens_derive(src)
    assert dst.ens_download_member(M - 1).tobytes() == first[M - 1].tobytes()
    # twenty rounds of set / derive, alternating pool and r_lat: replaced, not grown
    calls = dst.counter("ens_derive_calls")
    assert calls == 3

    def round_(r):
      pool = (R.MAX, R.MEAN, R.NONE)[r % 3]
      dst.ens_derive_set(**_copy_plan("even", C, pool, (0, 3, 12)[r % 3] if pool else 0, cases[r % 4] if pool else None))
      dst.ens_derive(src)

    for r in range(3):
      round_(r)
    flat = dst.counter("device_allocations"), src.counter("device_allocations")
    for r in range(20):
      round_(r)
      assert (dst.counter("device_allocations"), src.counter("device_allocations")) == flat
    assert dst.counter("ens_derive_calls") == calls + 23 and dst.counter("ens_derive_device_us") >= 0
    last = _copy_plan("even", C, R.MEAN, 3, cases[3])          # round 19: what the store holds is that plan's result
    got, ref = dst.ens_download_member(0), R.apply(members[0], last)
    assert np.all(np.abs(got.astype(np.float64) - ref) <= R.mean_bound(members[0], ref, 24))
  finally:
    src.close()
    dst.close()


# ---- 7. every documented error ------------------------------------------------------------------------------------------------
def test_every_documented_error():
  gr = _grid("even")[0]
  G, B, C, CD, M = gr.num_grid_nodes, 2, 6, 3, 2
  members, truth = R.data(M, G, B, C, seed=71)
  rw, r_lon = _grid("even")[3], np.full(13, 2, np.int32)
  op, a, b = np.array([1, 0, 0], np.int32), np.array([0, 2, 5], np.int32), np.array([1, 0, 0], np.int32)
  aff = np.tile([1.0, 0.0, 1.0, 0.0], (CD, 1))
  dp = _lib.ctypes.POINTER(_lib.ctypes.c_double)
  p = lambda x, ty: None if x is None else x.ctypes.data_as(ty)
  I, INV, STATE, UNSUP = _lib._i32p, _lib.GC_ERR_INVALID_ARGUMENT, _lib.GC_ERR_STATE, _lib.GC_ERR_UNSUPPORTED

  def c_set(h, c_src=C, op=op, a=a, b=b, aff=aff, pool=1, n_lat=13, n_lon=24, r_lat=1, r_lon=r_lon, rw=rw):
    return h._lib.gc_ens_derive_set(h._h, c_src, p(op, I), p(a, I), p(b, I), p(aff, dp), pool, n_lat, n_lon, r_lat, p(r_lon, I), p(rw, dp))

  good = dict(c_src=C, op=op, src_a=a, src_b=b, affine=aff, pool=1, n_lat=13, n_lon=24, r_lat=1, r_lon=r_lon, row_weight=rw)
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=CD + 4, c_out=CD, batch=B)
  src, dst, other_b, other_c = _handle(gr, B, C), _handle(gr, B, CD), _handle(gr, B + 1, C), _handle(gr, B, C + 1)
  small = _handle(_grid("odd")[0], B, C)
  lib = dst._lib
  try:
    # ---- gc_ens_derive_set
    assert c_set(bare) == STATE                               # before gc_set_graph
    assert lib.gc_ens_derive(bare._h, src._h, None) == STATE
    for kw in (dict(op=None), dict(a=None), dict(b=None), dict(aff=None), dict(r_lon=None), dict(rw=None)):
      assert c_set(dst, **kw) == INV, kw
    assert c_set(dst, pool=0, r_lon=None, rw=None) == _lib.GC_OK      # r_lon and row_weight may be NULL without a pool
    for kw in (dict(n_lat=12), dict(n_lat=24, n_lon=13 + 1), dict(n_lat=0, n_lon=0), dict(c_src=0),
               dict(a=np.array([0, 6, 5], np.int32)), dict(a=np.array([-1, 2, 5], np.int32)), dict(b=np.array([6, 0, 0], np.int32)),
               dict(c_src=5), dict(r_lat=-1), dict(r_lon=np.array([2] * 12 + [12], np.int32)), dict(r_lon=np.array([-1] + [2] * 12, np.int32)),
               dict(rw=np.where(np.arange(13) == 4, 0.0, rw)), dict(rw=np.where(np.arange(13) == 4, -1.0, rw)),
               dict(rw=np.where(np.arange(13) == 4, np.nan, rw)), dict(rw=np.where(np.arange(13) == 4, np.inf, rw))):
      assert c_set(dst, **kw) == INV, kw
    assert c_set(dst, b=np.array([1, -9, 99], np.int32)) == _lib.GC_OK     # src_b of a copy channel is ignored
    for kw in (dict(op=np.array([2, 0, 0], np.int32)), dict(op=np.array([0, -1, 0], np.int32)), dict(pool=4), dict(pool=-1)):
      assert c_set(dst, **kw) == UNSUP, kw
    for bad in (dict(op=op[:2]), dict(src_a=a[:2]), dict(src_b=np.zeros(4, np.int32)), dict(affine=aff[:, :3]), dict(op=np.array([2, 0, 0])),
                dict(src_a=np.array([0, 6, 5])), dict(src_b=np.array([6, 0, 0])), dict(c_src=0), dict(pool=4), dict(n_lat=12),
                dict(n_lat=None), dict(r_lat=-1), dict(r_lon=None), dict(row_weight=None), dict(r_lon=r_lon[:-1]), dict(row_weight=rw[:-1]),
                dict(r_lon=np.full(13, 12)), dict(r_lon=np.full(13, -1)), dict(row_weight=np.zeros(13)),
                dict(row_weight=np.where(np.arange(13) == 1, np.nan, rw))):
      with pytest.raises(ValueError):
        dst.ens_derive_set(**{**good, **bad})
    # ---- gc_ens_derive
    fresh = _handle(gr, B, CD)
    try:
      with pytest.raises(_lib.GencastHipError, match="no plan"):
        fresh.ens_derive(src)
      assert lib.gc_ens_derive(fresh._h, src._h, None) == STATE            # no plan
    finally:
      fresh.close()
    dst.ens_derive_set(**good)
    assert lib.gc_ens_derive(dst._h, dst._h, None) == INV and lib.gc_ens_derive(dst._h, None, None) == INV
    for bad in (dst, None, "src"):
      with pytest.raises(ValueError, match="another NativeDenoiser"):
        dst.ens_derive(bad)
    for h in (bare, other_b, other_c, small):                 # no graph; another batch; c_out != c_src; another G
      assert lib.gc_ens_derive(dst._h, h._h, None) == INV
      with pytest.raises(ValueError, match="other dimensions"):
        dst.ens_derive(h)
    with pytest.raises(_lib.GencastHipError, match="no member store"):       # on dst
      dst.ens_derive(src, truth)
    dst.ens_reserve(M)
    with pytest.raises(_lib.GencastHipError, match="no member store on the source"):
      dst.ens_derive(src, truth)
    src.ens_reserve(M + 1)
    with pytest.raises(_lib.GencastHipError, match="different numbers of members"):
      dst.ens_derive(src, truth)
    src.ens_reserve(M)
    src.ens_push_host(0, members[0])
    with pytest.raises(_lib.GencastHipError, match="source member slot 1 has not been pushed"):
      dst.ens_derive(src, truth)
    src.ens_push_host(1, members[1])
    with pytest.raises(_lib.GencastHipError, match="no truth on the source"):
      dst.ens_derive(src)
    assert lib.gc_ens_derive(dst._h, src._h, None) == STATE
    with pytest.raises(ValueError, match="truth must be"):
      dst.ens_derive(src, truth[..., :CD])
    assert dst.counter("ens_derive_calls") == 0
    dst.ens_derive(src, truth)
    dst.ens_derive(src)                                        # the truth stays in the source
    src.ens_set_node_weight(np.ones(G, np.float32))
    src.ens_score(None)                                        # ... as gc_ens_score(src, truth, ...) would have left it
    assert dst.counter("ens_derive_calls") == 2
    with pytest.raises(ValueError):
      dst.counter("ens_derive_no_such_counter")
  finally:
    for h in (bare, src, dst, other_b, other_c, small):
      h.close()


# ---- 8. the sampler is left alone ----------------------------------------------------------------------------------------------
def test_a_derive_call_leaves_the_sampler_state_alone():
  from oracle import gencast_oracle as O
  gr, dims, params, cond, _ = helpers.tiny_setup(batch=2, seed=2)
  rng = np.random.default_rng(8)
  G, C = gr.num_grid_nodes, dims.c_out
  noise = rng.standard_normal((G, 2, C)).astype(np.float32)
  truth = rng.standard_normal((G, 2, C)).astype(np.float32)
  plan = dict(c_src=C, op=np.array([1, 0], np.int32), src_a=np.array([0, 3], np.int32), src_b=np.array([1, 0], np.int32),
              affine=np.array([[3.7, -12.5, 0.9, 4.0], [1, 0, 1, 0]]), pool=R.MAX, n_lat=13, n_lon=24, r_lat=1,
              r_lon=_r_lon_cases("even")[2], row_weight=_grid("even")[3])
  nd = helpers.make_native(gr, dims, params, 2)
  other = helpers.make_native(gr, dims, params, 2)
  view = _handle(gr, 2, 2)
  try:
    for h in (nd, other):
      h.set_option("graphs", "on")
      h.set_noisy_slots(np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32))
      h.upload_cond(cond)
    nd.upload_noise(noise)
    other.upload_noise(-noise)
    sched = O.noise_schedule(80.0, 0.03, 4, 7.0).astype(np.float32)
    nd.sample_resident(sched)
    first = nd.download_sample()
    nd.sample_resident(sched)                                      # captured here
    np.testing.assert_array_equal(nd.download_sample(), first)
    nd.stash_sample()
    other.sample_resident(sched)
    second = other.download_sample()
    replays, captures = nd.counter("graph_replays"), nd.counter("graph_captures")
    nd.ens_reserve(2)
    nd.ens_push(0)
    nd.ens_push(1, src=other)
    view.ens_derive_set(**plan)
    view.ens_reserve(2)
    view.ens_derive(nd, truth)
    got = np.stack([view.ens_download_member(i) for i in range(2)])
    d = R.derive(np.stack([first, second]), plan["op"], plan["src_a"], plan["src_b"], plan["affine"])
    ref = R.apply(np.stack([first, second]), plan)
    np.testing.assert_array_equal(got[..., 1], ref[..., 1])         # the copy channel, pooled: exact
    # the norm channel: pooling commutes with a one-ulp error of its input up to that ulp
    assert np.all(np.abs(got[..., 0].astype(np.float64) - ref[..., 0]) <= np.spacing(ref[..., 0])) and np.isfinite(d).all()
    np.testing.assert_array_equal(nd.download_sample(), first)      # the last sample is still there
    np.testing.assert_array_equal(nd.download_stash(), first)
    np.testing.assert_array_equal(other.download_sample(), second)
    np.testing.assert_array_equal(nd.download_cond(), cond)
    np.testing.assert_array_equal(nd.download_noise(), noise)
    np.testing.assert_array_equal(nd.ens_download_member(0), first)
    np.testing.assert_array_equal(nd.ens_download_member(1), second)
    nd.sample_resident(sched)                                      # a replay of the captured graph: the same bytes
    np.testing.assert_array_equal(nd.download_sample(), first)
    assert nd.counter("graph_captures") == captures and nd.counter("graph_replays") == replays + 1
  finally:
    nd.close()
    other.close()
    view.close()
