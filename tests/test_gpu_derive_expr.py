"""The derive ops of gc_ens_derive_set_expr on the device -- sums and norms of term lists across
channels, vorticity and divergence along the grid -- against the definition restated in tests/derive_expr_reference.py,
within the bound that file computes from the inputs; copy channels move bits (==).

Grids: 13 x 24 and 11 x 15 (odd everything) with pole rows, 12 x 16 from 82.5 S to 82.5 N without, where the end rows take
the one-sided difference, and 13 x 24 with descending latitudes.  (B, c_src, M) = (2, 12, 3): one block column of 14 derived
columns, 18 node lanes; (1, 82, 2): 7 columns, 36 lanes.  The destination has c_d = 7 channels mixing all six ops; one sum has
37 terms, one norm two lists.  Handles with set_graph only.

The derived TRUTH has no download of its own: it is checked by running the call again with the fields rotated, so that the
former truth lies in a slot (tests/test_gpu_derive.py does the same)."""
import functools

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, geometry, losses
from tests import derive_expr_reference as X
from tests import derive_reference as R
from tests.helpers import graph_handle as _handle

pytestmark = pytest.mark.gpu

GRIDS = {"poles": (np.linspace(-90, 90, 13), 24), "odd": (np.linspace(-90, 90, 11), 15), "nopole": (np.linspace(-82.5, 82.5, 12), 16),
         "down": (np.linspace(90, -90, 13), 24)}
SIZES = [(2, 12, 3), (1, 82, 2)]                            # B, c_src, M
C_D = 7


@functools.lru_cache(maxsize=None)
def _grid(which):
  lat, n_lon = GRIDS[which]
  lon = np.arange(n_lon) * (360.0 / n_lon)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=2, attention_k_hop=2)
  assert gr.num_grid_nodes == lat.size * n_lon
  return gr, lat, lon


def _plan(which, c_src, seed=0, **pool):
  """c_d = 7: copy, norm2, a sum of 37 terms (every second one a product), a norm of two lists, vorticity, divergence, and a
  sum of one unit term."""
  _, lat, lon = _grid(which)
  rng = np.random.default_rng(seed)
  scale, loc = rng.uniform(0.5, 2.0, c_src), rng.uniform(-1.0, 1.0, c_src)
  long_list = [(float(rng.uniform(-2.0, 2.0)), (5 * t + 2) % c_src, (3 * t + 1) % c_src if t % 2 else -1) for t in range(37)]
  w = [float(v) for v in rng.uniform(0.1, 3.0, 5)]
  qu = [(w[k], 2 + k, (7 + k) % c_src) for k in range(5)]
  qv = [(w[k], 2 + k, (1 + 2 * k) % c_src) for k in range(5)]
  channels = [("copy", c_src - 1), ("norm2", 0, 1, (3.7, -12.5, 0.9, 4.0)), ("sum", long_list), ("norm", qu, qv),
              ("vorticity", 5, 6), ("divergence", 5, 6), ("sum", [(1.0, 7, -1)])]
  return X.raw_plan(c_src, channels, lat.size, lon.size, scale=scale, loc=loc, lat=lat, lon=lon, **pool)


def _fields(which, B, C, M, seed):
  """[M + 1, G, B, C]: M members, then the truth.  Channels span eight decades; scattered NaN and infinities, one NaN latitude
  row and a NaN next to a pole in the wind components of single members, so other pole rows stay finite."""
  _, lat, lon = _grid(which)
  n_lon, G = lon.size, lat.size * lon.size
  members, truth = R.data(M, G, B, C, seed)
  f = np.concatenate([members, truth[None]])
  rng = np.random.default_rng(seed + 100)
  n = 12
  for c, v in ((0, np.nan), (2, np.nan), (3, np.inf), (3, -np.inf), (4, np.nan), (7, np.inf), (C - 1, np.nan)):
    f[rng.integers(0, M + 1, n), rng.integers(0, G, n), rng.integers(0, B, n), c] = v
  f[1, 7, 0, C - 1] = np.uint32(0x7FC12345).view(np.float32)  # a NaN with a payload of its own, through the copy
  f[0, 4 * n_lon:5 * n_lon, 0, 5] = np.nan                    # u: one whole latitude row
  f[1, 1 * n_lon + 5, B - 1, 6] = np.nan                      # v: next to the first end row (a pole, but on "nopole")
  f[1, (lat.size - 2) * n_lon + 2, 0, 5] = np.inf             # u: next to the last end row
  f[M - 1, 6 * n_lon + 3, 0, 6] = -np.inf                     # v: in the interior
  return f


def _push_all(nd, members):
  nd.ens_reserve(len(members))
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _run(dst, src, fields):
  _push_all(src, fields[:-1])
  dst.ens_derive(src, fields[-1])
  return np.stack([dst.ens_download_member(i) for i in range(len(fields) - 1)])


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. every op against the reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,c_src,M", SIZES)
@pytest.mark.parametrize("which", sorted(GRIDS))
def test_every_op_is_within_the_computed_bound_of_the_reference(which, B, c_src, M):
  gr, lat, lon = _grid(which)
  n_lat, n_lon = lat.size, lon.size
  plan = _plan(which, c_src, seed=c_src)
  f = _fields(which, B, c_src, M, seed=c_src + M)
  ref, bound = X.derive(f, plan)
  # what the inputs were made for, on the reference: non-finite results in every computed channel, finite and NaN pole rows
  assert all((~np.isfinite(ref[..., j])).any() for j in range(1, C_D)) and np.isfinite(ref).mean() > 0.8
  g = ref.reshape(M + 1, n_lat, n_lon, B, C_D)
  if which != "nopole":
    assert plan["pole_row"].sum() == 2
    assert np.isnan(g[1, 0, :, B - 1, 4]).all()             # the NaN in v next to the first pole: its whole vorticity row
    assert np.isnan(g[1, n_lat - 1, :, 0, 5]).all()         # the inf in u next to the last: inf - inf in the zonal sum
    assert np.isfinite(g[M, 0, :, :, 4:6]).all() and np.all(g[M, 0, :, :, 4:6] == g[M, 0, :1, :, 4:6])   # one value per pole
  else:
    assert plan["pole_row"].sum() == 0 and np.isfinite(g[M, 0, :, :, 4:6]).all() and np.ptp(g[M, 0, :, 0, 4]) > 0
  src, dst = _handle(gr, B, c_src), _handle(gr, B, C_D)
  try:
    dst.ens_derive_set(**plan)
    dst.ens_reserve(M)
    got = _run(dst, src, f)
    worst = [X.within(got[..., j], ref[:M][..., j], bound[:M][..., j]) for j in range(1, C_D)]
    print(f"{which} ({B}, {c_src}) M={M}: largest error / bound per channel {[f'{w:.2g}' for w in worst]}, "
          f"ens_derive_device_us {dst.counter('ens_derive_device_us')}")
    np.testing.assert_array_equal(_bits(got[..., 0]), _bits(f[:M][..., c_src - 1]))             # the copy channel: the bits
    dst.ens_derive(src)                                          # two calls: the same bytes
    again = np.stack([dst.ens_download_member(i) for i in range(M)])
    assert again.tobytes() == got.tobytes()
    rot = np.roll(f, -1, axis=0)                                 # the former truth lies in the last slot now
    got = _run(dst, src, rot)
    for j in range(1, C_D):
      X.within(got[M - 1][..., j], ref[M][..., j], bound[M][..., j])
    np.testing.assert_array_equal(_bits(got[M - 1][..., 0]), _bits(f[M][..., c_src - 1]))
    assert dst.counter("ens_derive_calls") == 3
  finally:
    src.close()
    dst.close()


# ---- 2. pooling behind the new ops ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", [R.MAX, R.MEAN])
def test_pooling_behind_the_new_ops_equals_the_reference_pooled(pool):
  gr, lat, lon = _grid("poles")
  B, c_src, M = 2, 12, 3
  from gencast_flax_nnx_amd import DerivedSpec
  r_lat, r_lon = 1, DerivedSpec.window(lat, lon, 2500.0)[1]
  rw = np.asarray(losses.normalized_latitude_weights(lat), np.float64)
  plan = _plan("poles", c_src, seed=3, pool=pool, r_lat=r_lat, r_lon=r_lon, row_weight=rw)
  f = _fields("poles", B, c_src, M, seed=9)
  d, _ = X.derive(f[:M], plan)
  ref = np.moveaxis(R.pool_direct(np.moveaxis(d, 1, 0), pool, 13, 24, r_lat, r_lon, rw), 0, 1)
  src, dst = _handle(gr, B, c_src), _handle(gr, B, C_D)
  try:
    dst.ens_derive_set(**plan)
    dst.ens_reserve(M)
    got = _run(dst, src, f)
    np.testing.assert_array_equal(np.isnan(got), ~np.isfinite(d))
    if pool == R.MAX:
      np.testing.assert_array_equal(got, ref)
    else:
      ok = np.isfinite(ref)
      err, bound = np.abs(got.astype(np.float64) - ref), R.mean_bound(d, ref, 24)
      print(f"mean behind the new ops: largest error / bound {float((err[ok] / bound[ok]).max()):.3g}")
      assert np.all(err[ok] <= bound[ok])
  finally:
    src.close()
    dst.close()


# ---- 3. the legacy entry after the new one --------------------------------------------------------------------------------------
def test_the_legacy_entry_after_the_new_one_restores_the_legacy_plan():
  gr, lat, lon = _grid("poles")
  B, c_src, M = 2, 12, 3
  f = _fields("poles", B, c_src, M, seed=21)
  new = _plan("poles", c_src, seed=5)
  old = dict(c_src=c_src, op=np.array([1, 0, 0, 1, 0, 0, 0], np.int32), src_a=np.array([0, 3, 5, 4, 6, 7, 11], np.int32),
             src_b=np.array([1, 0, 0, 2, 0, 0, 0], np.int32),
             affine=np.tile([1.5, -0.25, 0.75, 2.0], (C_D, 1)), pool=0, n_lat=13, n_lon=24)
  ref_new, bound = X.derive(f[:M], new)
  ref_old = R.apply(f[:M], old)
  src, dst = _handle(gr, B, c_src), _handle(gr, B, C_D)
  try:
    dst.ens_reserve(M)
    _push_all(src, f[:M])
    truth, flat = f[M], None
    for r in range(4):
      dst.ens_derive_set(**(old if r % 2 else new))
      dst.ens_derive(src, truth)
      truth = None
      got = np.stack([dst.ens_download_member(i) for i in range(M)])
      if r % 2:
        cp = old["op"] == 0
        np.testing.assert_array_equal(_bits(got[..., cp]), _bits(ref_old[..., cp]))
        X.within(got[..., ~cp], ref_old[..., ~cp], np.spacing(np.abs(ref_old[..., ~cp])))       # norm2: one float32 ulp
      else:
        for j in range(1, C_D):
          X.within(got[..., j], ref_new[..., j], bound[..., j])
      if r == 1:
        flat = dst.counter("device_allocations")                # one plan replaces the other: nothing grows
    assert dst.counter("device_allocations") == flat and dst.counter("ens_derive_calls") == 4
  finally:
    src.close()
    dst.close()


# ---- 4. every validation error of the new entry -----------------------------------------------------------------------------------
def test_every_validation_error_of_the_new_entry():
  gr, lat, lon = _grid("poles")
  B, c_src = 2, 12
  good = _plan("poles", c_src, seed=1)
  rw, r_lon = np.asarray(losses.normalized_latitude_weights(lat), np.float64), np.full(13, 2, np.int32)
  dp, I = _lib.ctypes.POINTER(_lib.ctypes.c_double), _lib._i32p
  INV, STATE, UNSUP, OK = _lib.GC_ERR_INVALID_ARGUMENT, _lib.GC_ERR_STATE, _lib.GC_ERR_UNSUPPORTED, _lib.GC_OK
  order = ("op", "src_a", "src_b", "affine", "pool", "n_lat", "n_lon", "r_lat", "r_lon", "row_weight", "scale", "loc", "term_start",
           "n_terms", "term_coef", "term_a", "term_b", "coslat", "inv_rcos", "inv_dphi", "inv_2dlam", "pole_row")

  def c_set(h, **kw):
    a = dict(good, n_terms=len(good["term_coef"]))
    a.update(kw)
    args = []
    for k in order:
      v = a[k]
      if isinstance(v, np.ndarray):
        v = np.ascontiguousarray(v, np.float64 if v.dtype.kind == "f" else np.int32)
        a[k] = v                                               # (kept alive until the call returns)
        args.append(v.ctypes.data_as(dp if v.dtype.kind == "f" else I))
      else:
        args.append(v)
    return h._lib.gc_ens_derive_set_expr(h._h, a["c_src"], *args)

  def with_at(key, index, value):
    v = np.array(good[key], copy=True)
    v[index] = value
    return {key: v}

  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C_D + 4, c_out=C_D, batch=B)
  dst, src = _handle(gr, B, C_D), _handle(gr, B, c_src)
  try:
    assert c_set(bare) == STATE                                 # before gc_set_graph
    assert c_set(dst) == OK
    ts = good["term_start"]
    assert ts[2].tolist() == [0, 37, 37] and ts[3].tolist() == [37, 42, 47] and ts[6].tolist() == [47, 48, 48]
    long65 = dict(term_start=np.array([[0, 0, 0]] * 2 + [[0, 65, 65], [65, 70, 75]] + [[0, 0, 0]] * 2 + [[75, 76, 76]], np.int32),
                  n_terms=76, term_coef=np.ones(76), term_a=np.zeros(76, np.int32), term_b=np.full(76, -1, np.int32))
    long64 = dict(term_start=np.array([[0, 0, 0]] * 2 + [[0, 64, 64], [64, 69, 74]] + [[0, 0, 0]] * 2 + [[74, 75, 75]], np.int32),
                  n_terms=75, term_coef=np.ones(75), term_a=np.zeros(75, np.int32), term_b=np.full(75, -1, np.int32))
    table = lambda n: dict(n_terms=n, term_coef=np.ones(n), term_a=np.zeros(n, np.int32), term_b=np.full(n, -1, np.int32))
    invalid = [dict(op=None), dict(src_a=None), dict(src_b=None), dict(affine=None), dict(scale=None), dict(loc=None),
               dict(term_start=None), dict(term_coef=None), dict(term_a=None), dict(term_b=None), dict(coslat=None),
               dict(inv_rcos=None), dict(inv_dphi=None), dict(pole_row=None), dict(pool=1, r_lat=1, r_lon=None, row_weight=rw),
               dict(pool=1, r_lat=1, r_lon=r_lon, row_weight=None),
               dict(n_lat=12), dict(c_src=0), dict(r_lat=-1), dict(n_terms=-1),
               with_at("scale", 3, np.nan), with_at("loc", 0, np.inf),
               with_at("term_coef", 5, np.nan), with_at("term_coef", 40, -np.inf),
               with_at("term_a", 0, c_src), with_at("term_a", 47, -1), with_at("term_b", 1, c_src), with_at("term_b", 0, -2),
               with_at("src_a", 0, c_src), with_at("src_a", 4, -1), with_at("src_b", 1, c_src), with_at("src_b", 5, c_src),
               with_at("term_start", (2, 0), -1), with_at("term_start", (2, 1), 0),              # an empty first list
               with_at("term_start", (2, 2), 38),                                                # a sum with a second list
               with_at("term_start", (3, 2), 42),                                                # a norm without one
               with_at("term_start", (6, 2), 49), with_at("term_start", (6, 1), 49),             # beyond the table
               dict(inv_2dlam=0.0), dict(inv_2dlam=np.nan), with_at("coslat", 3, np.nan), with_at("inv_dphi", 3, 0.0),
               with_at("inv_dphi", 0, np.inf), with_at("inv_rcos", 6, np.inf),
               with_at("pole_row", 5, 1),                                                        # a pole row that is no end row
               with_at("pole_row", 1, 1),                                                        # two pole rows next to each other
               with_at("coslat", 0, 1e-3),                                                       # a pole row with cos(lat) != 0
               dict(c_src=8)]                                                                    # channels 8 .. 11 are in use
    for kw in invalid:
      assert c_set(dst, **kw) == INV, kw
    unsupported = [with_at("op", 0, 6), with_at("op", 3, -1), dict(pool=4), dict(pool=-1), long65, table(1025)]
    for kw in unsupported:
      assert c_set(dst, **kw) == UNSUP, kw
    assert c_set(dst, **long64) == OK and c_set(dst, **table(1024)) == OK                        # the caps themselves
    assert c_set(dst, **with_at("src_b", 0, -9)) == OK                                           # src_b of a copy channel is ignored
    assert c_set(dst, **with_at("inv_rcos", 0, np.inf)) == OK                                    # ... and 1 / (R cos) of a pole row
    # without vorticity / divergence no row table is read, without sum / norm no term table
    only_lists = dict(op=np.array([0, 1, 2, 3, 0, 0, 2], np.int32), coslat=None, inv_rcos=None, inv_dphi=None, pole_row=None, inv_2dlam=0.0)
    assert c_set(dst, **only_lists) == OK
    no_lists = dict(op=np.array([0, 1, 0, 1, 4, 5, 0], np.int32), term_start=None, n_terms=0, term_coef=None, term_a=None, term_b=None)
    assert c_set(dst, **no_lists) == OK
    # n_lon >= 3: a grid of two longitudes has the node count of none of these graphs, so the check is reached through
    # n_lat n_lon = G with n_lon = 2
    assert c_set(dst, n_lat=156, n_lon=2, coslat=np.ones(156), inv_rcos=np.ones(156), inv_dphi=np.ones(156),
                 pole_row=np.zeros(156, np.int32)) == INV
    # ---- the wrapper
    for bad in (dict(scale=None), dict(loc=None), dict(scale=np.ones(11)), dict(loc=np.full(c_src, np.nan)), with_at("op", 0, 6),
                dict(term_start=None), dict(term_start=ts[:, :2]), with_at("term_start", (2, 1), 0), with_at("term_start", (3, 2), 42),
                with_at("term_coef", 5, np.nan), dict(term_a=good["term_a"][:-1]), with_at("term_a", 0, c_src), with_at("term_b", 0, -2),
                with_at("src_a", 4, c_src), with_at("src_b", 5, -1), dict(coslat=None), dict(inv_2dlam=None), dict(pole_row=np.zeros(12, np.int32)),
                dict(inv_dphi=good["inv_dphi"][:-1])):
      with pytest.raises(ValueError):
        dst.ens_derive_set(**{**good, **bad})
    legacy = {k: good[k] for k in ("c_src", "src_a", "src_b", "affine", "pool", "n_lat", "n_lon")}
    with pytest.raises(ValueError, match="need scale and loc"):
      dst.ens_derive_set(op=np.zeros(C_D, np.int32), term_start=ts, **legacy)
    with pytest.raises(ValueError, match="0 \\(copy\\) or 1 \\(norm2\\)"):                      # the legacy entry knows two ops
      dst.ens_derive_set(op=good["op"], **legacy)
    assert dst._lib.gc_ens_derive_set(dst._h, c_src, good["op"].ctypes.data_as(I), good["src_a"].ctypes.data_as(I),
                                      good["src_b"].ctypes.data_as(I), good["affine"].ctypes.data_as(dp), 0, 13, 24, 0, None, None) == UNSUP
    # a failed call leaves the plan in force as it was: the store still derives
    dst.ens_derive_set(**good)
    assert c_set(dst, pool=4) == UNSUP
    f = _fields("poles", B, c_src, 2, seed=4)
    dst.ens_reserve(2)
    got = _run(dst, src, f)
    ref, bound = X.derive(f[:2], good)
    for j in range(1, C_D):
      X.within(got[..., j], ref[..., j], bound[..., j])
  finally:
    for h in (bare, dst, src):
      h.close()
