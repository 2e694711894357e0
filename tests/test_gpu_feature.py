"""Ensemble feature detection on the device (gc_ens_feature_*) against the definition restated in
tests/feature_reference.py.  The definition holds comparisons and one double subtraction: every comparison here is exact --
integer equality of counts and nodes, the bits of the listed values, == on the 0 / 1 / NaN strike fields.

Sizes: the 13 x 24 grid (G = 312: two blocks of the column pass, the second partial) and the 11 x 15 grid (G = 165, odd
everything), handles with set_graph only.  (B, C, M) = (2, 6, 9): M + 1 = 10 fields, two chunks of the work buffers; (1, 82, 2):
a wide source row; (1, 7, 2) on the odd grid.  Extremum windows: r_lat in {0, 1, 3}, r_lon all 0, all 2, the 2500 km window
(whole rows at the poles) and all (n_lon - 1) // 2.

The strike field of the TRUTH has no download of its own: it is checked by running the call again with the fields rotated,
so that the former truth lies in a slot, and through `ens_score(None)` of the destination."""
import functools

import numpy as np
import pytest

from gencast_flax_nnx_amd import DerivedSpec, _lib
from tests import feature_reference as R
from tests.helpers import graph_handle as _handle

pytestmark = pytest.mark.gpu

GRIDS = {"even": (13, 24), "odd": (11, 15)}
SHAPES = [("even", 2, 6, 9), ("even", 1, 82, 2), ("odd", 1, 7, 2)]      # grid, B, C, M
R_LATS = (0, 1, 3)


@functools.lru_cache(maxsize=None)
def _grid(which):
  from gencast_flax_nnx_amd import geometry
  n_lat, n_lon = GRIDS[which]
  lat, lon = np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=2, attention_k_hop=2)
  assert gr.num_grid_nodes == n_lat * n_lon
  return gr, lat, lon


def _r_lon_cases(which):
  _, lat, lon = _grid(which)
  n_lat, n_lon = GRIDS[which]
  cap = (n_lon - 1) // 2
  by_radius = DerivedSpec.window(lat, lon, 2500.0)[1]
  assert by_radius[0] == by_radius[-1] == cap and by_radius.min() < cap          # the pole rows are capped, the others not
  return [np.zeros(n_lat, np.int32), np.full(n_lat, 2, np.int32), by_radius, np.full(n_lat, cap, np.int32)]


def _smooth(rng, n_lat, n_lon, cols):
  """Smooth noise [G, cols] rounded to multiples of 0.25: ties are frequent."""
  x = rng.standard_normal((n_lat, n_lon) + cols)
  for _ in range(2):
    x = (x + np.roll(x, 1, 0) + np.roll(x, -1, 0) + np.roll(x, 1, 1) + np.roll(x, -1, 1)) / 5.0
  return (np.round(x * 24.0) / 4.0).astype(np.float32).reshape((n_lat * n_lon,) + cols)


@functools.lru_cache(maxsize=None)
def _fields(which, B, C, M):
  """[M + 1, G, B, C]: M members, then the truth.  Channels: 0 smooth with scattered NaN and planted lows (a pole row, j = 0,
  j = n_lon - 1); 1 smooth with +-inf and a whole NaN row; 2 NaN but for one node; 3 constant; 4 ones with a -0.0 next to a
  +0.0; 5 smooth with a NaN where its lowest value was; the others smooth."""
  n_lat, n_lon = GRIDS[which]
  G = n_lat * n_lon
  rng = np.random.default_rng(1000 * C + M)
  f = np.moveaxis(_smooth(rng, n_lat, n_lon, (M + 1, B, C)), 0, 1).copy()
  n = 30
  f[rng.integers(0, M + 1, n), rng.integers(0, G, n), rng.integers(0, B, n), 0] = np.nan
  f[:, 0 * n_lon + 5, :, 0] = np.float32(-50.0)             # a centre in a pole row
  f[:, 6 * n_lon + 0, :, 0] = np.float32(-40.0)             # a centre at j = 0
  f[:, (n_lat - 3) * n_lon + n_lon - 1, :, 0] = np.float32(-45.0)     # a centre at j = n_lon - 1
  f[rng.integers(0, M + 1, n), rng.integers(0, G, n), rng.integers(0, B, n), 1] = np.inf
  f[rng.integers(0, M + 1, n), rng.integers(0, G, n), rng.integers(0, B, n), 1] = -np.inf
  f[:, 4 * n_lon:5 * n_lon, 0, 1] = np.nan                  # one whole latitude row
  f[..., 2] = np.nan                                        # a finite centre, every neighbour NaN
  f[:, 6 * n_lon + 5, :, 2] = np.float32(2.5)
  f[..., 3] = np.float32(7.25)                              # a constant field
  f[..., 4] = np.float32(1.0)                               # the two zeros side by side, in both orders
  f[0::2, 5 * n_lon + 7, :, 4], f[0::2, 5 * n_lon + 8, :, 4] = np.float32(-0.0), np.float32(0.0)
  f[1::2, 5 * n_lon + 7, :, 4], f[1::2, 5 * n_lon + 8, :, 4] = np.float32(0.0), np.float32(-0.0)
  f[:, 9 * n_lon + 0, :, 4], f[:, 9 * n_lon + n_lon - 1, :, 4] = np.float32(0.0), np.float32(-0.0)   # ... and across the wrap
  for z in range(M + 1):                                    # a NaN at what would be a centre
    for b in range(B):
      f[z, np.argmin(f[z, :, b, 5]), b, 5] = np.nan
  f.setflags(write=False)
  return f


def _push_all(nd, members):
  nd.ens_reserve(len(members))
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _bits(a):
  return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _detector(which, channel, r_lat, r_lon, *, direction=-1, threshold=None, ring=True, depth=0.5, strike=(1, 2)):
  n_lat, n_lon = GRIDS[which]
  cap = (n_lon - 1) // 2
  det = dict(channel=channel, direction=direction, threshold=threshold, r_lat=r_lat, r_lon=r_lon, strike_lat=strike[0],
             strike_lon=np.minimum(cap, np.full(n_lat, strike[1])) if np.ndim(strike[1]) == 0 else strike[1])
  if ring:
    det.update(ring_lat=r_lat + 1, ring_lon=np.minimum(cap, np.asarray(r_lon) + 1), depth=depth)
  return det


def _check(dst, src, fields, plan, M, msg=""):
  """One call on (members = fields[:-1], truth = fields[-1]) against the reference: the lists of all M + 1 fields and the
  strike fields of the M members.  -> (reference count, reference strike [M + 1, G, B, D])."""
  dst.ens_feature(src, fields[-1])
  count, node, value = dst.ens_feature_centres()
  got = np.stack([dst.ens_download_member(i) for i in range(M)])
  r_count, r_node, r_value, r_strike = R.apply(fields, plan)
  np.testing.assert_array_equal(count, r_count, err_msg=msg)
  np.testing.assert_array_equal(node, r_node, err_msg=msg)
  np.testing.assert_array_equal(_bits(value), _bits(r_value), err_msg=msg)
  np.testing.assert_array_equal(got, r_strike[:M], err_msg=msg)
  return r_count, r_strike


# ---- 1. one detector ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,B,C,M", SHAPES)
def test_one_detector_equals_the_definition(which, B, C, M):
  gr = _grid(which)[0]
  n_lat, n_lon = GRIDS[which]
  f = np.array(_fields(which, B, C, M))
  src, dst = _handle(gr, B, C), _handle(gr, B, 1)
  seen = np.zeros(6, np.int64)
  try:
    dst.ens_reserve(M)
    _push_all(src, f[:M])
    case = 0
    for r_lat in R_LATS:
      for r_lon in _r_lon_cases(which):
        ch = case % 6                                       # every special channel under two windows
        # the threshold admits most of a channel's range; channel 2 (one finite node) has no finite ring: no ring test there
        det = _detector(which, ch, r_lat, r_lon, direction=1 if case % 4 == 3 else -1, threshold=None if ch in (2, 3) else 0.25,
                        ring=ch in (0, 1, 5), strike=(case % 3, 1 + case % 3))
        plan = R.plan_of(C, n_lat, n_lon, [det])
        dst.ens_feature_set(**plan)
        r_count, r_strike = _check(dst, src, f, plan, M, msg=f"channel {ch} r_lat {r_lat} r_lon {r_lon.tolist()}")
        seen[ch] += r_count.sum()
        assert np.array_equal(np.isnan(r_strike[..., 0]), ~np.isfinite(f[..., ch]))
        case += 1
    assert np.all(seen[[0, 2, 3, 4]] > 0), seen              # the planted centres were there to be found
    print(f"{which} ({B}, {C}) M={M}: centres per channel {seen.tolist()}, ens_feature_device_us {dst.counter('ens_feature_device_us')}")
  finally:
    src.close()
    dst.close()


def test_the_planted_centres_are_centres():
  """What the fields are built for, stated on the reference and found by the device: a centre in a pole row, at j = 0 and at
  j = n_lon - 1, the finite node among NaNs, one centre per window of a constant field, the lower node of two equal zeros."""
  which, B, C, M = "even", 2, 6, 9
  gr = _grid(which)[0]
  n_lat, n_lon = GRIDS[which]
  f = np.array(_fields(which, B, C, M))
  two = np.full(n_lat, 2, np.int32)
  src, dst = _handle(gr, B, C), _handle(gr, B, 1)
  try:
    dst.ens_reserve(M)
    _push_all(src, f[:M])

    def nodes(det):
      plan = R.plan_of(C, n_lat, n_lon, [det])
      dst.ens_feature_set(**plan)
      _check(dst, src, f, plan, M)
      count, node, _ = dst.ens_feature_centres()
      return count[..., 0], node[..., 0, :]

    count, node = nodes(_detector(which, 0, 1, two, threshold=-30.0))
    assert np.all(count == 3) and np.all(node[..., :3] == [5, 6 * n_lon, (n_lat - 3) * n_lon + n_lon - 1])
    count, node = nodes(_detector(which, 2, 3, two, ring=False))
    assert np.all(count == 1) and np.all(node[..., 0] == 6 * n_lon + 5)
    count, _ = nodes(_detector(which, 2, 3, two))           # ... whose ring holds no finite value
    assert np.all(count == 0)
    count, node = nodes(_detector(which, 3, n_lat, np.full(n_lat, (n_lon - 1) // 2, np.int32), ring=False))
    assert np.all(node[..., 0] == 0) and np.all(count == 1)  # every other node has an equal one of lower index in its window
    count, node = nodes(_detector(which, 4, 1, two, threshold=0.5, ring=False))
    assert np.all(count == 2) and np.all(node[..., :2] == [5 * n_lon + 7, 9 * n_lon])       # -0.0 == +0.0: the lower node
    count, _ = nodes(_detector(which, 3, 1, two, direction=1, threshold=7.5, ring=False))
    assert np.all(count == 0)                               # a maximum must reach its threshold: 7.25 < 7.5
  finally:
    src.close()
    dst.close()


# ---- 2. three detectors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,B,C,M", SHAPES)
def test_three_detectors_equal_the_definition_and_the_truth_goes_through_a_slot(which, B, C, M):
  gr = _grid(which)[0]
  n_lat, n_lon = GRIDS[which]
  f = np.array(_fields(which, B, C, M))
  cases = _r_lon_cases(which)
  src, dst = _handle(gr, B, C), _handle(gr, B, 3)
  try:
    dst.ens_reserve(M)
    _push_all(src, f[:M])
    plan = None
    for a, r_lat in enumerate(R_LATS):
      for c, r_lon in enumerate(cases):
        dets = [_detector(which, C - 1, r_lat, r_lon, threshold=0.5, strike=(1, cases[2])),                      # min, both tests
                _detector(which, 1, R_LATS[(a + 1) % 3], cases[(c + 1) % 4], direction=1, depth=0.25, strike=(0, 0)),   # max, no threshold
                _detector(which, 4, R_LATS[(a + 2) % 3], cases[(c + 2) % 4], threshold=0.5, ring=False, strike=(2, 1))]  # min, no ring
        plan = R.plan_of(C, n_lat, n_lon, dets)
        dst.ens_feature_set(**plan)
        r_count, _ = _check(dst, src, f, plan, M, msg=f"r_lat {r_lat} r_lon {r_lon.tolist()}")
        assert r_count[..., 2].min() >= 1
    # the truth, through a slot: the fields rotated by one under the last plan
    rot = np.roll(f, -1, axis=0)
    _push_all(src, rot[:M])
    dst.ens_reserve(M)
    _check(dst, src, rot, plan, M, msg="rotated")
    assert dst.counter("ens_feature_calls") == 13
    print(f"{which} ({B}, {C}) M={M} D=3: ens_feature_device_us {dst.counter('ens_feature_device_us')}")
  finally:
    src.close()
    dst.close()


# ---- 3. more centres than the list holds ------------------------------------------------------------------------------------------------
def test_a_full_list_keeps_the_lowest_nodes_and_the_true_count():
  which, B, C, M = "even", 2, 6, 9
  gr = _grid(which)[0]
  n_lat, n_lon = GRIDS[which]
  f = np.array(_fields(which, B, C, M))
  src, dst = _handle(gr, B, C), _handle(gr, B, 2)
  try:
    dst.ens_reserve(M)
    _push_all(src, f[:M])
    # r = 0: every finite node is its own window's extremum; channel 0 holds NaNs, so the lists differ between the fields
    dets = [_detector(which, 0, 0, np.zeros(n_lat, np.int32), ring=False, strike=(0, 0)),
            _detector(which, 5, 1, np.full(n_lat, 2, np.int32), ring=False, strike=(1, 1))]
    plan = R.plan_of(C, n_lat, n_lon, dets, max_centres=2)
    dst.ens_feature_set(**plan)
    r_count, r_strike = _check(dst, src, f, plan, M)
    count, node, _ = dst.ens_feature_centres()
    finite = np.isfinite(f[..., 0]).sum(axis=1)              # [M + 1, B]
    np.testing.assert_array_equal(count[..., 0], finite)
    assert node.shape[-1] == 2 and count[..., 0].min() > 250 and count[..., 1].min() > 2
    first_two = np.stack([[np.flatnonzero(np.isfinite(f[z, :, b, 0]))[:2] for b in range(B)] for z in range(M + 1)])
    np.testing.assert_array_equal(node[..., 0, :], first_two)
    # the strike field uses ALL centres: with r = 0 and a strike window of the node itself it is 1 wherever the source is finite
    got = np.stack([dst.ens_download_member(i) for i in range(M)])
    np.testing.assert_array_equal(got[..., 0], np.where(np.isfinite(f[:M, ..., 0]), np.float32(1.0), np.float32(np.nan)))
    assert (got[..., 1] == 1.0).sum() > 9 * 3 * M
  finally:
    src.close()
    dst.close()


# ---- 4. the scorers of the destination, determinism, state ------------------------------------------------------------------------------
def test_the_scorers_see_the_strike_store_and_a_second_call_gives_the_same_bytes():
  which, B, C, M = "even", 2, 6, 9
  gr = _grid(which)[0]
  n_lat, n_lon = GRIDS[which]
  G = n_lat * n_lon
  f = np.array(_fields(which, B, C, M))
  cases = _r_lon_cases(which)
  dets = [_detector(which, 0, 1, cases[1], threshold=0.5, strike=(1, cases[2])),
          _detector(which, 5, 3, cases[2], direction=1, strike=(2, 2))]
  plan = R.plan_of(C, n_lat, n_lon, dets)
  w = np.random.default_rng(5).uniform(0.5, 1.5, G).astype(np.float32)
  src, dst, third = _handle(gr, B, C), _handle(gr, B, 2), _handle(gr, B, 2)
  try:
    _push_all(src, f[:M])
    src.ens_set_node_weight(w)
    before = src.ens_score(f[M])
    dst.ens_reserve(M)
    dst.ens_set_node_weight(w)
    dst.ens_feature_set(**plan)
    dst.ens_feature(src)                                       # the truth of the source's ens_score
    _, _, _, ref = R.apply(f, plan)
    _push_all(third, ref[:M])
    third.ens_set_node_weight(w)
    a = dst.ens_score(None, want_fields=True) + dst.ens_download_fields()
    b = third.ens_score(ref[M], want_fields=True) + third.ens_download_fields()
    for x, y in zip(a, b):
      assert x.tobytes() == y.tobytes()
    assert dst.counter("ens_invalid_points") == third.counter("ens_invalid_points") > 0
    first = [dst.ens_download_member(i) for i in range(M)] + list(dst.ens_feature_centres()) + list(dst.ens_score(None))
    dst.ens_feature(src)
    with pytest.raises(_lib.GencastHipError, match="no mean / variance"):      # the fields were of the store before
      dst.ens_download_fields()
    second = [dst.ens_download_member(i) for i in range(M)] + list(dst.ens_feature_centres()) + list(dst.ens_score(None))
    for x, y in zip(first, second):
      assert x.tobytes() == y.tobytes()
    # the source: members and scores as they were
    for i in range(M):
      assert src.ens_download_member(i).tobytes() == f[i].tobytes()
    for x, y in zip(before, src.ens_score(None)):
      assert x.tobytes() == y.tobytes()
    # the plan survives gc_ens_reserve; rounds of set / call replace their buffers, they do not grow
    dst.ens_reserve(M)
    dst.ens_feature(src)
    assert dst.ens_download_member(M - 1).tobytes() == first[M - 1].tobytes()
    calls = dst.counter("ens_feature_calls")
    assert calls == 3

    def round_(r):
      dst.ens_feature_set(**R.plan_of(C, n_lat, n_lon, [_detector(which, r % 6, R_LATS[r % 3], cases[r % 4], ring=r % 2 == 0)] * 2,
                                      max_centres=(4, 64)[r % 2]))
      dst.ens_feature(src)

    for r in range(2):
      round_(r)
    flat = dst.counter("device_allocations"), src.counter("device_allocations")
    for r in range(2, 10):
      round_(r)
      assert (dst.counter("device_allocations"), src.counter("device_allocations")) == flat
    assert dst.counter("ens_feature_calls") == calls + 10 and dst.counter("ens_feature_device_us") >= 0
  finally:
    for h in (src, dst, third):
      h.close()


# ---- 5. every documented error ----------------------------------------------------------------------------------------------------------
def test_every_documented_error():
  gr = _grid("even")[0]
  G, B, C, D, M = gr.num_grid_nodes, 2, 6, 2, 2
  f = np.array(_fields("even", B, C, 9))[:M + 1]
  members, truth = f[:M], f[M]
  two = np.full(13, 2, np.int32)
  good = R.plan_of(C, 13, 24, [_detector("even", 0, 1, two, threshold=0.5), _detector("even", 1, 2, two, direction=1)])
  dp = _lib.ctypes.POINTER(_lib.ctypes.c_double)
  I, F = _lib._i32p, _lib._f32p
  INV, STATE, UNSUP = _lib.GC_ERR_INVALID_ARGUMENT, _lib.GC_ERR_STATE, _lib.GC_ERR_UNSUPPORTED
  p = lambda x, ty: None if x is None else np.ascontiguousarray(x).ctypes.data_as(ty)
  err = lambda h: h._lib.gc_last_error(h._h).decode()

  def c_set(h, D=D, **kw):
    a = {k: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for k, v in {**good, **kw}.items()}
    keep.append(a)
    return h._lib.gc_ens_feature_set(h._h, a["c_src"], D, p(a["channel"], I), p(a["direction"], I), p(a["use_threshold"], I),
                                     p(a["threshold"], F), a["n_lat"], a["n_lon"], p(a["r_lat"], I), p(a["r_lon"], I), p(a["ring_lat"], I),
                                     p(a["ring_lon"], I), p(a["depth"], dp), p(a["strike_lat"], I), p(a["strike_lon"], I), a["max_centres"])

  keep = []
  i32 = lambda *v: np.array(v, np.int32)
  lon_bad = lambda v: np.where(np.arange(26).reshape(2, 13) == 17, v, 2).astype(np.int32)
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=D + 4, c_out=D, batch=B)
  src, dst, other_b, other_c = _handle(gr, B, C), _handle(gr, B, D), _handle(gr, B + 1, C), _handle(gr, B, C + 1)
  small, wide = _handle(_grid("odd")[0], B, C), _handle(gr, B, 9)
  lib = dst._lib
  try:
    # ---- gc_ens_feature_set
    assert c_set(bare) == STATE and "gc_set_graph" in err(bare)       # before gc_set_graph
    assert lib.gc_ens_feature(bare._h, src._h, None) == STATE
    assert c_set(dst) == _lib.GC_OK
    for key in ("channel", "direction", "use_threshold", "threshold", "r_lat", "r_lon", "ring_lat", "ring_lon", "depth", "strike_lat",
                "strike_lon"):
      assert c_set(dst, **{key: None}) == INV and err(dst) == "null argument", key
    for kw, msg in ((dict(c_src=0), "c_src must be positive"), (dict(n_lat=12), "n_lat * n_lon"), (dict(n_lat=24, n_lon=14), "n_lat * n_lon"),
                    (dict(n_lat=0, n_lon=0), "n_lat * n_lon"), (dict(D=1), "D must lie in 1 .. 8 and equal c_out"), (dict(D=3), "D must"),
                    (dict(max_centres=0), "max_centres outside 1 .. 1024"), (dict(max_centres=1025), "max_centres"),
                    (dict(channel=i32(0, 6)), "detector 1: source channel outside"), (dict(channel=i32(-1, 1)), "detector 0: source channel"),
                    (dict(c_src=1), "source channel"), (dict(direction=i32(-1, 0)), "detector 1: direction is 0"),
                    (dict(threshold=np.array([np.nan, 0.0], np.float32)), "detector 0: threshold is not finite"),
                    (dict(r_lat=i32(1, -1)), "detector 1: r_lat is negative"), (dict(ring_lat=i32(-2, 3)), "detector 0: ring_lat is negative"),
                    (dict(strike_lat=i32(1, -1)), "detector 1: strike_lat is negative"),
                    (dict(depth=np.array([0.5, np.inf])), "detector 1: depth is not finite"),
                    (dict(depth=np.array([np.nan, 0.5])), "detector 0: depth is not finite"),
                    (dict(r_lon=lon_bad(12)), "detector 1: r_lon[4] outside 0 .. (n_lon - 1) / 2"),
                    (dict(ring_lon=lon_bad(-1)), "detector 1: ring_lon[4] outside"), (dict(strike_lon=lon_bad(12)), "detector 1: strike_lon[4]")):
      assert c_set(dst, **kw) == INV, kw
      assert msg is None or msg in err(dst), (kw, err(dst))
    # a threshold that is not in use, and the depth of a ring that is not, may be anything
    assert c_set(dst, threshold=np.array([0.5, np.nan], np.float32)) == _lib.GC_OK
    assert c_set(dst, ring_lat=i32(2, 0), depth=np.array([0.5, np.nan])) == _lib.GC_OK
    assert c_set(wide, D=9) == INV                            # more than 8 detectors
    for bad in (dict(channel=i32(0)), dict(channel=i32(0, 6)), dict(direction=i32(0, 1)), dict(threshold=np.array([np.inf, 0.0])),
                dict(c_src=0), dict(n_lat=12), dict(n_lat=None), dict(r_lat=i32(1, -1)), dict(ring_lat=i32(-1, 1)), dict(strike_lat=i32(-1, 1)),
                dict(depth=np.array([np.nan, 1.0])), dict(depth=np.zeros(3)), dict(r_lon=two), dict(r_lon=lon_bad(12)), dict(ring_lon=lon_bad(-1)),
                dict(strike_lon=np.full((2, 12), 2)), dict(max_centres=0), dict(max_centres=1025), dict(max_centres=2.5)):
      with pytest.raises(ValueError):
        dst.ens_feature_set(**{**good, **bad})
    with pytest.raises(ValueError, match="c_out in 1 .. 8"):
      wide.ens_feature_set(**good)
    # a row that does not fit the LDS of the row pass: 4097 longitudes (0.25 degrees fits: test_a_quarter_degree_row_fits)
    from gencast_flax_nnx_amd import geometry
    long_gr = geometry.build_denoiser_graph(grid_lat=np.array([-45.0, 45.0]), grid_lon=np.arange(4097) * (360.0 / 4097), mesh_size=2,
                                            attention_k_hop=2)
    long_row = _handle(long_gr, 1, 1)
    try:
      z1, z2 = np.zeros(1, np.int32), np.zeros((1, 2), np.int32)
      rc = c_set(long_row, D=1, c_src=1, channel=z1, direction=z1 - 1, use_threshold=z1, threshold=np.zeros(1, np.float32), n_lat=2,
                 n_lon=4097, r_lat=z1, r_lon=z2, ring_lat=z1, ring_lon=z2, depth=np.zeros(1), strike_lat=z1, strike_lon=z2)
      assert rc == UNSUP and "n_lon is too large" in err(long_row) and "64 KB of LDS" in err(long_row)
    finally:
      long_row.close()
    # ---- gc_ens_feature and gc_ens_feature_centres
    fresh = _handle(gr, B, D)
    try:
      with pytest.raises(_lib.GencastHipError, match="no plan"):
        fresh.ens_feature(src)
      assert lib.gc_ens_feature(fresh._h, src._h, None) == STATE and "no plan" in err(fresh)
      with pytest.raises(_lib.GencastHipError, match="no centre lists"):
        fresh.ens_feature_centres()
      cnt = np.zeros(8, np.int32)
      assert lib.gc_ens_feature_centres(fresh._h, p(cnt, I), p(cnt, I), p(cnt.astype(np.float32), F)) == STATE
      assert lib.gc_ens_feature_centres(fresh._h, None, p(cnt, I), None) == INV
    finally:
      fresh.close()
    dst.ens_feature_set(**good)
    with pytest.raises(_lib.GencastHipError, match="no centre lists"):
      dst.ens_feature_centres()
    assert lib.gc_ens_feature(dst._h, dst._h, None) == INV and lib.gc_ens_feature(dst._h, None, None) == INV
    for bad in (dst, None, "src"):
      with pytest.raises(ValueError, match="another NativeDenoiser"):
        dst.ens_feature(bad)
    for h in (bare, other_b, other_c, small):                 # no graph; another batch; c_out != c_src; another G
      assert lib.gc_ens_feature(dst._h, h._h, None) == INV and "other dimensions" in err(dst)
    with pytest.raises(_lib.GencastHipError, match="no member store"):       # on dst
      dst.ens_feature(src, truth)
    dst.ens_reserve(M)
    with pytest.raises(_lib.GencastHipError, match="no member store on the source"):
      dst.ens_feature(src, truth)
    src.ens_reserve(M + 1)
    with pytest.raises(_lib.GencastHipError, match="different numbers of members"):
      dst.ens_feature(src, truth)
    src.ens_reserve(M)
    src.ens_push_host(0, members[0])
    with pytest.raises(_lib.GencastHipError, match="source member slot 1 has not been pushed"):
      dst.ens_feature(src, truth)
    src.ens_push_host(1, members[1])
    with pytest.raises(_lib.GencastHipError, match="no truth on the source"):
      dst.ens_feature(src)
    assert lib.gc_ens_feature(dst._h, src._h, None) == STATE
    with pytest.raises(ValueError, match="truth must be"):
      dst.ens_feature(src, truth[..., :D])
    assert dst.counter("ens_feature_calls") == 0
    dst.ens_feature(src, truth)
    dst.ens_feature(src)                                       # the truth stays in the source
    assert dst.counter("ens_feature_calls") == 2
    count, node, value = dst.ens_feature_centres()
    assert count.shape == (M + 1, B, D) and node.shape == value.shape == (M + 1, B, D, 64)
    dst.ens_feature_set(**good)                                # a new plan: the lists of the old one are gone
    with pytest.raises(_lib.GencastHipError, match="no centre lists"):
      dst.ens_feature_centres()
    with pytest.raises(ValueError):
      dst.counter("ens_feature_no_such_counter")
  finally:
    for h in (bare, src, dst, other_b, other_c, small, wide):
      h.close()


# ---- 6. a row of 1440 longitudes ----------------------------------------------------------------------------------------------------------
def test_a_quarter_degree_row_fits():
  """n_lon = 1440: every thread of the row pass owns several longitudes, the column pass has twelve blocks and the list pass
  several blocks per thread's segment.  Two rows, so that the reference stays cheap; the pole-like row takes the whole row."""
  from gencast_flax_nnx_amd import geometry
  n_lat, n_lon, B, C, M = 2, 1440, 1, 2, 2
  gr = geometry.build_denoiser_graph(grid_lat=np.array([-45.0, 45.0]), grid_lon=np.arange(n_lon) * 0.25, mesh_size=2, attention_k_hop=2)
  G = n_lat * n_lon
  rng = np.random.default_rng(1440)
  f = np.moveaxis(_smooth(rng, n_lat, n_lon, (M + 1, B, C)), 0, 1).copy()
  f[rng.integers(0, M + 1, 40), rng.integers(0, G, 40), 0, 0] = np.nan
  f[:, [0, n_lon - 1], :, 0] = np.float32(-30.0)            # a tie across the wrap: node 0 takes it
  f[:, [n_lon + 700, 2 * n_lon - 1], :, 0] = np.float32(-28.0)     # ... and what its ring finds a row apart
  dets = [dict(channel=0, direction=-1, threshold=0.0, r_lat=1, r_lon=np.array([719, 257]), ring_lat=1, ring_lon=np.array([300, 200]),
               depth=0.25, strike_lat=1, strike_lon=np.array([130, 2]))]
  plan = R.plan_of(C, n_lat, n_lon, dets, max_centres=16)
  src, dst = _handle(gr, B, C), _handle(gr, B, 1)
  try:
    dst.ens_reserve(M)
    _push_all(src, f[:M])
    dst.ens_feature_set(**plan)
    r_count, _ = _check(dst, src, f, plan, M)
    assert r_count.min() >= 1 and dst.ens_feature_centres()[1][0, 0, 0, 0] == 0
    print(f"2 x 1440 M={M}: centres {r_count.sum(axis=(0, 1)).tolist()}, ens_feature_device_us {dst.counter('ens_feature_device_us')}")
  finally:
    src.close()
    dst.close()
