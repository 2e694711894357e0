"""The fractions sums on the device (gc_ens_fss_*) against the definition restated in
tests/fss_reference.py (its row-and-column form, which tests/test_fss.py holds to the literal one).

A, B, N and M N are integers that double holds exactly, a lone double division is correctly rounded on both sides (the build
has no fast-math flag) and so is the conversion to float32: the fields `prob` and `obs` are compared with ==, NaN pattern
included.  The per-term values of the sums are then bit-equal and only the order of addition differs: for non-negative terms
|got - ref| <= G 2^-53 ref + spacing(ref), ref the math.fsum value, computed here per sum.

Sizes, as in tests/test_gpu_derive.py: the 13 x 24 grid (G = 312) and the 11 x 15 grid (G = 165, odd everything), handles with
set_graph only.  (B, C) = (2, 6): one partial row tile of 16 columns; (1, 82): three row tiles of 32, a chunk of 96 columns
with 64 idle threads in the column pass; (4, 82): W = 328, two chunks of columns, the second partial; (1, 7) on the odd grid:
a tile of 8; (1, 257): a second chunk with one live column.  S = 4 scales pair r_lat in {0, 1, 3, 12} (12 covers the whole column) with r_lon all 0, all 2, a 2500 km window
(capped at the poles) and all (n_lon - 1) // 2; at 15 longitudes that is the whole row."""
import functools

import numpy as np
import pytest

from gencast_flax_nnx_amd import DerivedSpec, EventScores, _lib, losses
from gencast_flax_nnx_amd.verification import FractionsScores, quantize_node_weights, quantize_row_weights
from tests import event_reference as ER
from tests import fss_reference as R
from tests import helpers
from tests.helpers import graph_handle as _handle

pytestmark = pytest.mark.gpu

GRIDS = {"even": (13, 24), "odd": (11, 15)}
SHAPES = [("even", 2, 6, 9), ("even", 1, 82, 2), ("even", 4, 82, 2), ("odd", 1, 7, 2), ("even", 1, 257, 3)]   # grid, B, C, M
R_LATS = np.array([0, 1, 3, 12], np.int32)


@functools.lru_cache(maxsize=None)
def _grid(which):
  from gencast_flax_nnx_amd import geometry
  n_lat, n_lon = GRIDS[which]
  lat, lon = np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=2, attention_k_hop=2)
  assert gr.num_grid_nodes == n_lat * n_lon
  cap = (n_lon - 1) // 2
  by_radius = DerivedSpec.window(lat, lon, 2500.0)[1]
  assert by_radius[0] == by_radius[-1] == cap and by_radius.min() < cap          # the pole rows are capped, the others not
  r_lons = np.stack([np.zeros(n_lat, np.int32), np.full(n_lat, 2, np.int32), by_radius, np.full(n_lat, cap, np.int32)])
  return gr, r_lons.astype(np.int32), quantize_row_weights(losses.normalized_latitude_weights(lat))


def _push_all(nd, members):
  nd.ens_reserve(len(members))
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _inputs(which, B, C, M, T, seed):
  """`event_reference.data` with every kind of point that does not count.  T = 3: directions (+, +, -); T = 1: the third
  threshold alone, direction -."""
  n_lat, n_lon = GRIDS[which]
  G = n_lat * n_lon
  members, truth, w, thr, d = ER.data(M, G, B, C, seed, T=3)
  rng = np.random.default_rng(seed + 100)
  n = 25
  members[rng.integers(0, M, n), rng.integers(0, G, n), rng.integers(0, B, n), 0] = np.nan          # scattered NaN
  truth[rng.integers(0, G, n), rng.integers(0, B, n), 1] = np.nan
  thr[rng.integers(0, 3, n), rng.integers(0, G, n), rng.integers(0, B, n), 1] = np.nan
  truth[4 * n_lon:5 * n_lon, 0, 2] = np.nan                 # one whole latitude row
  truth[:, B - 1, 3] = np.nan                               # one whole (b, c) column
  lone = truth[6 * n_lon + 5, 0, 4]
  truth[:, 0, 4] = np.nan                                   # a counted centre, its whole window otherwise not counted
  truth[6 * n_lon + 5, 0, 4] = lone
  members[:, :, B - 1, 5] = 0.0                             # a constant column: nobody is in the event
  truth[:, B - 1, 5] = 0.0
  if T == 1:
    thr, d = np.ascontiguousarray(thr[2:3]), d[2:3].copy()
  return members, truth, w, thr, d


def _check_sums(tag, got, ref, G):
  """The bound, per sum; -> the worst ratio of error to bound."""
  assert got.shape == ref.shape and got.dtype == np.float64
  assert (ref >= 0.0).all() and np.isfinite(got).all()
  err, lim = np.abs(got - ref), R.bound(ref, G)
  worst = float(np.max(err / lim))
  print(f"{tag}: worst |got - ref| / bound = {worst:.3f}")
  assert (err <= lim).all(), f"{tag}: {np.argwhere(err > lim)[:5]}"
  return worst


CASES = [shape + (T,) for shape in SHAPES for T in (1, 3)]


# ---- 1. fields and sums against the definition ------------------------------------------------------------------------------
@pytest.mark.parametrize("which,B,C,M,T", CASES)
def test_fields_and_sums_equal_the_definition(which, B, C, M, T):
  gr, r_lons, row_wq = _grid(which)
  n_lat, n_lon = GRIDS[which]
  G = n_lat * n_lon
  members, truth, w, thr, d = _inputs(which, B, C, M, T, seed=7 + C + T)
  wq, scale = quantize_node_weights(w)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members)
    nd.ens_event_set(thr, d, wq)
    nd.ens_fss_set(R_LATS, r_lons, row_wq)
    weighted, counts, _ = nd.ens_event_score(truth)
    code = np.stack([nd.ens_event_codes(t) for t in range(T)])
    np.testing.assert_array_equal(code, ER.tables(members, truth, thr, d, wq)["code"])
    ref = R.separable(code, M, n_lat, n_lon, R_LATS, r_lons, row_wq, wq)
    sums = nd.ens_fss_score()
    assert sums.shape == (T, 4, B, C, 4)
    # fields: ==, NaN pattern included
    for t in range(T):
      for s in range(4):
        prob, obs = nd.ens_fss_fields(t, s)
        assert prob.dtype == obs.dtype == np.float32 and prob.shape == (G, B, C)
        np.testing.assert_array_equal(prob, ref["prob"][t, s], err_msg=f"prob t={t} s={s}")
        np.testing.assert_array_equal(obs, ref["obs"][t, s], err_msg=f"obs t={t} s={s}")
        assert (np.isnan(prob) == (code[t] == 255)).all() and (np.isnan(obs) == (code[t] == 255)).all()
    # sums: the bound of a reordered sum
    _check_sums(f"{which} ({B}, {C}, {M}) T={T}", sums, ref["sums"], G)
    # what does not count
    assert (code[:, :, B - 1, 3] == 255).all()
    np.testing.assert_array_equal(sums[:, :, B - 1, 3], 0.0)                    # a column with no counted point: four zeros
    assert (code[:, :, 0, 4] != 255).sum() == T                                 # the lone centre sees itself only
    for t in range(T):
      c = int(code[t, 6 * n_lon + 5, 0, 4])
      p, o = nd.ens_fss_fields(t, 3)
      assert p[6 * n_lon + 5, 0, 4] == np.float32((c & 127) / M) and o[6 * n_lon + 5, 0, 4] == np.float32(c >> 7)
    assert (code[:, :, B - 1, 5] == 0).all()
    np.testing.assert_array_equal(sums[:, :, B - 1, 5, 1], 0.0)                 # nobody in the event: sums[1] = 0
    fr = FractionsScores(sums, weighted.sum(axis=(-1, -2)), M, d, (0.0, 1.0, 2.0, 3.0), scale)
    assert np.isnan(fr.fss[:, :, B - 1, 3]).all() and np.isnan(fr.fss[:, :, B - 1, 5]).all()
    assert np.isfinite(fr.fss[:, :, 0, 0]).all()
    # against what exists: at the point scale the fractions Brier score is the Brier score, the observed fraction the base rate
    ev = EventScores(weighted, counts, M, d, scale)
    np.testing.assert_array_equal(fr.weight, (ev.valid_weight * scale).astype(np.uint64))
    np.testing.assert_array_equal(fr.valid_weight, ev.valid_weight)
    with np.errstate(invalid="ignore"):
      brier_w = np.where(ev.valid_weight > 0, ev.brier * ev.valid_weight, 0.0)
      rate_w = np.where(ev.valid_weight > 0, ev.base_rate * ev.valid_weight, 0.0)
    for got, want in ((sums[:, 0, :, :, 0] / scale, brier_w), (sums[:, 0, :, :, 3] / scale, rate_w)):
      assert (np.abs(got - want) <= R.bound(want, G)).all()
    if which == "odd":                                       # the whole sphere: P and O are constants of the column
      assert R_LATS[3] >= n_lat - 1 and 2 * r_lons[3].min() + 1 == n_lon
      for t in range(T):
        for f in nd.ens_fss_fields(t, 3):
          spread = np.where(np.isnan(f), -np.inf, f).max(axis=0) - np.where(np.isnan(f), np.inf, f).min(axis=0)
          assert ((spread == 0.0) | (spread == -np.inf)).all() and (spread == 0.0).sum() >= B * C - 1
    assert nd.counter("ens_fss_calls") == 1 and nd.counter("ens_fss_device_us") >= 0
    print(f"{which} ({B}, {C}, {M}) T={T}: ens_fss_device_us {nd.counter('ens_fss_device_us')}")
  finally:
    nd.close()


# ---- 2. the displacement law, through real members, thresholds and truth --------------------------------------------------------
def test_displacement_law_on_the_device():
  gr, _, row_wq = _grid("even")
  n_lat, n_lon = GRIDS["even"]
  G, B, C, M = n_lat * n_lon, 1, 3, 4
  code = R.displacement_codes(n_lat, n_lon, M, 3).reshape(G)
  truth = np.zeros((G, B, C), np.float32)
  truth[code >> 7 == 1] = 1.0
  members = np.zeros((M, G, B, C), np.float32)
  members[:, (code & 127) == M] = 1.0
  thr = np.full((1, G, B, C), 0.5, np.float32)
  wq = np.repeat(row_wq, n_lon).astype(np.uint32)
  radii = (0, 1, 3, 5)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members)
    nd.ens_event_set(thr, np.array([1], np.int32), wq)
    nd.ens_fss_set(np.zeros(4, np.int32), np.stack([np.full(n_lat, r, np.int32) for r in radii]), row_wq)
    nd.ens_event_score(truth)
    np.testing.assert_array_equal(nd.ens_event_codes(0)[:, 0, 0], code)
    sums = nd.ens_fss_score()
    fss = 1.0 - sums[0, :, 0, :, 0] / sums[0, :, 0, :, 1]
    for s, r in enumerate(radii):
      want = max(0, 2 * r + 1 - 3) / (2 * r + 1)
      assert (np.abs(fss[s] - want) <= 1e-15).all(), (r, fss[s], want)
  finally:
    nd.close()


# ---- 3. determinism and ownership -----------------------------------------------------------------------------------------------
def test_determinism_and_ownership():
  gr, r_lons, row_wq = _grid("even")
  n_lat, n_lon = GRIDS["even"]
  G, B, C, M, T = n_lat * n_lon, 2, 6, 5, 3
  members, truth, w, thr, d = _inputs("even", B, C, M, T, seed=51)
  wq, _ = quantize_node_weights(w)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members)
    nd.ens_event_set(thr, d, wq)
    tables = nd.ens_event_score(truth)
    codes = [nd.ens_event_codes(t) for t in range(T)]
    nd.ens_fss_set(R_LATS, r_lons, row_wq)
    a = nd.ens_fss_score()
    fa = nd.ens_fss_fields(2, 2)
    b = nd.ens_fss_score()
    fb = nd.ens_fss_fields(2, 2)
    assert a.tobytes() == b.tobytes() and fa[0].tobytes() == fb[0].tobytes() and fa[1].tobytes() == fb[1].tobytes()
    # the codes and the members are what they were; the event tables come out the same again
    for t in range(T):
      assert nd.ens_event_codes(t).tobytes() == codes[t].tobytes()
    for i in range(M):
      np.testing.assert_array_equal(nd.ens_download_member(i), members[i])
    again = nd.ens_event_score(None)
    for x, y in zip(tables, again):
      assert x.tobytes() == y.tobytes()
    assert nd.ens_fss_score().tobytes() == a.tobytes()
    # the plan survives ens_reserve; the codes do not
    held = nd.counter("device_allocations")
    _push_all(nd, members)
    with pytest.raises(_lib.GencastHipError, match="no valid event codes"):
      nd.ens_fss_score()
    nd.ens_event_score(None)
    assert nd.ens_fss_score().tobytes() == a.tobytes()
    assert nd.counter("device_allocations") == held
    # twenty rounds of set / score with alternating S: replaced, not grown
    for r in range(20):
      S = 2 if r % 2 else 4
      nd.ens_fss_set(R_LATS[:S], r_lons[:S], row_wq)
      got = nd.ens_fss_score()
      assert got.shape[1] == S and nd.counter("device_allocations") == held
      assert got.tobytes() == np.ascontiguousarray(a[:, :S]).tobytes()
    assert nd.counter("ens_fss_calls") == 24
  finally:
    nd.close()


def test_an_fss_call_leaves_the_sampler_state_alone():
  from oracle import gencast_oracle as O
  gr, dims, params, cond, _ = helpers.tiny_setup(batch=2, seed=2)
  _, r_lons, row_wq = _grid("even")
  rng = np.random.default_rng(8)
  G = gr.num_grid_nodes
  assert G == 312
  noise = rng.standard_normal((G, 2, dims.c_out)).astype(np.float32)
  truth = rng.standard_normal((G, 2, dims.c_out)).astype(np.float32)
  thr = np.zeros((2, G, 2, dims.c_out), np.float32)
  thr[1] = 0.5
  d = np.array([1, -1], np.int32)
  wq, _ = quantize_node_weights(np.linspace(0.5, 1.5, G))
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    nd.set_option("graphs", "on")
    nd.set_noisy_slots(np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32))
    nd.upload_cond(cond)
    nd.upload_noise(noise)
    sched = O.noise_schedule(80.0, 0.03, 4, 7.0).astype(np.float32)
    nd.sample_resident(sched)
    first = nd.download_sample()
    nd.sample_resident(sched)                                      # captured here
    np.testing.assert_array_equal(nd.download_sample(), first)
    replays, captures = nd.counter("graph_replays"), nd.counter("graph_captures")
    nd.ens_reserve(2)
    nd.ens_push(0)
    nd.ens_push_host(1, -first)
    nd.ens_event_set(thr, d, wq)
    nd.ens_fss_set(R_LATS, r_lons, row_wq)
    nd.ens_event_score(truth)
    sums = nd.ens_fss_score()
    nd.ens_fss_fields(1, 2)
    code = np.stack([nd.ens_event_codes(t) for t in range(2)])
    _check_sums("pushed samples", sums, R.separable(code, 2, 13, 24, R_LATS, r_lons, row_wq, wq)["sums"], G)
    np.testing.assert_array_equal(nd.download_sample(), first)      # the last sample is still there
    np.testing.assert_array_equal(nd.download_cond(), cond)
    np.testing.assert_array_equal(nd.download_noise(), noise)
    nd.sample_resident(sched)                                      # a replay of the captured graph: the same bytes
    np.testing.assert_array_equal(nd.download_sample(), first)
    assert nd.counter("graph_captures") == captures and nd.counter("graph_replays") == replays + 1
  finally:
    nd.close()


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------
def test_every_documented_error():
  gr, r_lons, row_wq = _grid("even")
  n_lat, n_lon = GRIDS["even"]
  G, B, C, M, T = n_lat * n_lon, 2, 6, 2, 2
  members, truth, w, thr, d = ER.data(M, G, B, C, seed=41, T=T)
  wq, _ = quantize_node_weights(w)
  ct = _lib.ctypes
  i32, u32, f64 = _lib._i32p, ct.POINTER(ct.c_uint32), ct.POINTER(ct.c_double)
  p = lambda a, ty: a.ctypes.data_as(ty)
  rl, ro = R_LATS.copy(), np.ascontiguousarray(r_lons)
  out = np.zeros((T, 8, B, C, 4))
  f1, f2 = np.zeros((G, B, C), np.float32), np.zeros((G, B, C), np.float32)
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  try:                                                        # before gc_set_graph: every entry
    assert bare._lib.gc_ens_fss_set(bare._h, 4, n_lat, n_lon, p(rl, i32), p(ro, i32), p(row_wq, u32)) == _lib.GC_ERR_STATE
    assert bare._lib.gc_ens_fss_score(bare._h, p(out, f64)) == _lib.GC_ERR_STATE
    assert bare._lib.gc_ens_fss_fields(bare._h, 0, 0, p(f1, _lib._f32p), p(f2, _lib._f32p)) == _lib.GC_ERR_STATE
  finally:
    bare.close()
  nd = _handle(gr, B, C)
  lib, h = nd._lib, nd._h
  fss_set = lambda S=4, a=n_lat, b=n_lon, x=rl, y=ro, z=row_wq: lib.gc_ens_fss_set(
      h, S, a, b, None if x is None else p(x, i32), None if y is None else p(y, i32), None if z is None else p(z, u32))
  try:
    # no plan
    assert lib.gc_ens_fss_score(h, p(out, f64)) == _lib.GC_ERR_STATE
    assert lib.gc_ens_fss_fields(h, 0, 0, p(f1, _lib._f32p), p(f2, _lib._f32p)) == _lib.GC_ERR_STATE
    with pytest.raises(_lib.GencastHipError, match="ens_fss_set"):
      nd.ens_fss_score()
    # gc_ens_fss_set
    assert fss_set(S=0) == _lib.GC_ERR_UNSUPPORTED and fss_set(S=9) == _lib.GC_ERR_UNSUPPORTED
    assert fss_set(a=1, b=16385) == _lib.GC_ERR_UNSUPPORTED
    for kw in (dict(x=None), dict(y=None), dict(z=None)):
      assert fss_set(**kw) == _lib.GC_ERR_INVALID_ARGUMENT
    assert fss_set(a=n_lat, b=n_lon + 1) == _lib.GC_ERR_INVALID_ARGUMENT
    neg = rl.copy()
    neg[2] = -1
    assert fss_set(x=neg) == _lib.GC_ERR_INVALID_ARGUMENT
    for bad in (-1, (n_lon - 1) // 2 + 1):
      wide = ro.copy()
      wide[3, 5] = bad
      assert fss_set(y=wide) == _lib.GC_ERR_INVALID_ARGUMENT
    for bad in (0, 2 ** 24):
      zero = row_wq.copy()
      zero[7] = bad
      assert fss_set(z=zero) == _lib.GC_ERR_INVALID_ARGUMENT
    top = row_wq.copy()
    top[7] = 2 ** 24 - 1
    assert fss_set(z=top) == _lib.GC_OK
    with pytest.raises(ValueError):
      nd.ens_fss_set(R_LATS, r_lons[:, :-1], row_wq)
    nd.ens_fss_set(R_LATS, r_lons, row_wq)
    # no valid codes: no thresholds; thresholds but no scoring call; after a new ens_event_set; after ens_reserve
    assert lib.gc_ens_fss_score(h, p(out, f64)) == _lib.GC_ERR_STATE
    with pytest.raises(_lib.GencastHipError, match="ens_event_set"):
      nd.ens_fss_score()
    nd.ens_event_set(thr, d, wq)
    assert lib.gc_ens_fss_score(h, p(out, f64)) == _lib.GC_ERR_STATE
    with pytest.raises(_lib.GencastHipError, match="no valid event codes"):
      nd.ens_fss_fields(0, 0)
    _push_all(nd, members)
    nd.ens_event_score(truth)
    assert lib.gc_ens_fss_score(h, p(out, f64)) == _lib.GC_OK
    nd.ens_event_set(thr, d, wq)
    assert lib.gc_ens_fss_score(h, p(out, f64)) == _lib.GC_ERR_STATE
    nd.ens_event_score(None)
    assert lib.gc_ens_fss_score(h, p(out, f64)) == _lib.GC_OK
    nd.ens_reserve(M)
    assert lib.gc_ens_fss_score(h, p(out, f64)) == _lib.GC_ERR_STATE
    assert lib.gc_ens_fss_fields(h, 0, 0, p(f1, _lib._f32p), p(f2, _lib._f32p)) == _lib.GC_ERR_STATE
    _push_all(nd, members)
    nd.ens_event_score(None)
    # null pointers; t and s out of range
    assert lib.gc_ens_fss_score(h, None) == _lib.GC_ERR_INVALID_ARGUMENT
    assert lib.gc_ens_fss_fields(h, 0, 0, None, p(f2, _lib._f32p)) == _lib.GC_ERR_INVALID_ARGUMENT
    assert lib.gc_ens_fss_fields(h, 0, 0, p(f1, _lib._f32p), None) == _lib.GC_ERR_INVALID_ARGUMENT
    for t, s in ((-1, 0), (T, 0), (0, -1), (0, 4)):
      assert lib.gc_ens_fss_fields(h, t, s, p(f1, _lib._f32p), p(f2, _lib._f32p)) == _lib.GC_ERR_INVALID_ARGUMENT
      with pytest.raises(ValueError):
        nd.ens_fss_fields(t, s)
    assert lib.gc_ens_fss_fields(h, T - 1, 3, p(f1, _lib._f32p), p(f2, _lib._f32p)) == _lib.GC_OK
    assert lib.gc_ens_fss_set(None, 4, n_lat, n_lon, p(rl, i32), p(ro, i32), p(row_wq, u32)) == _lib.GC_ERR_INVALID_ARGUMENT
    assert lib.gc_ens_fss_score(None, p(out, f64)) == _lib.GC_ERR_INVALID_ARGUMENT
  finally:
    nd.close()
