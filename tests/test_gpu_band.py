"""Spectral band views on the device (gc_ens_band_set / gc_ens_band) against the float64 definition
restated in tests/band_reference.py.

Device and reference send the same float32 data through the same float32 tables in binary64 and differ in summation order
and in the fusing of multiply-adds only, so the bound is the derived one of tests/band_reference.py (u = 2^-53, every
rounding counted, doubled for the reference's own).  The device rounds its binary64 result to float32 once; for every finite
point the assertion is float32(ref - tol) <= got <= float32(ref + tol), and the NaN patterns must be equal: a float32
synthesis or a second rounding cannot pass it.  Every case prints the share of bit-equal values and the worst ratio to the
bound before it asserts."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import BandSpec, SphericalAnalysis, _lib
from tests import band_reference as R
from tests import helpers
from tests.helpers import graph_handle as _handle, small_graph as _graph

pytestmark = pytest.mark.gpu


def _latlon(n_lat, n_lon):
  return np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)


def _tables(n_lat, n_lon, lmax):
  sa = SphericalAnalysis(*_latlon(n_lat, n_lon), lmax)
  return sa.device_tables(), sa.synthesis_tables()


def _data(M, G, B, C, seed, scale):
  rng = np.random.default_rng(seed)
  members = ((rng.standard_normal((M, G, B, C)) + 0.5) * scale).astype(np.float32)
  truth = ((rng.standard_normal((G, B, C)) + 0.5) * scale).astype(np.float32)
  return members, truth


def _push_all(nd, members):
  nd.ens_reserve(len(members))
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _plan(lmax, c_src, src_channel, bands, taper, stabs):
  """The keywords of `ens_band_set`: every band of `bands` on every channel of `src_channel`, band-major."""
  response, complement = BandSpec(bands, taper=taper).responses(lmax)
  K = len(response)
  return dict(c_src=c_src, response=response, complement=complement, src_channel=np.tile(np.asarray(src_channel, np.int32), K),
              band=np.repeat(np.arange(K, dtype=np.int32), len(src_channel)), legendre_synthesis=stabs[0], cos_s=stabs[1],
              sin_s=stabs[2])


def _reference(fields, n_lat, n_lon, plan, atabs, stabs):
  """[(d, tol, bad)] of the fields [M + 1, G, B, c_src]: computed once per case, shared by what checks it."""
  return [R.band_fields(f, n_lat, n_lon, plan["response"], plan["complement"], plan["src_channel"], plan["band"], atabs, stabs)
          for f in fields]


def _download(dst, M):
  return [dst.ens_download_member(i) for i in range(M)]


THREE = {"low": (0, 3), "mid": (4, 8), "high": dict(l=(0, 3), complement=True)}


def _case_13x24(M, seed=5):
  n_lat, n_lon, L, B, C = 13, 24, 12, 2, 6
  atabs, stabs = _tables(n_lat, n_lon, L)
  plan = _plan(L, C, [0, 3, 5], THREE, 1, stabs)             # three bands read by three source channels: c_d = 9
  members, truth = _data(M, n_lat * n_lon, B, C, seed + M, np.logspace(-3, 5, C))
  return n_lat, n_lon, B, C, atabs, stabs, plan, members, truth


# ---- 1. the definition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 8])
def test_band_fields_match_the_float64_definition_13x24(M):
  n_lat, n_lon, B, C, atabs, stabs, plan, members, truth = _case_13x24(M)
  gr = _graph(n_lat, n_lon)
  ref = _reference(list(members) + [truth], n_lat, n_lon, plan, atabs, stabs)
  src, dst, third = _handle(gr, B, C), _handle(gr, B, 9), _handle(gr, B, 9)
  try:
    _push_all(src, members)
    w = np.linspace(0.5, 1.5, gr.num_grid_nodes).astype(np.float32)
    src.ens_set_node_weight(w)
    before = src.ens_score(truth)
    dst.spec_set_tables(*atabs)
    dst.ens_band_set(**plan)
    dst.ens_reserve(M)
    dst.ens_band(src)                                          # the truth of the source's ens_score
    got = _download(dst, M)
    for i in range(M):
      R.check(got[i], ref[i][0], ref[i][1], f"13x24 M={M} member {i}")
    assert dst.counter("ens_band_calls") == 1 and dst.counter("ens_band_invalid_columns") == 0
    assert dst.counter("ens_band_device_us") >= 0
    print(f"13x24 M={M}: ens_band_device_us {dst.counter('ens_band_device_us')}")
    # the band truth has no download of its own: the truth goes through the same map as a member, so it is read back as one
    src.ens_push_host(0, truth)
    dst.ens_band(src)
    band_truth = dst.ens_download_member(0)
    R.check(band_truth, ref[M][0], ref[M][1], f"13x24 M={M} truth")
    src.ens_push_host(0, members[0])
    # a second call returns identical bytes
    dst.ens_band(src)
    for x, y in zip(got, _download(dst, M)):
      assert x.tobytes() == y.tobytes()
    assert dst.counter("ens_band_calls") == 3
    # the scorers of the view: bit-equal to a plain handle into which the downloaded band fields were pushed
    _push_all(third, got)
    for h in (dst, third):
      h.ens_set_node_weight(w)
    a = dst.ens_score(None, want_fields=True) + dst.ens_download_fields()
    b = third.ens_score(band_truth, want_fields=True) + third.ens_download_fields()
    for x, y in zip(a, b):
      assert x.tobytes() == y.tobytes()
    assert np.isfinite(a[0]).all() and a[1].sum() > 0
    # the source: members and scores (so its truth) as they were
    for i in range(M):
      np.testing.assert_array_equal(src.ens_download_member(i), members[i])
    for x, y in zip(before, src.ens_score(None)):
      assert x.tobytes() == y.tobytes()
  finally:
    for h in (src, dst, third):
      h.close()


def test_band_fields_match_the_float64_definition_21x40():
  """c_d = 70 columns cross a 64-lane group; l above 16 crosses a 16-row group, the 21 latitudes and 40 longitudes too; for m
  near lmax - 1 only one l remains."""
  n_lat, n_lon, L, B, C, M = 21, 40, 20, 1, 40, 3
  atabs, stabs = _tables(n_lat, n_lon, L)
  plan = _plan(L, C, list(range(2, 37)), {"planetary": (0, 5), "rest": dict(l=(0, 5), complement=True)}, 0, stabs)
  assert len(plan["band"]) == 70
  members, truth = _data(M, n_lat * n_lon, B, C, 9, np.logspace(-2, 4, C))
  ref = _reference(list(members) + [truth], n_lat, n_lon, plan, atabs, stabs)
  gr = _graph(n_lat, n_lon)
  src, dst = _handle(gr, B, C), _handle(gr, B, 70)
  try:
    _push_all(src, members)
    dst.spec_set_tables(*atabs)
    dst.ens_band_set(**plan)
    dst.ens_reserve(M)
    dst.ens_band(src, truth)
    for i in range(M):
      R.check(dst.ens_download_member(i), ref[i][0], ref[i][1], f"21x40 member {i}")
    # low + complement(low) is the field again, to the two roundings of the two views
    got = dst.ens_download_member(0).astype(np.float64)
    back, f = got[..., :35] + got[..., 35:], members[0][..., 2:37].astype(np.float64)
    ulp = np.spacing(np.maximum(np.abs(got[..., :35]), np.abs(got[..., 35:])).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(back - f) <= ulp + ref[0][1][..., :35] + ref[0][1][..., 35:])
    print(f"21x40: ens_band_device_us {dst.counter('ens_band_device_us')}")
  finally:
    src.close()
    dst.close()


# ---- 2. values that are not finite ----------------------------------------------------------------------------------------------
def test_a_value_that_is_not_finite_marks_the_channels_that_read_it_in_that_field_only():
  M = 2
  n_lat, n_lon, B, C, atabs, stabs, plan, members, truth = _case_13x24(M)
  gr = _graph(n_lat, n_lon)
  dirty = members.copy()
  dirty[1, 100, 1, 3] = np.nan                                 # member 1, batch 1, source channel 3: read by 3 derived channels
  dirty[0, 7, 0, 1] = np.inf                                   # a channel no band reads: nothing happens
  src, dst = _handle(gr, B, C), _handle(gr, B, 9)
  try:
    dst.spec_set_tables(*atabs)
    dst.ens_band_set(**plan)
    dst.ens_reserve(M)
    dst.ens_set_node_weight(np.ones(gr.num_grid_nodes, np.float32))
    _push_all(src, members)
    dst.ens_band(src, truth)
    clean = _download(dst, M)
    dst.ens_score(None)
    assert dst.counter("ens_band_invalid_columns") == 0 and dst.counter("ens_invalid_points") == 0
    _push_all(src, dirty)
    dst.ens_band(src)
    got = _download(dst, M)
    reads = plan["src_channel"] == 3
    assert reads.sum() == 3
    assert np.isnan(got[1][:, 1, reads]).all()
    keep = np.ones(got[1].shape, bool)
    keep[:, 1, reads] = False
    assert got[1][keep].tobytes() == clean[1][keep].tobytes() and got[0].tobytes() == clean[0].tobytes()
    assert dst.counter("ens_band_invalid_columns") == 1
    dst.ens_score(None)
    assert dst.counter("ens_invalid_points") == 3 * gr.num_grid_nodes
    # the truth goes through the same map
    bad_truth = truth.copy()
    bad_truth[5, 0, 0] = -np.inf
    dst.ens_band(src, bad_truth)
    assert dst.counter("ens_band_invalid_columns") == 2
    dst.ens_score(None)
    assert dst.counter("ens_invalid_points") == 6 * gr.num_grid_nodes
  finally:
    src.close()
    dst.close()


# ---- 3. state -----------------------------------------------------------------------------------------------------------------
def test_a_replaced_plan_keeps_the_allocations_flat_and_new_tables_drop_it():
  M = 2
  n_lat, n_lon, B, C, atabs, stabs, plan, members, truth = _case_13x24(M)
  gr = _graph(n_lat, n_lon)
  other = _plan(12, C, [1, 2, 4], {"a": (0, 1), "b": (2, 11), "c": dict(l=(5, 9), complement=True)}, 0, stabs)
  src, dst = _handle(gr, B, C), _handle(gr, B, 9)
  try:
    _push_all(src, members)
    dst.spec_set_tables(*atabs)
    dst.ens_reserve(M)
    dst.ens_band_set(**plan)
    dst.ens_band(src, truth)
    first = _download(dst, M)
    dst.ens_band_set(**other)
    dst.ens_band(src)
    flat = dst.counter("device_allocations"), src.counter("device_allocations")
    for r in range(6):
      dst.ens_band_set(**(plan if r % 2 else other))
      dst.ens_band(src)
      assert (dst.counter("device_allocations"), src.counter("device_allocations")) == flat
    assert dst.counter("ens_band_calls") == 8
    for x, y in zip(first, _download(dst, M)):                 # round 5 set `plan` again
      assert x.tobytes() == y.tobytes()
    # the plan survives gc_ens_reserve ...
    dst.ens_reserve(M)
    dst.ens_band(src)
    assert dst.ens_download_member(M - 1).tobytes() == first[M - 1].tobytes()
    # ... and goes with the tables it was made for
    dst.spec_set_tables(*atabs)
    with pytest.raises(_lib.GencastHipError, match="no plan"):
      dst.ens_band(src)
    assert dst._lib.gc_ens_band(dst._h, src._h, None) == _lib.GC_ERR_STATE
    dst.ens_band_set(**plan)
    dst.ens_band(src)
    assert dst.ens_download_member(0).tobytes() == first[0].tobytes()
  finally:
    src.close()
    dst.close()


# ---- 4. every documented error ------------------------------------------------------------------------------------------------
def test_every_documented_error():
  M, CD = 2, 9
  n_lat, n_lon, B, C, atabs, stabs, good, members, truth = _case_13x24(M)
  gr = _graph(n_lat, n_lon)
  L = 12
  dp, F, I = _lib.ctypes.POINTER(_lib.ctypes.c_double), _lib._f32p, _lib._i32p
  p = lambda x, ty: None if x is None else np.ascontiguousarray(x).ctypes.data_as(ty)
  INV, STATE, UNSUP = _lib.GC_ERR_INVALID_ARGUMENT, _lib.GC_ERR_STATE, _lib.GC_ERR_UNSUPPORTED
  resp, comp, ch, bd = good["response"], good["complement"], good["src_channel"], good["band"]

  def c_set(h, c_src=C, K=3, resp=resp, comp=comp, ch=ch, bd=bd, leg=stabs[0], cs=stabs[1], sn=stabs[2]):
    keep = [None if x is None else np.ascontiguousarray(x) for x in (resp, comp, ch, bd, leg, cs, sn)]
    return h._lib.gc_ens_band_set(h._h, c_src, K, p(keep[0], dp), p(keep[1], I), p(keep[2], I), p(keep[3], I), p(keep[4], F),
                                  p(keep[5], F), p(keep[6], F))

  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=CD + 4, c_out=CD, batch=B)
  src, dst, other_b, other_c = _handle(gr, B, C), _handle(gr, B, CD), _handle(gr, B + 1, C), _handle(gr, B, C + 1)
  small = _handle(_graph(11, 15), B, C)
  lib = dst._lib
  try:
    # ---- gc_ens_band_set
    assert c_set(bare) == STATE                                # before gc_set_graph
    assert c_set(dst) == STATE                                 # before gc_spec_set_tables
    assert lib.gc_ens_band(dst._h, src._h, None) == STATE
    with pytest.raises(_lib.GencastHipError, match="no analysis tables"):
      dst.ens_band_set(**good)
    dst.spec_set_tables(*atabs)
    for kw in (dict(resp=None), dict(comp=None), dict(ch=None), dict(bd=None), dict(leg=None), dict(cs=None), dict(sn=None)):
      assert c_set(dst, **kw) == INV, kw
    for K in (0, 9, -1):
      assert c_set(dst, K=K, resp=np.ones((9, L))) == UNSUP, K
    bad_resp = resp.copy()
    bad_resp[2, 11] = np.inf
    nan_resp = resp.copy()
    nan_resp[0, 0] = np.nan
    for kw in (dict(c_src=0), dict(c_src=5), dict(ch=np.where(np.arange(CD) == 4, -1, ch).astype(np.int32)),
               dict(ch=np.where(np.arange(CD) == 4, C, ch).astype(np.int32)), dict(bd=np.where(np.arange(CD) == 8, 3, bd).astype(np.int32)),
               dict(bd=np.where(np.arange(CD) == 0, -1, bd).astype(np.int32)), dict(resp=bad_resp), dict(resp=nan_resp)):
      assert c_set(dst, **kw) == INV, kw
    for bad in (dict(c_src=0), dict(response=resp[:, :11]), dict(response=np.ones((9, L))), dict(response=bad_resp), dict(complement=comp[:2]),
                dict(src_channel=ch[:8]), dict(band=bd[:8]), dict(src_channel=np.full(CD, C)), dict(band=np.full(CD, 3)),
                dict(legendre_synthesis=stabs[0][:, :12]), dict(cos_s=stabs[1][:11]), dict(sin_s=stabs[2][:, :23])):
      with pytest.raises(ValueError):
        dst.ens_band_set(**{**good, **bad})
    # ---- gc_ens_band
    with pytest.raises(_lib.GencastHipError, match="no plan"):
      dst.ens_band(src)
    assert lib.gc_ens_band(dst._h, src._h, None) == STATE      # no plan
    dst.ens_band_set(**good)
    assert lib.gc_ens_band(dst._h, dst._h, None) == INV and lib.gc_ens_band(dst._h, None, None) == INV
    for bad in (dst, None, "src"):
      with pytest.raises(ValueError, match="another NativeDenoiser"):
        dst.ens_band(bad)
    for h in (bare, other_b, other_c, small):                  # no graph; another batch; c_out != c_src; another G
      assert lib.gc_ens_band(dst._h, h._h, None) == INV
      with pytest.raises(ValueError, match="other dimensions"):
        dst.ens_band(h)
    with pytest.raises(_lib.GencastHipError, match="no member store"):      # on dst
      dst.ens_band(src, truth)
    dst.ens_reserve(M)
    with pytest.raises(_lib.GencastHipError, match="no member store on the source"):
      dst.ens_band(src, truth)
    src.ens_reserve(M + 1)
    with pytest.raises(_lib.GencastHipError, match="different numbers of members"):
      dst.ens_band(src, truth)
    src.ens_reserve(M)
    src.ens_push_host(0, members[0])
    with pytest.raises(_lib.GencastHipError, match="source member slot 1 has not been pushed"):
      dst.ens_band(src, truth)
    src.ens_push_host(1, members[1])
    with pytest.raises(_lib.GencastHipError, match="no truth on the source"):
      dst.ens_band(src)
    assert lib.gc_ens_band(dst._h, src._h, None) == STATE
    with pytest.raises(ValueError, match="truth must be"):
      dst.ens_band(src, truth[..., :CD - 4])
    assert dst.counter("ens_band_calls") == 0
    dst.ens_band(src, truth)
    dst.ens_band(src)                                          # the truth stays in the source
    assert dst.counter("ens_band_calls") == 2
    with pytest.raises(ValueError):
      dst.counter("ens_band_no_such_counter")
  finally:
    for h in (bare, src, dst, other_b, other_c, small):
      h.close()


# ---- 5. the sampler is left alone ----------------------------------------------------------------------------------------------
def test_a_band_call_leaves_the_sampler_state_alone():
  from oracle import gencast_oracle as O
  gr, dims, params, cond, _ = helpers.tiny_setup(batch=2, seed=2)
  rng = np.random.default_rng(8)
  G, C = gr.num_grid_nodes, dims.c_out
  assert G == 13 * 24
  noise = rng.standard_normal((G, 2, C)).astype(np.float32)
  truth = rng.standard_normal((G, 2, C)).astype(np.float32)
  atabs, stabs = _tables(13, 24, 12)
  plan = _plan(12, C, [0, C - 1], {"low": (0, 3), "high": dict(l=(0, 3), complement=True)}, 0, stabs)
  nd = helpers.make_native(gr, dims, params, 2)
  other = helpers.make_native(gr, dims, params, 2)
  view = _handle(gr, 2, 4)
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
    view.spec_set_tables(*atabs)
    view.ens_band_set(**plan)
    view.ens_reserve(2)
    view.ens_band(nd, truth)
    ref = _reference([first, second], 13, 24, plan, atabs, stabs)
    for i in range(2):
      R.check(view.ens_download_member(i), ref[i][0], ref[i][1], f"sampled member {i}")
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
