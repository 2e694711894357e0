"""Ensemble event verification on the device (gc_ens_event_*) against the definition restated in
tests/event_reference.py.  Everything the device returns is an integer, so every comparison is ==: there is no tolerance
in this file except rtol = 1e-12 on the float64 scores derived on the host from equal tables.

Sizes: the 13 x 24 grid (G = 312) with set_graph only; (B, C) = (2, 6): W = 12, two node-range blocks with a remainder;
(1, 82): the real channel count, one column tile at small M and several at M = 50 / 64 (the tables of a tile fit 40 KB);
(4, 82): W = 328, at least two column tiles at every M.  One 11 x 15 grid (G = 165) with (1, 7): a field length that is no
multiple of 4, the one-point-per-thread form of the code pass."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import (EnsembleSampler, EventScores, EventSpec, GenCast, _lib, config, datasets, rollout, synthetic,
                                  verification, weights)
from gencast_flax_nnx_amd.denoiser import dims_from_arch
from gencast_flax_nnx_amd.verification import event_probability, quantize_node_weights
from tests import event_reference as R
from tests import helpers
from tests.helpers import graph_handle as _handle, small_graph as _graph
from tests.test_gpu_host_api import _small_arch
from tests.test_rollout import _stats

pytestmark = pytest.mark.gpu

ALPHAS = np.array([0.05, 0.2, 0.5, 0.9])


def _push_all(nd, members):
  nd.ens_reserve(len(members))
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _check_tables(tag, got, ref, nd, G):
  weighted, counts, invalid = got
  T = len(ref["invalid"])
  assert weighted.dtype == counts.dtype == invalid.dtype == np.uint64
  np.testing.assert_array_equal(weighted, ref["weighted"], err_msg=f"{tag}: weighted")
  np.testing.assert_array_equal(counts, ref["counts"], err_msg=f"{tag}: counts")
  np.testing.assert_array_equal(invalid, ref["invalid"], err_msg=f"{tag}: invalid")
  for t in range(T):
    code = nd.ens_event_codes(t)
    assert code.dtype == np.uint8
    np.testing.assert_array_equal(code, ref["code"][t], err_msg=f"{tag}: code bytes of threshold {t}")
    skipped = (code == 255).sum(axis=0).astype(np.uint64)
    np.testing.assert_array_equal(counts[t].sum(axis=(-1, -2)) + skipped, np.full(skipped.shape, G, np.uint64))
  assert nd.counter("ens_event_invalid_points") == int(ref["invalid"].sum())


# ---- 1. equality with the definition ------------------------------------------------------------------------------------
CASES = [  # (M, T, B, C, reference must reach bins 0 and M in both rows)
    (2, 1, 2, 6, True), (3, 3, 2, 6, True), (8, 4, 4, 82, True), (50, 8, 1, 82, False), (64, 3, 1, 82, False),
    (50, 4, 4, 82, False), (64, 8, 2, 6, False), (2, 4, 1, 82, True), (3, 8, 4, 82, False)]


@pytest.mark.parametrize("M,T,B,C,full", CASES)
def test_tables_and_codes_equal_the_definition(M, T, B, C, full):
  gr = _graph()
  G = gr.num_grid_nodes
  assert G == 312
  members, truth, w, thr, d = R.data(M, G, B, C, seed=M, T=T)
  assert (d > 0).any() and ((d < 0).any() or T == 1)
  wq, scale = quantize_node_weights(w)
  ref = R.tables(members, truth, thr, d, wq)
  if full:
    assert R.every_bin_is_reached(ref["weighted"]), "the reference itself leaves a bin untouched"
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members)
    nd.ens_event_set(thr, d, wq)
    got = nd.ens_event_score(truth)
    assert got[0].shape == got[1].shape == (T, B, C, 2, M + 1) and got[2].shape == (T,)
    _check_tables(f"M={M} T={T} ({B}, {C})", got, ref, nd, G)
    assert nd.counter("ens_event_calls") == 1 and int(got[2].sum()) == 0
    print(f"M={M} T={T} ({B}, {C}): ens_event_device_us {nd.counter('ens_event_device_us')}")
    es = EventScores(*got[:2], M, d, scale, got[2])
    for name, want in R.scores(ref["weighted"], scale, M, ALPHAS).items():
      have = es.economic_value(ALPHAS) if name == "economic_value" else getattr(es, name)
      np.testing.assert_allclose(have, want, rtol=1e-12, equal_nan=True, err_msg=name)
    prob, obs = event_probability(nd.ens_event_codes(0), M)
    np.testing.assert_array_equal(prob, (R.in_event(members, thr[0], d[0]).sum(axis=0) / np.float32(M)).astype(np.float32))
    np.testing.assert_array_equal(obs, R.in_event(truth, thr[0], d[0]))
  finally:
    nd.close()


@pytest.mark.parametrize("M,T", [(3, 1), (8, 5)])
def test_a_field_length_that_is_no_multiple_of_four(M, T):
  gr = _graph(11, 15)
  G, B, C = gr.num_grid_nodes, 1, 7
  assert G == 165 and (G * B * C) % 4 != 0
  members, truth, w, thr, d = R.data(M, G, B, C, seed=7 + M, T=T)
  truth[G - 1, 0, C - 1] = np.nan                             # the very last point of the field
  wq, _ = quantize_node_weights(w)
  ref = R.tables(members, truth, thr, d, wq)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members)
    nd.ens_event_set(thr, d, wq)
    _check_tables(f"odd field M={M} T={T}", nd.ens_event_score(truth), ref, nd, G)
  finally:
    nd.close()


# ---- 2. ties and invalid points ---------------------------------------------------------------------------------------
def test_ties_and_invalid_points():
  gr = _graph()
  G, B, C, M, T = gr.num_grid_nodes, 2, 6, 8, 5
  members, truth, w, thr, d = R.data(M, G, B, C, seed=21, T=T)
  ties = np.array([0, 5, 77, 200, G - 1])
  # members and truth EXACTLY on the threshold: not an event, whichever the direction (thresholds 1: above, 2: below)
  for t in (1, 2):
    members[2, ties, 0, t] = thr[t, ties, 0, t]
    members[5, ties, 1, t] = thr[t, ties, 1, t]
    truth[ties, 0, t] = thr[t, ties, 0, t]
  nan_truth, inf_member, nan_thr = np.array([3, 4, 150, 300]), np.array([9, 120, 250]), np.array([11, 12, 13, 310])
  truth[nan_truth] = np.nan                                   # every (b, c) of those nodes, every threshold
  members[5, inf_member, 1, 2] = np.inf
  members[6, inf_member[0], 0, 4] = -np.inf
  thr[3, nan_thr, :, 5] = np.nan                              # threshold 3 only
  thr[0, 40, 1, 1] = np.inf
  thr[4] = np.nan                                             # a threshold field that is entirely NaN
  wq, scale = quantize_node_weights(w)
  ref = R.tables(members, truth, thr, d, wq)
  nd = _handle(gr, B, C)
  try:
    _push_all(nd, members)
    nd.ens_event_set(thr, d, wq)
    got = nd.ens_event_score(truth)
    _check_tables("ties", got, ref, nd, G)
    weighted, counts, invalid = got
    base = len(nan_truth) * B * C + len(inf_member) + 1
    assert invalid.tolist() == [base + 1, base, base, base + len(nan_thr) * B, G * B * C]
    assert not weighted[4].any() and not counts[4].any()
    assert (nd.ens_event_codes(4) == 255).all()
    code1, code2, code0 = (nd.ens_event_codes(t) for t in (1, 2, 0))
    assert ((code1[ties, 0, 1] >> 7) == 0).all()            # threshold 1 (above): the tied truth is not in the event either
    # at the tie points of threshold 2 (below): the truth is not in the event, and neither is the tied member 2
    assert ((code2[ties, 0, 2] >> 7) == 0).all()
    k_wo = sum(R.in_event(members[i, ties, 0, 2], thr[2, ties, 0, 2], -1).astype(int) for i in range(M) if i != 2)
    np.testing.assert_array_equal(code2[ties, 0, 2] & 127, k_wo)
    want255 = np.zeros((G, B, C), bool)
    want255[nan_truth] = True
    want255[inf_member, 1, 2] = True
    want255[inf_member[0], 0, 4] = True
    want255[40, 1, 1] = True
    np.testing.assert_array_equal(code0 == 255, want255)
    es = EventScores(weighted, counts, M, d, scale, invalid)
    assert np.isnan(es.brier[4]).all() and np.isfinite(es.brier[:4]).all()
  finally:
    nd.close()


# ---- 3. state ------------------------------------------------------------------------------------------------------------
def test_state_determinism_and_ownership():
  gr = _graph()
  G, B, C, M, T = gr.num_grid_nodes, 2, 6, 8, 3
  members, truth, w, thr, d = R.data(M, G, B, C, seed=31, T=T)
  wq, _ = quantize_node_weights(w)
  from gencast_flax_nnx_amd import spectra
  nd = _handle(gr, B, C)
  try:
    base = nd.counter("device_allocations")
    _push_all(nd, members)
    nd.ens_set_node_weight(w)
    spectra.ensure_tables(nd, _template(13, 24, B), None)
    score0 = nd.ens_score(truth)                              # uploads the truth
    spec0 = nd.ens_spectrum(None)
    nd.ens_event_set(thr, d, wq)
    a = nd.ens_event_score(None)                              # the truth of the earlier ens_score
    codes_a = [nd.ens_event_codes(t) for t in range(T)]
    ref = R.tables(members, truth, thr, d, wq)
    _check_tables("truth=None", a, ref, nd, G)
    b = nd.ens_event_score(truth)
    for x, y in zip(a + tuple(codes_a), b + tuple(nd.ens_event_codes(t) for t in range(T))):
      assert x.tobytes() == y.tobytes()
    # the other scores of the same store: the same bytes before and after
    score1, spec1 = nd.ens_score(None), nd.ens_spectrum(None)
    for x, y in zip(score0 + (spec0,), score1 + (spec1,)):
      assert x.tobytes() == y.tobytes()
    for i in range(M):
      np.testing.assert_array_equal(nd.ens_download_member(i), members[i])
    # another M without another ens_event_set: the thresholds survive the store
    held = nd.counter("device_allocations")
    _push_all(nd, members[:3])
    with pytest.raises(_lib.GencastHipError, match="no event codes"):
      nd.ens_event_codes(0)
    c = nd.ens_event_score(None)
    _check_tables("M = 3 after ens_reserve", c, R.tables(members[:3], truth, thr, d, wq), nd, G)
    assert nd.counter("device_allocations") == held
    # twenty rounds of set / score, alternating T: replaced, not grown
    nd.ens_event_set(thr[:2], d[:2], wq)
    nd.ens_event_score(None)
    flat = nd.counter("device_allocations")
    assert flat == held
    for r in range(20):
      t_now = 2 if r % 2 else 3
      nd.ens_event_set(thr[:t_now], d[:t_now], wq)
      got = nd.ens_event_score(None)
      assert got[0].shape[0] == t_now
      assert nd.counter("device_allocations") == flat
    np.testing.assert_array_equal(got[0], R.tables(members[:3], truth, thr[:2], d[:2], wq)["weighted"])
    assert nd.counter("ens_event_calls") == 24 and flat > base
  finally:
    nd.close()


def _template(n_lat, n_lon, batch):
  return synthetic.make_example(lat=np.linspace(-90, 90, n_lat), lon=np.arange(n_lon) * (360.0 / n_lon), batch=batch, seed=0)[1]


def test_every_documented_error():
  gr = _graph()
  G, B, C, M, T = gr.num_grid_nodes, 2, 6, 2, 2
  members, truth, w, thr, d = R.data(M, G, B, C, seed=41, T=T)
  wq, _ = quantize_node_weights(w)
  u64, u32, u8 = (_lib.ctypes.POINTER(t) for t in (_lib.ctypes.c_uint64, _lib.ctypes.c_uint32, _lib.ctypes.c_uint8))
  p = lambda a, ty: a.ctypes.data_as(ty)
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  try:                                                        # before gc_set_graph
    rc = bare._lib.gc_ens_event_set(bare._h, T, p(thr, _lib._f32p), p(d, _lib._i32p), p(wq, u32))
    assert rc == _lib.GC_ERR_STATE
  finally:
    bare.close()
  nd = _handle(gr, B, C)
  lib, h = nd._lib, nd._h
  table = np.zeros((8, B, C, 2, M + 1), np.uint64)
  code = np.zeros((G, B, C), np.uint8)
  try:
    # gc_ens_event_score / download without thresholds
    with pytest.raises(_lib.GencastHipError, match="no thresholds"):
      nd.ens_event_score(truth)
    assert lib.gc_ens_event_score(h, p(truth, _lib._f32p), p(table, u64), None, None) == _lib.GC_ERR_STATE
    assert lib.gc_ens_event_download(h, 0, p(code, u8)) == _lib.GC_ERR_STATE
    with pytest.raises(_lib.GencastHipError, match="no thresholds"):
      nd.ens_event_codes(0)
    # gc_ens_event_set: T outside 1..8, a zero direction, null pointers, shapes
    eight = np.ascontiguousarray(np.broadcast_to(thr[:1], (9,) + thr.shape[1:]))
    assert lib.gc_ens_event_set(h, 0, p(thr, _lib._f32p), p(d, _lib._i32p), p(wq, u32)) == _lib.GC_ERR_UNSUPPORTED
    assert lib.gc_ens_event_set(h, 9, p(eight, _lib._f32p), p(np.ones(9, np.int32), _lib._i32p), p(wq, u32)) == _lib.GC_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="1..8"):
      nd.ens_event_set(eight, np.ones(9, np.int32), wq)
    with pytest.raises(ValueError, match="zero"):
      nd.ens_event_set(thr, np.array([1, 0], np.int32), wq)
    for args in ((None, p(d, _lib._i32p), p(wq, u32)), (p(thr, _lib._f32p), None, p(wq, u32)), (p(thr, _lib._f32p), p(d, _lib._i32p), None)):
      assert lib.gc_ens_event_set(h, T, *args) == _lib.GC_ERR_INVALID_ARGUMENT
    for bad in ((thr[:, :-1], d, wq), (thr[0], d, wq), (thr, d[:1], wq), (thr, d, wq[:-1]), (thr, d, w), (thr, d, -wq.astype(np.int64))):
      with pytest.raises(ValueError):
        nd.ens_event_set(*bad)
    assert nd.counter("device_allocations") == nd.counter("device_allocations")
    nd.ens_event_set(thr, d, wq)
    # no member store; a slot not pushed; no truth
    with pytest.raises(_lib.GencastHipError, match="no member store"):
      nd.ens_event_score(truth)
    assert lib.gc_ens_event_score(h, p(truth, _lib._f32p), p(table, u64), None, None) == _lib.GC_ERR_STATE
    nd.ens_reserve(M)
    nd.ens_push_host(0, members[0])
    with pytest.raises(_lib.GencastHipError, match="slot 1 has not been pushed"):
      nd.ens_event_score(truth)
    nd.ens_push_host(1, members[1])
    with pytest.raises(_lib.GencastHipError, match="no truth"):
      nd.ens_event_score(None)
    with pytest.raises(ValueError, match="truth must be"):
      nd.ens_event_score(truth[:-1])
    assert lib.gc_ens_event_score(h, p(truth, _lib._f32p), None, None, None) == _lib.GC_ERR_INVALID_ARGUMENT
    # download: nothing scored yet; t outside [0, T); null; after a new set; after a new reserve
    with pytest.raises(_lib.GencastHipError, match="no event codes"):
      nd.ens_event_codes(0)
    assert nd.counter("ens_event_calls") == 0
    weighted, counts, invalid = nd.ens_event_score(truth)       # counts and invalid may be NULL in C
    only = np.zeros_like(weighted)
    assert lib.gc_ens_event_score(h, None, p(only, u64), None, None) == _lib.GC_OK
    np.testing.assert_array_equal(only, weighted)
    nd.ens_event_codes(T - 1)
    for t in (-1, T):
      with pytest.raises(ValueError, match="threshold outside"):
        nd.ens_event_codes(t)
    assert lib.gc_ens_event_download(h, 0, None) == _lib.GC_ERR_INVALID_ARGUMENT
    nd.ens_event_set(thr, d, wq)
    assert lib.gc_ens_event_download(h, 0, p(code, u8)) == _lib.GC_ERR_STATE
    nd.ens_event_score(None)
    nd.ens_event_codes(0)
    nd.ens_reserve(M)
    assert lib.gc_ens_event_download(h, 0, p(code, u8)) == _lib.GC_ERR_STATE
    with pytest.raises(ValueError):
      nd.counter("ens_event_no_such_counter")
  finally:
    nd.close()


# ---- 4. through the stack --------------------------------------------------------------------------------------------------
HORIZON, SB, SC = 2, 2, 82


class _Setup:
  """The small model of tests/test_gpu_ensemble_rollout.py: the 9 x 16 grid (G = 144), batch 2, latent 128, 2 layers, 4 noise
  levels; targets and forcings of HORIZON random frames."""

  def __init__(self):
    arch = _small_arch()
    self.lat, self.lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
    self.inp, tgt1, frc1 = synthetic.make_example(lat=self.lat, lon=self.lon, batch=SB, seed=4)
    self.tgt1, self.frc1 = tgt1, frc1
    rng = np.random.default_rng(5)

    def stretch(ds, nt):
      out = {}
      for k, v in ds.items():
        shape = list(v.data.shape)
        shape[v.dims.index("time")] = nt
        out[k] = datasets.Variable(v.dims, rng.standard_normal(shape).astype(np.float32))
      return datasets.Dataset(out, ds.coords)

    self.targets, self.forcings = stretch(tgt1, HORIZON), stretch(frc1, HORIZON)
    sc = config.SamplerConfig(num_noise_levels=4, stochastic_churn_rate=0.0)
    params = weights.random_params(dims_from_arch(arch, 262, SC), seed=3)
    self.gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=1)
    self.wrapper = rollout.InputsAndResiduals(self.gc, *_stats(config.TASK))
    self.G = len(self.lat) * len(self.lon)
    self.template0 = rollout.isel_time(self.targets, slice(0, 1)).map(np.zeros_like)
    clim = rng.standard_normal((3, 9, 16)) * 0.5                       # a map per event for one surface variable
    self.spec = EventSpec({"2m_temperature": clim,
                           "temperature": np.array([0.0, 0.7, -0.7]).reshape(3, 1, 1, 1) * np.linspace(0.5, 1.5, 13).reshape(1, 13, 1, 1),
                           "10m_u_component_of_wind": np.array([0.0, 1.0, -1.0]),
                           "geopotential": np.array([-0.3, 0.3, 0.0])}, [1, 1, -1])

  def norm(self, which):
    return self.wrapper if which == "wrapper" else None

  def stats_per_channel(self, which):
    norm = self.norm(which)
    layout = datasets.channel_layout(self.template0)
    if norm is None:
      return np.ones(SC), np.zeros(SC)
    s = np.concatenate([rollout._per_channel_stat(norm._scales, n, self.template0[n], 1.0) for n, _, _ in layout])
    l = np.concatenate([rollout._per_channel_stat(norm._locations, n, self.template0[n], 0.0) for n, _, _ in layout])
    return s, l

  def normalised(self, field, which):
    """A packed field in physical units in the members' units: (x - l) / s in float64, rounded once."""
    if self.norm(which) is None:
      return field.astype(np.float32)
    s, l = self.stats_per_channel(which)
    return ((field.astype(np.float64) - l) / s).astype(np.float32)

  def truth(self, k, which):
    tk = rollout.isel_time(self.targets, slice(k, k + 1))
    y = np.transpose(datasets.dataset_to_stacked(tk, tk.sizes), (1, 2, 0, 3)).reshape(self.G, SB, SC)
    return self.normalised(y, which)


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  for lane in getattr(s.gc.denoiser, "_lanes", None) or []:
    lane.close()
  s.gc.denoiser.native.close()


def _stack(ds):
  a = np.transpose(datasets.dataset_to_stacked(ds, ds.sizes), (1, 2, 0, 3))
  return np.ascontiguousarray(a.reshape((-1,) + a.shape[2:]), dtype=np.float32)


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_rollout_events_equal_the_definition_on_the_kept_members(setup, which):
  M = 3
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which), base_seed=3, concurrent_members=2)
  res = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, keep_members=True, events=setup.spec)
  plain = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, keep_members=True)
  assert plain.events is None and len(res.events) == HORIZON
  wq, scale = quantize_node_weights(verification.node_weights(setup.template0))
  thr = setup.normalised(setup.spec.packed(setup.template0), which)
  given = ~np.isnan(thr[0, 0, 0])
  assert 0 < given.sum() < SC                                  # some channels carry thresholds, the others are NaN
  for k in range(HORIZON):
    ref = R.tables(np.stack(res.members[k]), setup.truth(k, which), thr, setup.spec.directions, wq)
    ev = res.events[k]
    np.testing.assert_array_equal(ev.weighted, ref["weighted"], err_msg=f"{which} lead {k}")
    np.testing.assert_array_equal(ev.counts, ref["counts"], err_msg=f"{which} lead {k}")
    np.testing.assert_array_equal(ev.invalid, ref["invalid"], err_msg=f"{which} lead {k}")
    assert ev.n_members == M and ev.scale == scale and ev.directions == (1, 1, -1)
    assert int(ev.invalid[0]) == setup.G * SB * int((~given).sum())
    assert (ref["counts"].sum(axis=(1, 2)) > 0).sum() > 3 * 2                   # not everything in one bin
    np.testing.assert_array_equal(ev.valid_points[:, :, given], np.full((3, SB, int(given.sum())), setup.G, np.uint64))
    # the other results of the same run: the bytes of a run without events
    assert res.scores[k].sums.tobytes() == plain.scores[k].sums.tobytes()
    assert res.scores[k].rank_histogram.tobytes() == plain.scores[k].rank_histogram.tobytes()
    for m in range(M):
      np.testing.assert_array_equal(res.members[k][m], plain.members[k][m])
  per_var = res.events[0].per_variable(setup.template0)
  assert per_var["brier"]["temperature"].shape == (3, SB, 13) and np.isnan(per_var["brier"]["specific_humidity"]).all()
  merged = res.merge(res)
  np.testing.assert_array_equal(merged.events[1].weighted, 2 * res.events[1].weighted)
  with pytest.raises(ValueError, match="carries events"):
    res.merge(plain)
  # one spec per lead time: the second lead with other thresholds
  other = EventSpec({"2m_temperature": np.array([0.2, 0.4, 0.1])}, [1, 1, -1])
  per_lead = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, keep_members=True, events=[setup.spec, other])
  np.testing.assert_array_equal(per_lead.events[0].weighted, res.events[0].weighted)
  thr1 = setup.normalised(other.packed(setup.template0), which)
  ref1 = R.tables(np.stack(per_lead.members[1]), setup.truth(1, which), thr1, other.directions, wq)
  np.testing.assert_array_equal(per_lead.events[1].weighted, ref1["weighted"])
  with pytest.raises(ValueError, match="equal directions"):
    er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, events=[setup.spec, EventSpec({"2m_temperature": np.zeros(3)}, [1, 1, 1])])
  with pytest.raises(ValueError, match="equal directions"):
    er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, events=[setup.spec] * 3)


def test_single_step_events_equal_the_definition_on_the_members_the_sampler_returns(setup):
  M = 3
  gc, inp, tgt, frc = setup.gc, setup.inp, setup.tgt1, setup.frc1
  ens = EnsembleSampler(gc._sampler, base_seed=5, concurrent_members=2)
  fields = [_stack(d) for _, d in sorted(ens(inp, tgt.map(np.zeros_like), frc, M), key=lambda t: t[0])]
  wq, scale = quantize_node_weights(verification.node_weights(tgt))
  ref = R.tables(np.stack(fields), _stack(tgt), setup.spec.packed(tgt), setup.spec.directions, wq)
  ev = gc.ensemble_events(inp, tgt, frc, num_members=M, spec=setup.spec, rngs=5, concurrent_members=2)
  np.testing.assert_array_equal(ev.weighted, ref["weighted"])
  np.testing.assert_array_equal(ev.counts, ref["counts"])
  np.testing.assert_array_equal(ev.invalid, ref["invalid"])
  assert ev.scale == scale and ev.n_members == M and (ref["counts"].sum(axis=(1, 2)) > 0).sum() > 3 * 2
  ev2 = ens.events(inp, tgt, frc, M, setup.spec)
  assert ev2.weighted.tobytes() == ev.weighted.tobytes()
  with pytest.raises(ValueError, match="ens_push_host"):
    EnsembleSampler(gc._sampler, rank=0, world_size=2).events(inp, tgt, frc, M, setup.spec)
  # under the wrappers: the thresholds take the map of the targets, so a threshold that IS the target field ties with it
  from gencast_flax_nnx_amd import NaNCleaner
  tied = EventSpec({"2m_temperature": np.stack([tgt["2m_temperature"].data, tgt["2m_temperature"].data + 100.0])}, [1, -1])
  fill = datasets.Dataset({"2m_temperature": datasets.Variable((), np.float32(0.0))})
  stack = NaNCleaner(setup.wrapper, var_to_clean="2m_temperature", fill_value=fill, reintroduce_nans=True)
  wrapped = stack.ensemble_events(inp, tgt, frc, num_members=M, spec=tied, rngs=5)
  off = {n: o for n, o, _ in datasets.channel_layout(tgt)}["2m_temperature"]
  assert not wrapped.weighted[0, :, off, 1].any()             # the truth equals threshold 0 everywhere: never an event
  assert not wrapped.weighted[1, :, off, 0].any()             # and lies below threshold 1 everywhere: always one
  np.testing.assert_array_equal(wrapped.valid_points[:, :, off], np.full((2, SB), setup.G, np.uint64))
  assert int(wrapped.invalid[0]) == setup.G * SB * (SC - 1)


def test_an_event_call_leaves_the_sampler_state_alone():
  from oracle import gencast_oracle as O
  gr, dims, params, cond, _ = helpers.tiny_setup(batch=2, seed=2)
  rng = np.random.default_rng(8)
  G = gr.num_grid_nodes
  noise = rng.standard_normal((G, 2, dims.c_out)).astype(np.float32)
  truth = rng.standard_normal((G, 2, dims.c_out)).astype(np.float32)
  thr = np.zeros((2, G, 2, dims.c_out), np.float32)
  thr[1] = 0.5
  d = np.array([1, -1], np.int32)
  wq, _ = quantize_node_weights(np.linspace(0.5, 1.5, G))
  nd = helpers.make_native(gr, dims, params, 2)
  other = helpers.make_native(gr, dims, params, 2)
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
    nd.ens_event_set(thr, d, wq)
    got = nd.ens_event_score(truth)
    ref = R.tables(np.stack([first, second]), truth, thr, d, wq)
    _check_tables("pushed samples", got, ref, nd, G)
    np.testing.assert_array_equal(nd.download_sample(), first)      # the last sample is still there
    np.testing.assert_array_equal(nd.download_stash(), first)
    np.testing.assert_array_equal(other.download_sample(), second)
    np.testing.assert_array_equal(nd.download_cond(), cond)
    np.testing.assert_array_equal(nd.download_noise(), noise)
    nd.sample_resident(sched)                                      # a replay of the captured graph: the same bytes
    np.testing.assert_array_equal(nd.download_sample(), first)
    assert nd.counter("graph_captures") == captures and nd.counter("graph_replays") == replays + 1
  finally:
    nd.close()
    other.close()
