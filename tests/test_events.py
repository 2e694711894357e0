"""Ensemble event verification, host side: `quantize_node_weights`, `EventScores` on tables of the reference
(tests/event_reference.py), `event_probability`, `EventSpec` packing and `EnsembleRolloutResult.merge` with events.
The device side is tests/test_gpu_events.py.  Sizes: the 13 x 24 grid of the GPU tests (G = 312), B = 2, C = 6."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import EventScores, EventSpec, datasets, rollout, synthetic, verification
from gencast_flax_nnx_amd.verification import event_probability, quantize_node_weights
from tests import event_reference as R

G, B, C = 312, 2, 6
ALPHAS = np.array([0.05, 0.2, 0.5, 0.9])
_CACHE = {}


def _case(M):
  """(members, truth, w, thresholds, directions, wq, scale, reference tables): computed once per M and left unchanged."""
  if M not in _CACHE:
    members, truth, w, thr, d = R.data(M, G, B, C, seed=M)
    wq, scale = quantize_node_weights(w)
    _CACHE[M] = (members, truth, w, thr, d, wq, scale, R.tables(members, truth, thr, d, wq))
  return _CACHE[M]


def _scores(M):
  *_, d, _, scale, ref = _case(M)
  return EventScores(ref["weighted"], ref["counts"], M, d, scale, ref["invalid"])


# ---- quantize_node_weights ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [1.0, 1.9999, 2.0, 3e-7, 4.0e9, 2.0 ** 32 - 1, 2.0 ** 40])
def test_quantize_node_weights_scale_is_the_largest_power_of_two(top):
  w = np.array([0.0, 0.25 * top, top, 0.5 * top, 0.0])
  wq, scale = quantize_node_weights(w)
  assert wq.dtype == np.uint32 and wq.shape == w.shape
  m, _ = np.frexp(scale)
  assert m == 0.5                                           # a power of two
  assert int(wq.max()) <= 2 ** 32 - 1 and top * scale <= 2 ** 32 - 1 and top * (2.0 * scale) > 2 ** 32 - 1
  assert wq[0] == 0 and wq[-1] == 0
  np.testing.assert_array_equal(wq, np.rint(w * scale).astype(np.uint32))
  ref_wq, ref_scale = R.quantize(w)
  assert ref_scale == scale
  np.testing.assert_array_equal(ref_wq, wq)


def test_quantize_node_weights_of_latitude_weights_keeps_them_to_2_pow_minus_31():
  w = verification.node_weights(synthetic.make_example(lat=np.linspace(-90, 90, 13), lon=np.arange(24) * 15.0, batch=1, seed=0)[1])
  wq, scale = quantize_node_weights(w)
  assert np.abs(wq.astype(np.float64) / scale - w.astype(np.float64)).max() <= 0.5 / scale
  assert scale >= 2.0 ** 31 / float(w.max()) / 2.0


@pytest.mark.parametrize("bad", [[1.0, -0.5], [1.0, np.nan], [np.inf, 1.0], [0.0, 0.0], []])
def test_quantize_node_weights_rejects(bad):
  with pytest.raises(ValueError):
    quantize_node_weights(np.array(bad))


# ---- EventScores on reference tables ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3])
def test_the_reference_reaches_every_bin(M):
  assert R.every_bin_is_reached(_case(M)[-1]["weighted"])


@pytest.mark.parametrize("M", [2, 3, 8])
def test_brier_is_the_direct_weighted_mean_and_the_decomposition_closes(M):
  members, truth, _, thr, d, wq, scale, ref = _case(M)
  es = _scores(M)
  direct = R.brier_direct(members, truth, thr, d, wq.astype(np.float64) / scale)
  np.testing.assert_allclose(es.brier, direct, rtol=1e-12)
  np.testing.assert_allclose(es.brier, es.reliability - es.resolution + es.uncertainty, rtol=1e-12, atol=1e-15)
  assert np.all(es.brier_fair <= es.brier)
  np.testing.assert_array_equal(es.valid_points + 0, ref["counts"].sum(axis=(-1, -2)))
  np.testing.assert_array_equal(es.valid_points, np.full((4, B, C), G, np.uint64))
  np.testing.assert_allclose(es.valid_weight, (wq.astype(np.float64) / scale).sum(), rtol=0, atol=0)


@pytest.mark.parametrize("M", [2, 3, 8])
def test_every_derived_score_equals_the_reference_formula(M):
  *_, scale, ref = _case(M)
  es = _scores(M)
  want = R.scores(ref["weighted"], scale, M, ALPHAS)
  for name, value in want.items():
    got = es.economic_value(ALPHAS) if name == "economic_value" else getattr(es, name)
    np.testing.assert_allclose(got, value, rtol=1e-12, equal_nan=True, err_msg=name)
  p, freq, n = es.reliability_curve
  np.testing.assert_array_equal(p, np.arange(M + 1) / M)
  assert freq.shape == n.shape == (4, B, C, M + 1)
  np.testing.assert_array_equal(np.isnan(freq), n == 0)


@pytest.mark.parametrize("M", [2, 3, 8])
def test_roc_and_economic_value_properties(M):
  es = _scores(M)
  h, f = es.hit_rate, es.false_alarm_rate
  assert h.shape == f.shape == (4, B, C, M + 2)
  big_o = es.weighted[..., 1, :].sum(axis=-1)
  big_n = es.weighted.sum(axis=(-1, -2))
  degenerate = (big_o == 0) | (big_o == big_n)
  if M == 8:
    assert degenerate.any()                                 # the 2.3 sigma event is never observed in some column
  ok = ~np.isnan(h).any(axis=-1) & ~np.isnan(f).any(axis=-1)
  np.testing.assert_array_equal(ok, ~degenerate)
  for r in (h[ok], f[ok]):
    assert np.all(np.diff(r, axis=-1) <= 0) and np.all(r[..., 0] == 1.0) and np.all(r[..., -1] == 0.0)
  area = es.roc_area
  np.testing.assert_array_equal(np.isnan(area), degenerate)
  assert np.all((area[ok] >= 0.0) & (area[ok] <= 1.0))
  assert np.all(area[0] > 0.5)                              # at the median threshold: the members share the truth's signal
  value = es.economic_value(ALPHAS)
  assert value.shape == (4, B, C, 4)
  np.testing.assert_array_equal(np.isnan(value), np.broadcast_to(degenerate[..., None], value.shape))
  assert np.all((value[ok] >= 0.0) & (value[ok] <= 1.0))
  assert es.economic_value(0.3).shape == (4, B, C)
  for bad in (0.0, 1.0, [0.2, 1.5]):
    with pytest.raises(ValueError):
      es.economic_value(bad)


def test_roc_area_is_one_half_when_the_observed_frequency_does_not_depend_on_the_forecast():
  M = 5
  rng = np.random.default_rng(0)
  n = 4 * rng.integers(1, 1000, size=(2, 1, 3, M + 1)).astype(np.uint64)       # o_k / n_k = 1 / 4 in every bin
  weighted = np.stack([n - n // 4, n // 4], axis=-2)
  es = EventScores(weighted, weighted, M, [1, -1], 8.0)
  np.testing.assert_allclose(es.roc_area, 0.5, rtol=0, atol=1e-15)
  np.testing.assert_allclose(es.resolution, 0.0, rtol=0, atol=1e-30)
  np.testing.assert_allclose(es.base_rate, 0.25, rtol=0, atol=0)
  np.testing.assert_allclose(es.economic_value([0.1, 0.25, 0.6]), 0.0, rtol=0, atol=1e-15)


def test_all_zero_tables_give_nan_not_an_exception():
  es = EventScores(np.zeros((1, 1, 2, 2, 4), np.uint64), np.zeros((1, 1, 2, 2, 4), np.uint64), 3, [1], 1.0)
  for name in ("base_rate", "brier", "brier_fair", "reliability", "resolution", "uncertainty", "brier_skill", "roc_area"):
    assert np.isnan(getattr(es, name)).all(), name
  assert np.isnan(es.economic_value(0.5)).all() and (es.valid_points == 0).all()


@pytest.mark.parametrize("M", [3, 8])
def test_merge_of_two_halves_of_the_nodes_is_the_whole(M):
  members, truth, _, thr, d, wq, scale, ref = _case(M)
  cut = 151
  parts = [EventScores(r["weighted"], r["counts"], M, d, scale, r["invalid"])
           for r in (R.tables(members[:, :cut], truth[:cut], thr[:, :cut], d, wq[:cut]),
                     R.tables(members[:, cut:], truth[cut:], thr[:, cut:], d, wq[cut:]))]
  whole = EventScores.merge(parts)
  np.testing.assert_array_equal(whole.weighted, ref["weighted"])
  np.testing.assert_array_equal(whole.counts, ref["counts"])
  np.testing.assert_array_equal(whole.invalid, ref["invalid"])
  assert whole.weighted.dtype == np.uint64 and whole.scale == scale and whole.directions == tuple(d)
  np.testing.assert_array_equal(parts[0].weighted, R.tables(members[:, :cut], truth[:cut], thr[:, :cut], d, wq[:cut])["weighted"])


def test_merge_and_constructor_raise_on_mismatch():
  *_, d, _, scale, ref = _case(3)
  es = _scores(3)
  other_m = _scores(2)
  flipped = EventScores(ref["weighted"], ref["counts"], 3, -np.asarray(d), scale)
  rescaled = EventScores(ref["weighted"], ref["counts"], 3, d, 2.0 * scale)
  for other in (other_m, flipped, rescaled):
    with pytest.raises(ValueError, match="merge"):
      EventScores.merge([es, other])
  with pytest.raises(ValueError):
    EventScores.merge([])
  with pytest.raises(ValueError):
    EventScores(ref["weighted"], ref["counts"], 4, d, scale)
  with pytest.raises(ValueError):
    EventScores(ref["weighted"], ref["counts"][..., :-1], 3, d, scale)
  with pytest.raises(ValueError):
    EventScores(ref["weighted"], ref["counts"], 3, [1, 0, 1, 1], scale)
  with pytest.raises(ValueError):
    EventScores(ref["weighted"], ref["counts"], 3, d, 0.0)


# ---- event_probability -------------------------------------------------------------------------------------------------
def test_event_probability_round_trips_the_codes():
  M = 64
  k = np.array([0, 1, 63, 64, 0, 64, 17])
  o = np.array([0, 1, 0, 1, 1, 0, 1])
  code = np.concatenate([(k | (o << 7)).astype(np.uint8), np.array([255], np.uint8)]).reshape(2, 4)
  prob, obs = event_probability(code, M)
  assert prob.dtype == np.float32 and obs.dtype == np.bool_ and prob.shape == obs.shape == (2, 4)
  np.testing.assert_array_equal(prob.reshape(-1)[:-1], (k / M).astype(np.float32))
  np.testing.assert_array_equal(obs.reshape(-1)[:-1], o.astype(bool))
  assert np.isnan(prob[1, 3]) and not obs[1, 3]
  ref = _case(8)[-1]
  prob, obs = event_probability(ref["code"], 8)
  assert not np.isnan(prob).any() and set(np.unique(prob * 8)) <= set(range(9))
  assert int(obs[0].sum()) == int(ref["counts"][0, :, :, 1, :].sum())


# ---- EventSpec ------------------------------------------------------------------------------------------------------------
def _targets():
  return synthetic.make_example(lat=np.linspace(-90, 90, 5), lon=np.arange(8) * 45.0, batch=2, seed=1)[1]


def test_event_spec_packs_in_channel_order_with_nan_for_a_missing_variable():
  tgt = _targets()
  layout = {name: (off, n) for name, off, n in datasets.channel_layout(tgt)}
  clim = np.arange(2 * 5 * 8, dtype=np.float64).reshape(2, 5, 8)
  spec = EventSpec({"2m_temperature": np.array([1.5, -2.5]),
                    "temperature": np.arange(26.0).reshape(2, 13, 1, 1),
                    "10m_u_component_of_wind": clim}, [3, -1])
  assert spec.n_thresholds == 2 and spec.directions == (1, -1)
  packed = spec.packed(tgt)
  assert packed.shape == (2, 40, 2, 82) and packed.dtype == np.float32
  given = np.zeros(82, bool)
  off, n = layout["2m_temperature"]
  given[off:off + n] = True
  np.testing.assert_array_equal(packed[0][..., off], np.float32(1.5))
  np.testing.assert_array_equal(packed[1][..., off], np.float32(-2.5))
  off, n = layout["temperature"]
  given[off:off + n] = True
  assert n == 13
  for t in range(2):
    np.testing.assert_array_equal(packed[t][..., off:off + n], np.broadcast_to(np.arange(13.0) + 13 * t, (40, 2, 13)))
  off, n = layout["10m_u_component_of_wind"]
  given[off:off + n] = True
  for t in range(2):                                        # node = lat_i n_lon + lon_j, the same for every batch member
    np.testing.assert_array_equal(packed[t][:, :, off], np.broadcast_to(clim[t].reshape(40, 1), (40, 2)))
  assert np.isnan(packed[..., ~given]).all() and not np.isnan(packed[..., given]).any()
  fields = spec.fields(tgt)
  assert len(fields) == 2 and fields[0]["temperature"].dims == tgt["temperature"].dims
  assert fields[0]["temperature"].data.shape == tgt["temperature"].data.shape


def test_event_spec_mapped_sends_full_fields_through_the_map_of_the_targets():
  tgt = _targets()
  spec = EventSpec({"2m_temperature": np.array([1.0, 2.0, 3.0])}, [1, 1, -1])
  def fn(name, v):                                          # a shift per batch member, as a residual map is
    shift = np.arange(2, dtype=np.float32).reshape((2,) + (1,) * (v.data.ndim - 1))
    return datasets.Variable(v.dims, (v.data - shift) / np.float32(4.0))

  mapped = spec.mapped(tgt, fn)
  assert mapped.directions == spec.directions
  off = {name: o for name, o, _ in datasets.channel_layout(tgt)}["2m_temperature"]
  packed = mapped.packed(tgt)
  for t in range(3):
    for b in range(2):
      np.testing.assert_array_equal(packed[t][:, b, off], np.float32((t + 1.0 - b) / 4.0))
  assert np.isnan(np.delete(packed, off, axis=-1)).all()


def test_event_spec_rejects():
  tgt = _targets()
  with pytest.raises(ValueError):
    EventSpec({"2m_temperature": np.array([1.0, 2.0])}, [1, 0])
  with pytest.raises(ValueError):
    EventSpec({"2m_temperature": np.array([1.0, 2.0])}, [1])
  with pytest.raises(ValueError):
    EventSpec({}, [])
  with pytest.raises(ValueError, match="not a target variable"):
    EventSpec({"no_such_variable": np.array([1.0])}, [1]).packed(tgt)
  with pytest.raises(ValueError, match="more axes"):
    EventSpec({"2m_temperature": np.zeros((1, 13, 5, 8))}, [1]).packed(tgt)


# ---- EnsembleRolloutResult ------------------------------------------------------------------------------------------
def _result(seed, horizon=2, with_events=True, M=3):
  rng = np.random.default_rng(seed)
  scores = [verification.EnsembleScores(rng.uniform(1.0, 2.0, (B, C, 6)), rng.integers(0, 9, (B, C, M + 1)).astype(np.uint64), M)
            for _ in range(horizon)]
  events = None
  if with_events:
    events = [EventScores(rng.integers(0, 2 ** 40, (2, B, C, 2, M + 1)).astype(np.uint64),
                          rng.integers(0, 99, (2, B, C, 2, M + 1)).astype(np.uint64), M, [1, -1], 2.0 ** 30,
                          rng.integers(0, 5, 2).astype(np.uint64)) for _ in range(horizon)]
  return rollout.EnsembleRolloutResult(scores, n_members=M, scores_normalized=scores, events=events)


def test_rollout_result_merge_adds_the_event_tables_lead_time_by_lead_time():
  a, b = _result(1), _result(2)
  m = a.merge(b)
  assert len(m.events) == 2
  for k in range(2):
    np.testing.assert_array_equal(m.events[k].weighted, a.events[k].weighted + b.events[k].weighted)
    np.testing.assert_array_equal(m.events[k].counts, a.events[k].counts + b.events[k].counts)
    np.testing.assert_array_equal(m.events[k].invalid, a.events[k].invalid + b.events[k].invalid)
  plain = _result(3, with_events=False).merge(_result(4, with_events=False))
  assert plain.events is None and plain.horizon == 2
  with pytest.raises(ValueError, match="only one of the two results carries events"):
    a.merge(_result(5, with_events=False))
  with pytest.raises(ValueError, match="only one of the two results carries events"):
    _result(5, with_events=False).merge(a)
  with pytest.raises(ValueError, match="same lead times"):
    rollout.EnsembleRolloutResult(a.scores, n_members=3, events=a.events[:1])
