"""Every unit with its fresh device allocations poisoned (GC_DEBUG_POISON=1, DESIGN.md "Poisoned allocations").

The library clears a buffer in a handful of places; everything else is right only if each call writes every word it later
reads.  A fresh process usually gets zeroed device memory, so a read of a word nobody wrote sees 0.0, 0 or "no count" and
the result still equals its definition -- the other device tests cannot see such a read.  With the switch on, `dev_alloc`
fills every new buffer before anything else touches it: NaN bytes (0xFF) in floating-point buffers, 0x01 bytes in integer
ones (a stray count reads 16 843 009, a stray event code k = 1, o = 0), 0xFF in the pinned staging buffers.

Every case runs the same calls on a poisoned and on an unpoisoned handle in this process and asserts
  * `poison_allocs` > 0 on the first and == 0 on the second (the switch was picked up, and only where it was set);
  * the rule the unit's own device test holds it to against its reference, imported from that test or from
    tests/*_reference.py -- byte equality where the unit promises it, its derived bound elsewhere -- on BOTH runs;
  * the same bytes in every output array of the two runs.

Shapes of the ensemble units, 13 x 24 grid (G = 312), graph-only handles: (B, C, M) = (2, 6, 3) (padded size 4: one padded
register), (2, 6, 33) (padded size 64) and (1, 257, 3) (a second column tile of one column).  Plans have T = 2 thresholds,
Q = 2 quantiles, K = 2 groups and S = 2 scales where they exist.  One truth value and one member value are NaN, so the
skipped-point counters and the flagged-column paths run.  Units that fill a store from another handle (derive, band,
feature, window) take the shape on the SOURCE handle; their destination has the channels the plan makes.  The entries
that need a model (gc_ens_push_state, the context store, the forward and what hangs on it) run on `helpers.tiny_setup`,
whose c_out is 6: they take the two member counts and no 257-column shape.

fp16 node features: the existing test holds the raw output to max 2e-2 / rms 2e-3 against the oracle IN THE SAME MODE
(tests/test_gpu_parity.py, F16_TOL_MAX / F16_TOL_RMS), not to the float32 TOL; so does the case here."""
import functools
import time

import numpy as np
import pytest

from gencast_flax_nnx_amd import BandSpec, DerivedSpec, SphericalAnalysis, losses
from gencast_flax_nnx_amd import noise as noise_mod
from gencast_flax_nnx_amd.verification import efi_table, quantize_node_weights, quantize_row_weights
from oracle import gencast_oracle as O
from tests import band_reference as BR
from tests import clim_reference as CR
from tests import derive_expr_reference as XR
from tests import derive_reference as DR
from tests import efi_reference as FR
from tests import event_reference as ER
from tests import feature_reference as TR
from tests import fss_reference as SR
from tests import helpers
from tests import map_reference as PR
from tests import multivar_reference as MR
from tests import order_reference as OR
from tests import region_reference as RR
from tests import sampler_cases as SC
from tests import spectrum_reference as SPR
from tests import tail_reference as LR
from tests import test_gpu_edge_terms as ET
from tests import test_gpu_loss as TL
from tests import test_gpu_mid_grid as MID
from tests import verification_reference as VR
from tests import window_reference as WR
from tests.test_gpu_clim import _check as _check_clim
from tests.test_gpu_order import _check as _check_order
from tests.test_gpu_parity import F16_TOL_MAX, F16_TOL_RMS, TOL, _oracle
from tests.test_gpu_spectra import _check as _check_spec
from tests.test_gpu_verification import _check_fields as _check_ens_fields
from tests.test_gpu_verification import _check_sums as _check_ens_sums

pytestmark = pytest.mark.gpu

N_LAT, N_LON = 13, 24
G = N_LAT * N_LON
SHAPES = [(2, 6, 3), (2, 6, 33), (1, 257, 3)]               # (B, C, M)
SHAPE_IDS = [f"B{b}-C{c}-M{m}" for b, c, m in SHAPES]
NAN_NODE_MEMBER, NAN_NODE_TRUTH = 7, G - 2                  # slot 1, (0, min(3, C - 1)) / (B - 1, C - 1)
shapes = pytest.mark.parametrize("B,C,M", SHAPES, ids=SHAPE_IDS)


@functools.lru_cache(maxsize=None)
def _graph(n_lat=N_LAT, n_lon=N_LON):
  return helpers.small_graph(n_lat, n_lon)


def _latlon():
  return np.linspace(-90, 90, N_LAT), np.arange(N_LON) * (360.0 / N_LON)


def _plant(members, truth):
  members[1, NAN_NODE_MEMBER, 0, min(3, members.shape[-1] - 1)] = np.nan
  truth[NAN_NODE_TRUTH, -1, -1] = np.nan


@functools.lru_cache(maxsize=None)
def _data(B, C, M, seed=0):
  """(members [M, G, B, C], truth [G, B, C], w [G]) float32, shared and read-only: channels over eight decades, a tie
  between two members and one with the truth, one NaN member value and one NaN truth value."""
  rng = np.random.default_rng(1000 * M + C + seed)
  scale = np.logspace(-3, 5, C).astype(np.float32)
  members = rng.standard_normal((M, G, B, C), dtype=np.float32) * scale
  truth = rng.standard_normal((G, B, C), dtype=np.float32) * scale
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  members[1, 40:44] = members[0, 40:44]
  truth[50:54] = members[0, 50:54]
  _plant(members, truth)
  for a in (members, truth, w):
    a.setflags(write=False)
  return members, truth, w


def _columns(C):
  """The channels a reference that is filled point by point runs on: all six, or the edges of both column tiles of 257 and
  the columns with the planted NaNs."""
  return np.arange(C) if C <= 6 else np.array([0, 3, 127, 128, 255, 256])


def _push_all(nd, members, w=None):
  nd.ens_reserve(len(members))
  if w is not None:
    nd.ens_set_node_weight(w)
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


class _Tracked:
  """The handles of one run: every one is closed, and says whether its allocations were poisoned."""

  def __init__(self):
    self.made = []

  def __call__(self, nd):
    self.made.append(nd)
    return nd

  def graph(self, B, C, gr=None):
    return self(helpers.graph_handle(gr if gr is not None else _graph(), B, C))

  def native(self, gr, dims, params, batch, **kw):
    return self(helpers.make_native(gr, dims, params, batch, **kw))


def _same_bytes(tag, name, a, b):
  a, b = np.atleast_1d(np.ascontiguousarray(a)), np.atleast_1d(np.ascontiguousarray(b))
  assert a.shape == b.shape and a.dtype == b.dtype, f"{tag} {name}: {a.shape} {a.dtype} poisoned, {b.shape} {b.dtype} not"
  if a.tobytes() != b.tobytes():
    words = a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,))
    bad = np.argwhere(words.any(axis=-1))
    raise AssertionError(f"{tag} {name}: {len(bad)} of {a.size} values differ between the poisoned and the unpoisoned handle, "
                         f"first at {bad[:5].tolist()}: {a[tuple(bad[0])]!r} against {b[tuple(bad[0])]!r}")


def _both(monkeypatch, tag, case):
  """`case(new)` -> {name: array}: the calls of a unit on handles made through `new` (a _Tracked), with the unit's own
  rule asserted inside.  Run poisoned, then unpoisoned; the counters, then the bytes."""
  outs = []
  t0 = time.perf_counter()
  for poisoned in (True, False):
    if poisoned:
      monkeypatch.setenv("GC_DEBUG_POISON", "1")
    else:
      monkeypatch.delenv("GC_DEBUG_POISON")
    new = _Tracked()
    try:
      out = case(new)
      assert new.made, tag
      for nd in new.made:
        n, nbytes = nd.counter("poison_allocs"), nd.counter("poison_bytes")
        assert (n > 0 and nbytes > 0) if poisoned else (n == 0 and nbytes == 0), f"{tag}: poison_allocs {n}, poison_bytes {nbytes}, poisoned {poisoned}"
        if poisoned:
          assert n >= nd.counter("device_allocations")      # every buffer the handle holds was filled (and those it has replaced)
    finally:
      for nd in new.made:
        nd.close()
    outs.append({k: np.array(v) for k, v in out.items()})
  assert outs[0].keys() == outs[1].keys() and outs[0], tag
  for name in outs[0]:
    _same_bytes(tag, name, outs[0][name], outs[1][name])
  print(f"{tag}: {time.perf_counter() - t0:.2f} s wall, {len(outs[0])} arrays equal byte for byte")
  return outs[0]


def _within(tag, got, ref, tol):
  MID._within(tag, got, ref, tol)


# ---- the ensemble units ------------------------------------------------------------------------------------------------------
@shapes
def test_ens_score_with_fields(B, C, M, monkeypatch):
  members, truth, w = _data(B, C, M)
  ref = VR.reference(members, truth, w)
  tag = f"ens_score B={B} C={C} M={M}"

  def case(new):
    nd = new.graph(B, C)
    _push_all(nd, members, w)
    sums, hist = nd.ens_score(truth, want_fields=True)
    mean, var = nd.ens_download_fields()
    _check_ens_sums(tag, sums, hist, ref, G, M)
    _check_ens_fields(tag, mean, var, ref)
    assert nd.counter("ens_invalid_points") == 2
    again, hist2 = nd.ens_score(None)
    return dict(sums=sums, hist=hist, mean=mean, var=var, again=again, hist2=hist2)

  out = _both(monkeypatch, tag, case)
  assert out["again"].tobytes() == out["sums"].tobytes() and out["hist2"].tobytes() == out["hist"].tobytes()


PROBS = (0.1, 0.9)                                          # Q = 2


@shapes
def test_ens_order_score_fields_and_quantiles(B, C, M, monkeypatch):
  members, truth, w = _data(B, C, M)
  ref = OR.reference(members, truth, w, PROBS)
  tag = f"order B={B} C={C} M={M}"

  def case(new):
    nd = new.graph(B, C)
    _push_all(nd, members, w)
    nd.ens_order_set(PROBS)
    nd.ens_order_fields()                                   # the field pass alone, before any score
    alone = [nd.ens_order_quantile(q) for q in range(len(PROBS))]
    for q in range(len(PROBS)):
      np.testing.assert_array_equal(alone[q], ref["fields"][q], err_msg=f"{tag}: quantile field {q} of the field pass")
    out = nd.ens_order_score(truth)
    _check_order(tag, out, ref, G)
    assert out[4] == 2 == nd.counter("ens_order_invalid_points")
    fields = [nd.ens_order_quantile(q) for q in range(len(PROBS))]
    for q in range(len(PROBS)):
      np.testing.assert_array_equal(fields[q], ref["fields"][q], err_msg=f"{tag}: quantile field {q}")
    return dict(bins=out[0], extra=out[1], pinball=out[2], counts=out[3], invalid=np.array(out[4]), fields=np.stack(fields),
                alone=np.stack(alone))

  _both(monkeypatch, tag, case)


@shapes
def test_ens_clim_score(B, C, M, monkeypatch):
  K = 5
  members, truth, w = _data(B, C, M)
  clim = _data(B, C, K, seed=77)[0]
  ref = CR.reference(members, clim, truth, w)
  tag = f"clim B={B} C={C} M={M}"

  def case(new):
    nd, cl = new.graph(B, C), new.graph(B, C)
    _push_all(nd, members, w)
    _push_all(cl, clim)
    out = nd.ens_clim_score(cl, truth)
    _check_clim(tag, out, ref, G)
    assert nd.counter("ens_clim_invalid_points") == out[2] == ref["invalid"]
    return dict(sums=out[0], counts=out[1], invalid=np.array(out[2]))

  _both(monkeypatch, tag, case)


@shapes
def test_ens_efi_score_and_fields(B, C, M, monkeypatch):
  K, ranks, dirs, E = 3, (2, 1), (+1, -1), 20                # T = 2 events
  members, truth, w = _data(B, C, M)
  clim = _data(B, C, K, seed=33)[0]
  wq, _ = quantize_node_weights(w)
  cs = _columns(C)
  ref = FR.reference(members[..., cs], clim[..., cs], truth[..., cs], w, ranks, dirs, E, wq)
  alone_ref = FR.fields_only(members[..., cs], clim[..., cs])
  keep = MID._keep(members, truth) & np.isfinite(clim).all(0)
  bits = MID._bits
  tag = f"efi B={B} C={C} M={M}"

  def case(new):
    nd, cl = new.graph(B, C), new.graph(B, C)
    _push_all(nd, members, w)
    _push_all(cl, clim)
    nd.ens_efi_set(ranks, dirs, E, wq)
    nd.ens_efi_fields(cl, efi_table(K))                     # the index pass alone, before any score
    alone = nd.ens_efi_field(0)
    assert bits(alone[..., cs]).tobytes() == bits(alone_ref).tobytes(), f"{tag}: EFI field of the index pass"
    sums, weighted, counts, invalid = nd.ens_efi_score(cl, efi_table(K), truth)
    assert invalid == int((~keep).sum()) == nd.counter("ens_efi_invalid_points")
    efi, obs = nd.ens_efi_field(0), nd.ens_efi_field(1)
    assert int(np.isnan(efi).sum()) == invalid and int(np.isnan(obs).sum()) == invalid
    assert bits(efi[..., cs]).tobytes() == bits(ref["efi"]).tobytes(), f"{tag}: EFI field"
    assert bits(obs[..., cs]).tobytes() == bits(ref["observed"]).tobytes(), f"{tag}: observed index"
    np.testing.assert_array_equal(weighted[:, :, cs], ref["weighted"], err_msg="weighted")
    np.testing.assert_array_equal(counts[:, :, cs], ref["counts"], err_msg="counts")
    for t in range(2):                                      # every column: each valid point in one bin
      np.testing.assert_array_equal(counts[t].sum(axis=(-1, -2)), keep.sum(0).astype(np.uint64))
    _within(tag, sums[:, cs], ref["sums"], FR.tolerance(ref, G))
    return dict(sums=sums, weighted=weighted, counts=counts, invalid=np.array(invalid), efi=efi, obs=obs, alone=alone)

  _both(monkeypatch, tag, case)


def _event_case(B, C, M, seed=9, T=2):
  members, truth, w, thr, d = ER.data(M, G, B, C, seed=seed + M + C, T=T + 1)
  thr, d = np.ascontiguousarray(thr[1:]), d[1:].copy()       # +1.3 above, -1.3 below
  _plant(members, truth)
  thr[T - 1, 11, 0, 0] = np.nan                             # a NaN threshold: not counted for that t alone
  wq, _ = quantize_node_weights(w)
  return members, truth, w, thr, d, wq


@shapes
def test_ens_events(B, C, M, monkeypatch):
  members, truth, w, thr, d, wq = _event_case(B, C, M)
  ref = ER.tables(members, truth, thr, d, wq)
  tag = f"events B={B} C={C} M={M}"

  def case(new):
    nd = new.graph(B, C)
    _push_all(nd, members)
    nd.ens_event_set(thr, d, wq)
    weighted, counts, invalid = nd.ens_event_score(truth)
    np.testing.assert_array_equal(weighted, ref["weighted"], err_msg="weighted")
    np.testing.assert_array_equal(counts, ref["counts"], err_msg="counts")
    np.testing.assert_array_equal(invalid, ref["invalid"], err_msg="invalid")
    assert [int(v) for v in invalid] == [2, 3] and nd.counter("ens_event_invalid_points") == 5
    codes = np.stack([nd.ens_event_codes(t) for t in range(2)])
    np.testing.assert_array_equal(codes, ref["code"], err_msg="code bytes")
    return dict(weighted=weighted, counts=counts, invalid=invalid, codes=codes)

  _both(monkeypatch, tag, case)


@shapes
def test_ens_fss_sums_and_fields(B, C, M, monkeypatch):
  W = B * C
  members, truth, w, thr, d, wq = _event_case(B, C, M, seed=19)
  lat, lon = _latlon()
  r_lats = np.array([0, 2], np.int32)                        # S = 2
  r_lons = np.stack([np.zeros(N_LAT, np.int32), DerivedSpec.window(lat, lon, 2500.0)[1]]).astype(np.int32)
  row_wq = quantize_row_weights(losses.normalized_latitude_weights(lat))
  code_ref = ER.tables(members, truth, thr, d, wq)["code"]
  cols = np.arange(W) if W <= 12 else np.array([0, 3, 127, 128, 255, 256])
  ref = SR.separable(code_ref.reshape(2, G, W)[:, :, cols], M, N_LAT, N_LON, r_lats, r_lons, row_wq, wq)
  tag = f"fss B={B} C={C} M={M}"

  def case(new):
    nd = new.graph(B, C)
    _push_all(nd, members)
    nd.ens_event_set(thr, d, wq)
    nd.ens_fss_set(r_lats, r_lons, row_wq)
    nd.ens_event_score(truth)
    sums = nd.ens_fss_score()
    assert sums.shape == (2, 2, B, C, 4) and np.isfinite(sums).all()
    _within(tag, sums.reshape(2, 2, W, 4)[:, :, cols], ref["sums"], SR.bound(ref["sums"], G))
    out = dict(sums=sums)
    for t, s in ((0, 0), (1, 1)):                            # fields: ==, NaN pattern included
      prob, obs = nd.ens_fss_fields(t, s)
      np.testing.assert_array_equal(prob.reshape(G, W)[:, cols], ref["prob"][t, s], err_msg=f"prob t={t} s={s}")
      np.testing.assert_array_equal(obs.reshape(G, W)[:, cols], ref["obs"][t, s], err_msg=f"obs t={t} s={s}")
      assert (np.isnan(prob) == (code_ref[t] == 255)).all() and (np.isnan(obs) == (code_ref[t] == 255)).all()
      out[f"prob{t}{s}"], out[f"obs{t}{s}"] = prob, obs
    return out

  _both(monkeypatch, tag, case)


@shapes
def test_ens_energy_and_variogram(B, C, M, monkeypatch):
  members, truth, w = _data(B, C, M)
  group = (np.arange(C) % 2).astype(np.int32)                # K = 2
  if C > 6:
    group[5] = -1                                            # a channel in no group
  scale = 2.0 ** np.random.default_rng(5).integers(-3, 4, C)
  offsets = [(0, 1), (-3, N_LON - 1)]
  ref = MR.energy(members, truth, w, group, scale)
  vref = MR.variogram(members, truth, w, N_LAT, N_LON, offsets, 0.5)
  tag = f"multivar B={B} C={C} M={M}"

  def case(new):
    nd = new.graph(B, C)
    _push_all(nd, members, w)
    nd.ens_energy_set(2, group, scale)
    d2, s0, invalid = nd.ens_energy_score(truth)
    assert invalid == ref["invalid"] == nd.counter("ens_energy_invalid_points") == 2
    _within(f"{tag} D2", d2, ref["d2"], MR.energy_tolerance(ref))
    _within(f"{tag} S0", s0, ref["s0"], (ref["n"][None, :] + 8.0) * 2.0 ** -53 * ref["s0"])
    nd.ens_variogram_set(N_LAT, N_LON, offsets, 0.5)
    sums, counts = nd.ens_variogram_score(None)
    np.testing.assert_array_equal(counts, vref["counts"], err_msg="counts")
    _within(f"{tag} variogram", sums, vref["sums"], MR.variogram_tolerance(vref, G, M))
    return dict(d2=d2, s0=s0, invalid=np.array(invalid), vsums=sums, vcounts=counts)

  _both(monkeypatch, tag, case)


def _tail_thresholds(B, C, M):
  members = _data(B, C, M)[0]
  rng = np.random.default_rng(7)
  scale = np.logspace(-3, 5, C).astype(np.float32)
  thr = (rng.standard_normal((2, G, B, C), dtype=np.float32) * np.float32(0.5) + np.float32([[[[0.6]]], [[[-0.6]]]])) * scale
  thr[0, 100] = members[0, 100]                             # a threshold bit-equal to a member
  thr[1, 12, 0, 0] = np.nan                                 # a NaN threshold: not counted for that t alone
  return thr, (+1, -1)


@shapes
def test_ens_tail(B, C, M, monkeypatch):
  members, truth, w = _data(B, C, M)
  thr, dirs = _tail_thresholds(B, C, M)
  ref = LR.reference(members, truth, w, thr, dirs)
  tag = f"tail B={B} C={C} M={M}"

  def case(new):
    nd = new.graph(B, C)
    _push_all(nd, members, w)
    nd.ens_tail_set(thr, dirs)
    sums, counts, invalid = nd.ens_tail_score(truth)
    np.testing.assert_array_equal(counts, ref["counts"], err_msg="counts")
    np.testing.assert_array_equal(invalid, ref["invalid"], err_msg="invalid")
    assert [int(v) for v in invalid] == [2, 3]
    _within(tag, sums, ref["sums"], LR.sum_tolerance(ref, G, M))
    return dict(sums=sums, counts=counts, invalid=invalid)

  _both(monkeypatch, tag, case)


def _region_bits():
  """R = 3: rows 0-5, rows 4-12 but row 6, the last node alone; row 6 is in no region."""
  row = np.arange(G) // N_LON
  bits = np.zeros(G, np.uint32)
  bits[row < 6] |= 1
  bits[(row >= 4) & (row != 6)] |= 2
  bits[G - 1] |= 4
  return bits, 3


@shapes
def test_ens_region(B, C, M, monkeypatch):
  members, truth, w = _data(B, C, M)
  bits, R = _region_bits()
  ref = RR.reference(members, truth, w, bits, R)
  tag = f"region B={B} C={C} M={M}"

  def case(new):
    nd = new.graph(B, C)
    _push_all(nd, members, w)
    nd.ens_region_set(bits, R)
    sums, hist, invalid = nd.ens_region_score(truth)
    np.testing.assert_array_equal(hist, ref["hist"], err_msg="hist")
    np.testing.assert_array_equal(invalid, ref["invalid"], err_msg="invalid")
    assert [int(v) for v in invalid] == [1, 1, 0] and nd.counter("ens_region_invalid_points") == 2
    _within(tag, sums, ref["sums"], RR.sum_tolerance(ref, G, M))
    return dict(sums=sums, hist=hist, invalid=invalid)

  _both(monkeypatch, tag, case)


@shapes
def test_ens_map_accumulate_and_events_over_two_dates(B, C, M, monkeypatch):
  T = 2
  dates, thr, d, wq = [], None, None, None
  for k in range(2):
    members, truth, w, thr_k, d_k, wq_k = _event_case(B, C, M, seed=90 + k)
    if k == 0:
      thr, d, wq = thr_k, d_k, wq_k
    dates.append((members, truth))
  codes = [ER.tables(m, t, thr, d, wq)["code"] for m, t in dates]
  events_ref = np.zeros((T, 5, G, B, C), np.uint32)
  for code in codes:
    PR.accumulate_events(events_ref, code)
  ref_sums, ref_counts, ref_invalid = PR.reference(dates)
  tag = f"map B={B} C={C} M={M}"

  def case(new):
    nd = new.graph(B, C)
    nd.ens_event_set(thr, d, wq)
    nd.ens_map_set(None, 2, T)
    invalid = []
    for k, (members, truth) in enumerate(dates):
      if k == 0:
        nd.ens_reserve(M)
      for i, x in enumerate(members):
        nd.ens_push_host(i, x)
      nd.ens_event_score(truth)
      nd.ens_map_accumulate_events(1)
      nd.ens_map_accumulate(1)
      invalid.append(nd.counter("ens_map_invalid_points"))
    sums, counts, events, n = nd.ens_map_download(1)
    assert invalid == ref_invalid == [2, 2] and n.tolist() == [2, 2]
    assert events.dtype == np.uint32 and np.array_equal(events, events_ref)
    assert counts.tobytes() == np.ascontiguousarray(ref_counts).tobytes(), f"{tag}: counts"
    assert sums.tobytes() == np.ascontiguousarray(ref_sums).tobytes(), f"{tag}: sums"
    empty = nd.ens_map_download(0)                          # the slot nothing went into: zero, not what the allocation held
    assert not empty[0].any() and not empty[1].any() and not empty[2].any() and empty[3].tolist() == [0, 0]
    return dict(sums=sums, counts=counts, events=events, empty_sums=empty[0], empty_counts=empty[1], empty_events=empty[2])

  _both(monkeypatch, tag, case)


@shapes
def test_ens_window_emit(B, C, M, monkeypatch):
  Lw, n = 3, 4                                              # the ring wraps
  rng = np.random.default_rng(41 + M + C)
  f = (rng.standard_normal((n, M + 1, G, B, C)) * np.logspace(-2, 3, C)).astype(np.float32)
  f[n - 1, 1, 7, 0, min(3, C - 1)] = np.nan
  f[1, M, G - 2, B - 1, C - 1] = np.nan                     # the truth of a push still in the window
  f[0, :, 9, 0, 0] = np.inf                                 # (pushed out of the window by the fourth push)
  tag = f"window B={B} C={C} M={M}"

  def case(new):
    out = {}
    for kind in ("mean", "max"):
      code, coef = WR.coefficients(kind, Lw)
      want = WR.window(WR.last(list(f), Lw), code, coef)
      src, win = new.graph(B, C), new.graph(B, C)
      src.ens_reserve(M)
      win.ens_reserve(M)
      win.ens_window_set(code, Lw, coef)
      for i in range(n):
        for m in range(M):
          src.ens_push_host(m, f[i, m])
        win.ens_window_push(src, f[i, M])
      win.ens_window_emit()
      got = np.stack([win.ens_download_member(m) for m in range(M)])
      assert WR.same_bits(got, want[:M]), f"{tag} {kind}: {int((MID._bits(got) != MID._bits(want[:M])).sum())} of {got.size} words differ"
      assert not np.isinf(got).any() and win.counter("ens_window_emits") == 1 and win.counter("ens_window_pushes") == n
      out[kind] = got
    return out

  _both(monkeypatch, tag, case)


def _derive_fields(B, C, M, seed):
  """[M + 1, G, B, C]: M members, then the truth; a NaN member value, a NaN truth value, a NaN latitude row, an infinity."""
  members, truth = DR.data(M, G, B, C, seed)
  f = np.concatenate([members, truth[None]])
  f[1, NAN_NODE_MEMBER, 0, min(3, C - 1)] = np.nan
  f[M, NAN_NODE_TRUTH, B - 1, C - 1] = np.nan
  f[:, 6 * N_LON:7 * N_LON, 0, 2] = np.nan
  f[2, 200, B - 1, 0] = np.inf
  return f


def _derived(dst, src, fields):
  M = len(fields) - 1
  _push_all(src, fields[:M])
  dst.ens_derive(src, fields[M])
  return np.stack([dst.ens_download_member(i) for i in range(M)])


@shapes
def test_ens_derive(B, C, M, monkeypatch):
  """The point pass with as many derived channels as the source has (copy and norm2 alternating: the bits, one float32 ulp),
  then both pooling plans on six copied channels (their intermediate is the unit's integer-typed work buffer): MAX ==, MEAN
  within `derive_reference.mean_bound`."""
  f = _derive_fields(B, C, M, seed=12)
  idx = np.arange(C)
  pats = np.array([[3.7, -12.5, 0.9, 4.0], [1, 0, 1, 0], [1e-3, 250.0, 41.0, -3e4]])
  plan = dict(c_src=C, op=((idx + 1) % 2).astype(np.int32), src_a=((5 * idx + 3) % C).astype(np.int32),
              src_b=((7 * idx + 1) % C).astype(np.int32), affine=pats[idx % 3], pool=0, n_lat=N_LAT, n_lon=N_LON)
  ref = DR.apply(f[:M], plan)
  lat, lon = _latlon()
  r_lon = DerivedSpec.window(lat, lon, 2500.0)[1]
  rw = np.asarray(losses.normalized_latitude_weights(lat), np.float64)
  pooled = {}
  for pool in (DR.MAX, DR.MEAN):
    p = dict(c_src=C, op=np.zeros(6, np.int32), src_a=np.arange(6, dtype=np.int32), src_b=np.zeros(6, np.int32),
             affine=np.tile([1.0, 0.0, 1.0, 0.0], (6, 1)), pool=pool, n_lat=N_LAT, n_lon=N_LON, r_lat=2, r_lon=r_lon, row_weight=rw)
    pooled[pool] = (p, DR.apply(f[..., :6], dict(p, c_src=6), separable=True))
  tag = f"derive B={B} C={C} M={M}"

  def case(new):
    src, dst = new.graph(B, C), new.graph(B, C)
    dst.ens_derive_set(**plan)
    dst.ens_reserve(M)
    got = _derived(dst, src, f)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref))
    for j in np.flatnonzero(plan["op"] == 0):
      np.testing.assert_array_equal(MID._bits(got[..., j]), MID._bits(f[:M][..., plan["src_a"][j]]))
    ok = np.isfinite(ref)
    err = np.abs(got[ok].astype(np.float64) - ref[ok].astype(np.float64))
    assert np.all(err <= np.spacing(np.abs(ref[ok]))), f"{tag}: NORM2 beyond one float32 ulp"
    out = dict(point=got)
    pl = new.graph(B, 6)
    pl.ens_reserve(M)
    for pool, (p, want) in pooled.items():
      pl.ens_derive_set(**p)
      g = _derived(pl, src, f)
      np.testing.assert_array_equal(np.isnan(g), ~np.isfinite(f[:M][..., :6]))
      if pool == DR.MAX:
        np.testing.assert_array_equal(g, want[:M])
      else:
        bound = DR.mean_bound(f[:M][..., :6], want[:M], N_LON)
        fin = np.isfinite(want[:M])
        assert np.all(np.abs(g.astype(np.float64) - want[:M])[fin] <= bound[fin]), f"{tag}: pooled mean outside mean_bound"
      out[f"pool{pool}"] = g
    return out

  _both(monkeypatch, tag, case)


@shapes
def test_ens_derive_expr(B, C, M, monkeypatch):
  """copy, norm2, a sum of 37 terms, a norm of two lists, vorticity and divergence (both poles: the pole pass runs too),
  within the bound tests/derive_expr_reference.py computes from the inputs."""
  lat, lon = _latlon()
  rng = np.random.default_rng(12)
  scale, loc = rng.uniform(0.5, 2.0, C), rng.uniform(-1.0, 1.0, C)
  long_list = [(float(rng.uniform(-2.0, 2.0)), (5 * t + 2) % C, (3 * t + 1) % C if t % 2 else -1) for t in range(37)]
  wt = [float(v) for v in rng.uniform(0.1, 3.0, 5)]
  qu = [(wt[k], (2 + k) % C, (7 + k) % C) for k in range(5)]
  qv = [(wt[k], (2 + k) % C, (1 + 2 * k) % C) for k in range(5)]
  u, v = C - 2, C - 1
  channels = [("copy", C - 1), ("norm2", 0, 1, (3.7, -12.5, 0.9, 4.0)), ("sum", long_list), ("norm", qu, qv),
              ("vorticity", u, v), ("divergence", u, v)]
  plan = XR.raw_plan(C, channels, N_LAT, N_LON, scale=scale, loc=loc, lat=lat, lon=lon)
  assert plan["pole_row"].sum() == 2
  members, truth = DR.data(M, G, B, C, 21)
  f = np.concatenate([members, truth[None]])
  f[1, NAN_NODE_MEMBER, 0, min(3, C - 1)] = np.nan
  f[M, NAN_NODE_TRUTH, B - 1, C - 1] = np.nan
  f[0, 6 * N_LON:7 * N_LON, 0, u] = np.nan                  # u: one whole latitude row
  f[1, 1 * N_LON + 5, B - 1, v] = np.nan                    # v: next to the first pole
  ref, bound = XR.derive(f, plan)
  tag = f"derive-expr B={B} C={C} M={M}"

  def case(new):
    src, dst = new.graph(B, C), new.graph(B, 6)
    dst.ens_derive_set(**plan)
    dst.ens_reserve(M)
    got = _derived(dst, src, f)
    for j in range(1, 6):
      XR.within(got[..., j], ref[:M][..., j], bound[:M][..., j])
    np.testing.assert_array_equal(MID._bits(got[..., 0]), MID._bits(f[:M][..., C - 1]))
    rot = _derived(dst, src, np.roll(f, -1, axis=0))        # the former truth lies in the last slot now
    for j in range(1, 6):
      XR.within(rot[M - 1][..., j], ref[M][..., j], bound[M][..., j])
    return dict(got=got, rot=rot)

  _both(monkeypatch, tag, case)


@shapes
def test_ens_band(B, C, M, monkeypatch):
  """Three bands read by three source channels (c_d = 9): `band_reference.check`, the derived bound of tests/test_gpu_band.py.
  One member value is NaN: its source column is flagged and the band columns made from it are NaN on both sides."""
  lat, lon = _latlon()
  sa = SphericalAnalysis(lat, lon)
  L = sa.lmax
  atabs, stabs = sa.device_tables(), sa.synthesis_tables()
  response, complement = BandSpec({"low": (0, 2), "mid": (3, L - 1), "high": dict(l=(0, 2), complement=True)}, taper=1).responses(L)
  plan = dict(c_src=C, response=response, complement=complement, src_channel=np.tile(np.array([0, 3, 5], np.int32), 3),
              band=np.repeat(np.arange(3, dtype=np.int32), 3), legendre_synthesis=stabs[0], cos_s=stabs[1], sin_s=stabs[2])
  rng = np.random.default_rng(17 + M + C)
  scale = np.logspace(-3, 5, C)
  members = ((rng.standard_normal((M, G, B, C)) + 0.5) * scale).astype(np.float32)
  truth = ((rng.standard_normal((G, B, C)) + 0.5) * scale).astype(np.float32)
  clean = [BR.band_fields(x, N_LAT, N_LON, response, complement, plan["src_channel"], plan["band"], atabs, stabs)
           for x in (members[0], members[M - 1], truth)]
  members[1, NAN_NODE_MEMBER, 0, 3] = np.nan
  from_bad = plan["src_channel"] == 3                       # derived columns (0, j) read the flagged source column (0, 3)
  tag = f"band B={B} C={C} M={M}"

  def case(new):
    src, dst = new.graph(B, C), new.graph(B, 9)
    _push_all(src, members)
    dst.spec_set_tables(*atabs)
    dst.ens_band_set(**plan)
    dst.ens_reserve(M)
    dst.ens_band(src, truth)
    assert dst.counter("ens_band_invalid_columns") == 1
    got = np.stack([dst.ens_download_member(i) for i in range(M)])
    BR.check(got[0], clean[0][0], clean[0][1], f"{tag} member 0")
    BR.check(got[M - 1], clean[1][0], clean[1][1], f"{tag} member {M - 1}")
    bad = np.zeros((G, B, 9), bool)
    bad[:, 0, from_bad] = True
    np.testing.assert_array_equal(np.isnan(got[1]), bad, err_msg=f"{tag}: NaN columns of the member with a NaN")
    src.ens_push_host(0, truth)                             # the band truth has no download of its own: read back as a member
    dst.ens_band(src)
    back = dst.ens_download_member(0)
    BR.check(back, clean[2][0], clean[2][1], f"{tag} truth")
    return dict(got=got, truth=back)

  _both(monkeypatch, tag, case)


@shapes
def test_ens_feature(B, C, M, monkeypatch):
  """Two detectors (a minimum with threshold, ring and strike window; a maximum without a ring) on the last two source
  channels.  Everything is a comparison: integer equality of counts and nodes, the bits of the values, == on the strike
  fields."""
  rng = np.random.default_rng(77 + M + C)
  x = rng.standard_normal((N_LAT, N_LON, M + 1, B, C))
  for _ in range(2):
    x = (x + np.roll(x, 1, 0) + np.roll(x, -1, 0) + np.roll(x, 1, 1) + np.roll(x, -1, 1)) / 5.0
  f = np.moveaxis((np.round(x * 24.0) / 4.0).astype(np.float32).reshape(G, M + 1, B, C), 0, 1).copy()
  f[rng.integers(0, M + 1, 10), rng.integers(0, G, 10), 0, C - 1] = np.nan
  f[1, NAN_NODE_MEMBER, 0, C - 1] = np.nan
  f[M, NAN_NODE_TRUTH, B - 1, C - 1] = np.nan
  f[:, 0 * N_LON + 5, :, C - 1] = np.float32(-50.0)         # a centre in a pole row
  f[:, 6 * N_LON + 0, :, C - 1] = np.float32(-40.0)         # a centre at j = 0
  f[:, (N_LAT - 3) * N_LON + N_LON - 1, :, C - 1] = np.float32(-45.0)   # a centre at j = n_lon - 1
  dets = [dict(channel=C - 1, direction=-1, threshold=0.25, r_lat=1, r_lon=np.full(N_LAT, 2), ring_lat=2, ring_lon=np.full(N_LAT, 3),
               depth=0.5, strike_lat=1, strike_lon=np.full(N_LAT, 2)),
          dict(channel=C - 2, direction=+1, r_lat=2, r_lon=np.full(N_LAT, 3), strike_lat=0, strike_lon=np.full(N_LAT, 1))]
  plan = TR.plan_of(C, N_LAT, N_LON, dets, max_centres=64)
  r_count, r_node, r_value, r_strike = TR.apply(f, plan)
  assert r_count.min() >= 1 and r_count.max() <= 64
  tag = f"feature B={B} C={C} M={M}"

  def case(new):
    src, dst = new.graph(B, C), new.graph(B, 2)
    dst.ens_reserve(M)
    dst.ens_feature_set(**plan)
    _push_all(src, f[:M])
    dst.ens_feature(src, f[M])
    count, node, value = dst.ens_feature_centres()
    got = np.stack([dst.ens_download_member(i) for i in range(M)])
    np.testing.assert_array_equal(count, r_count)
    np.testing.assert_array_equal(node, r_node)
    np.testing.assert_array_equal(MID._bits(value), MID._bits(r_value))
    np.testing.assert_array_equal(got, r_strike[:M])
    return dict(count=count, node=node, value=value, strike=got)

  _both(monkeypatch, tag, case)


@shapes
def test_ens_spectrum_and_spec_field(B, C, M, monkeypatch):
  """The sums and the member power of the store and the power of one field, inside the bound of tests/test_gpu_spectra.py;
  the two columns with a NaN are NaN on both sides (`spec_invalid_columns`).  At 257 columns the reference runs on the
  edges of both column tiles and on the flagged columns."""
  N = B * C
  members, truth, _ = _data(B, C, M)
  tabs = SphericalAnalysis(*_latlon()).device_tables()
  cols = None if N <= 12 else [0, 3, 127, 128, 255, 256]
  ref = SPR.ensemble(members, truth, N_LAT, N_LON, tabs, cols=cols)
  field_ref, field_tol = SPR.field_spectrum(truth, N_LAT, N_LON, tabs, cols=cols)    # (flags the truth's own NaN column alone)
  pick = (lambda a: a) if cols is None else (lambda a: a[np.asarray(cols)])
  tag = f"spectrum B={B} C={C} M={M}"

  def case(new):
    nd = new.graph(B, C)
    nd.spec_set_tables(*tabs)
    _push_all(nd, members)
    sums, mp = nd.ens_spectrum(truth, want_member_power=True)
    L = sums.shape[2]
    assert nd.counter("spec_invalid_columns") == 2
    _check_spec(tag, pick(sums.reshape(N, L, 6)), ref["sums"], ref["tol"], SPR.SUM_NAMES)
    _check_spec(tag + " member power", np.stack([pick(p.reshape(N, L)) for p in mp]), ref["member_power"], ref["member_tol"])
    p0 = nd.spec_field(truth)
    _check_spec(tag + " spec_field(truth)", pick(p0.reshape(N, L)), field_ref, field_tol)
    assert nd.counter("spec_invalid_columns") == 1
    return dict(sums=sums, member_power=mp, field=p0)

  _both(monkeypatch, tag, case)


@pytest.mark.parametrize("M", [3, 33])
def test_ens_push_state_and_the_context_store(M, monkeypatch):
  """gc_ens_push_state is a gather and the context store copies: the member is bit for bit the conditioning channels (or,
  where state_src < 0, the sample's) it was gathered from, a saved context comes back bit for bit."""
  B = 2
  gr, dims, params, x, _ = helpers.tiny_setup(batch=B)
  noise = np.random.default_rng(5).standard_normal((gr.num_grid_nodes, B, dims.c_out)).astype(np.float32)
  sig = np.asarray(O.noise_schedule(80.0, 0.03, 3, 7.0), np.float32)
  state_src = np.array([0, 3, -1, 7, -1, 13], np.int32)
  x = x.copy()
  x[[0, 5, G - 1], 0, 3] = np.float32(-0.0)                 # a value whose bits a float comparison would not tell apart
  x2 = np.random.default_rng(8).standard_normal(x.shape).astype(np.float32)
  tag = f"push_state M={M}"

  def case(new):
    nd = new.native(gr, dims, params, B)
    nd.set_noisy_slots(np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32))
    nd.upload_cond(x)
    nd.upload_noise(noise)
    nd.sample_resident(sig, skip_dead_call=True, want_stats=False)
    sample = nd.download_sample()
    nd.ens_reserve(M)
    nd.ens_push_state(M - 1, state_src)
    nd.ens_push(0)
    got = nd.ens_download_member(M - 1)
    want = np.where(state_src >= 0, x[..., np.maximum(state_src, 0)], sample)
    np.testing.assert_array_equal(MID._bits(got), MID._bits(want))
    np.testing.assert_array_equal(MID._bits(nd.ens_download_member(0)), MID._bits(sample))
    nd.ctx_reserve(2)
    nd.ctx_save(1)
    nd.upload_cond(x2)
    nd.ctx_save(0)
    saved = np.stack([nd.ctx_download(0), nd.ctx_download(1)])
    nd.ctx_load(1)
    back = nd.download_cond()
    keep = np.ones(dims.c_in, bool)
    keep[dims.c_in - dims.c_out:] = False                   # the sampler rewrites the noisy-target slots
    np.testing.assert_array_equal(MID._bits(saved[0][..., keep]), MID._bits(x2[..., keep]))
    np.testing.assert_array_equal(MID._bits(saved[1][..., keep]), MID._bits(x[..., keep]))
    np.testing.assert_array_equal(MID._bits(back[..., keep]), MID._bits(saved[1][..., keep]))
    return dict(sample=sample, member=got, saved=saved[..., keep], back=back[..., keep])

  _both(monkeypatch, tag, case)


# ---- buffers made again for another M ----------------------------------------------------------------------------------------
def test_buffers_made_again_for_another_member_count(monkeypatch):
  """Order, tail, events and energy at M = 8 and then at M = 50 on ONE handle: the second round goes through `sized_for`,
  which drops the work buffers of M = 8 and makes new ones -- poisoned too.  Against the references of M = 50."""
  B, C = 2, 6
  m8 = _data(B, C, 8)
  members, truth, w = _data(B, C, 50)
  thr, dirs = _tail_thresholds(B, C, 50)
  _, _, _, ethr, d, _ = _event_case(B, C, 50)
  wq, _ = quantize_node_weights(w)
  group = (np.arange(C) % 2).astype(np.int32)
  scale = 2.0 ** np.random.default_rng(5).integers(-3, 4, C)
  ord_ref = OR.reference(members, truth, w, PROBS)
  tail_ref = LR.reference(members, truth, w, thr, dirs)
  evt_ref = ER.tables(members, truth, ethr, d, wq)
  en_ref = MR.energy(members, truth, w, group, scale)
  tag = "re-made M=8 -> M=50"

  def case(new):
    nd = new.graph(B, C)
    nd.ens_order_set(PROBS)
    nd.ens_tail_set(thr, dirs)
    nd.ens_event_set(ethr, d, wq)
    nd.ens_energy_set(2, group, scale)
    out = {}
    for mem, tr in ((m8[0], m8[1]), (members, truth)):
      _push_all(nd, mem, w)
      held = nd.counter("device_allocations")
      filled = nd.counter("poison_allocs")
      o = nd.ens_order_score(tr)
      t = nd.ens_tail_score(None)
      e = nd.ens_event_score(None)
      en = nd.ens_energy_score(None)
      if len(mem) == 50:
        assert nd.counter("device_allocations") == held     # replaced, not added ...
        if filled:
          assert nd.counter("poison_allocs") > filled       # ... and what replaced them was filled
    _check_order(tag, o, ord_ref, G)
    np.testing.assert_array_equal(t[1], tail_ref["counts"])
    np.testing.assert_array_equal(t[2], tail_ref["invalid"])
    _within(f"{tag} tail", t[0], tail_ref["sums"], LR.sum_tolerance(tail_ref, G, 50))
    np.testing.assert_array_equal(e[0], evt_ref["weighted"])
    np.testing.assert_array_equal(e[1], evt_ref["counts"])
    np.testing.assert_array_equal(e[2], evt_ref["invalid"])
    assert en[2] == en_ref["invalid"]
    _within(f"{tag} D2", en[0], en_ref["d2"], MR.energy_tolerance(en_ref))
    _within(f"{tag} S0", en[1], en_ref["s0"], (en_ref["n"][None, :] + 8.0) * 2.0 ** -53 * en_ref["s0"])
    out.update(bins=o[0], extra=o[1], pinball=o[2], ocounts=o[3], tail=t[0], tcounts=t[1], weighted=e[0], ecounts=e[1], d2=en[0], s0=en[1])
    return out

  _both(monkeypatch, tag, case)


# ---- above the block caps: workgroups with an empty node range still store their partials ---------------------------------------
def test_ens_score_above_its_cap(monkeypatch):
  """The 1.5 degree grid and the data of tests/test_gpu_mid_grid.py: loss_reduce_blocks = 2048 workgroups, per = 15, 112 of
  them with an empty node range -- their partials, rank counts and skipped words must be stored zeros, not what the
  allocation held."""
  members, truth, w = MID._data()
  ref = VR.reference(members, truth, w)
  tag = "ens_score 121x240"

  def case(new):
    nd = new.graph(MID.B, MID.C, MID._graph())
    _push_all(nd, members, w)
    sums, hist = nd.ens_score(truth, want_fields=True)
    assert nd.counter("ens_score_blocks") == 2048
    assert nd.counter("ens_invalid_points") == 2 * MID.PLANTED.size
    _check_ens_sums(tag, sums, hist, ref, MID.G, MID.M)
    mean, var = nd.ens_download_fields()
    _check_ens_fields(tag, mean, var, ref)
    return dict(sums=sums, hist=hist, mean=mean, var=var)

  _both(monkeypatch, tag, case)


def test_energy_above_its_cap(monkeypatch):
  """K = 4 on the 1.5 degree grid: 2048 / (B K) = 256 node ranges of 114 nodes, one empty workgroup per (b, k)."""
  members, truth, w = MID._data()
  C = MID.C
  group = (np.arange(C) % 4).astype(np.int32)
  group[C - 1] = -1
  group[3] = 0
  scale = 2.0 ** np.random.default_rng(5).integers(-3, 4, C)
  ref = MR.energy(members, truth, w, group, scale)
  tag = "energy 121x240 K=4"

  def case(new):
    nd = new.graph(MID.B, C, MID._graph())
    _push_all(nd, members, w)
    nd.ens_energy_set(4, group, scale)
    d2, s0, invalid = nd.ens_energy_score(truth)
    assert nd.counter("ens_energy_blocks") == 256
    assert invalid == ref["invalid"] == 2 * MID.PLANTED.size
    _within(f"{tag} D2", d2, ref["d2"], MR.energy_tolerance(ref))
    _within(f"{tag} S0", s0, ref["s0"], (ref["n"][None, :] + 8.0) * 2.0 ** -53 * ref["s0"])
    return dict(d2=d2, s0=s0)

  _both(monkeypatch, tag, case)


# ---- the forward and what hangs on it ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f16x3", "f32", "features_f16"])
def test_denoise_tiny(mode, monkeypatch):
  """`helpers.tiny_setup` against the oracle: TOL in either precision; with fp16 node features (physical fp16 storage on
  the f16x3 kernels: the K / V planes hold halfs and their lo planes are never written) the bound of the fp16 mode."""
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=2)
  if mode == "features_f16":
    ref = _oracle(params, gr, dims, x, sigma, attention="neighbour", feature_dtype=np.float16)
  else:
    ref = _oracle(params, gr, dims, x, sigma)
  tag = f"denoise {mode}"

  def case(new):
    nd = new.native(gr, dims, params, 2, precision="f32" if mode == "f32" else "f16x3")
    if mode == "features_f16":
      nd.set_option("features", "f16")
    y = nd.denoise(x, sigma)
    err = np.abs(y - ref)
    print(f"{tag}: max |device - oracle| {err.max():.3e}")
    if mode == "features_f16":
      assert nd.counter("fp16_storage") == 1
      assert err.max() < F16_TOL_MAX and np.sqrt((err ** 2).mean()) < F16_TOL_RMS
    else:
      assert err.max() < TOL
    assert nd.counter("range_fallbacks") == 0
    stages = {k: nd.debug_fetch(k) for k in ("g0", "m0", "e1", "agg1", "g1", "m2", "agg2", "g2")}
    return dict(y=y, again=nd.denoise(x, sigma), **stages)

  out = _both(monkeypatch, tag, case)
  assert out["again"].tobytes() == out["y"].tobytes()


def test_denoise_batch_three_with_a_ragged_tail_tile(monkeypatch):
  """The second configuration of tests/test_gpu_parity.py::test_other_shapes."""
  cfg = dict(latent=128, heads=1, ffw=384, layers=2, k_hop=3, mesh_size=2)
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=3, seed=7, **cfg)
  ref = _oracle(params, gr, dims, x, sigma)

  def case(new):
    nd = new.native(gr, dims, params, 3)
    y = nd.denoise(x, sigma)
    assert np.abs(y - ref).max() < TOL
    return dict(y=y)

  _both(monkeypatch, "denoise batch 3", case)


def test_denoise_with_two_hidden_layers(monkeypatch):
  """hidden_layers = 2: the leading layer of every MLP hands over through d_mlp_tmp."""
  gr, dims, params, x, sigma = helpers.tiny_setup(batch=2, seed=11, latent=128, heads=2, ffw=256, layers=2, hidden_layers=2)
  ref = _oracle(params, gr, dims, x, sigma)

  def case(new):
    nd = new.native(gr, dims, params, 2)
    y = nd.denoise(x, sigma)
    assert np.abs(y - ref).max() < TOL
    return dict(y=y)

  _both(monkeypatch, "denoise hidden_layers=2", case)


CHURN3 = SC.Case("poison_churn3", "T", SC.karras(3), True, (SC.RATE,) * 3, (), 5, 3, True, False)
PLAIN3 = SC.plain("T", SC.karras(3))


def test_three_level_sample_with_churn(monkeypatch):
  """Three noise levels, churn at every step, after gc_noise_set_tables: the noise scratch, the DPM buffers, the embed
  cache.  Against `sampler_cases.sample_oracle` within its TOL."""
  gr, dims, params, x, lat, lon, slots, noise, _ = SC.setup("T")
  ref, calls, draws = SC.sample_oracle(CHURN3)
  assert (calls, draws) == (CHURN3.calls, CHURN3.draws)

  def case(new):
    nd = new.native(gr, dims, params, x.shape[1])
    nd.noise_set_tables(len(lat), len(lon), *noise_mod.SphericalNoise(lat, lon).device_tables())
    nd.set_noisy_slots(slots)
    nd.set_churn(CHURN3.rates, CHURN3.inflation)
    nd.noise_seed(SC.SEED, 0)
    out, st = nd.sample(x, noise, np.asarray(CHURN3.sigmas), skip_dead_call=True)
    assert st["denoiser_calls"] == calls and nd.counter("noise_stream") == draws
    assert nd.counter("embed_cache") == 1 and nd.counter("range_fallbacks") == 0
    err = float(np.abs(out - ref).max() / max(1.0, np.abs(ref).max()))
    print(f"churn sample: error {err:.3g} of scale")
    assert np.isfinite(out).all() and err < SC.TOL
    nd.noise_draw()                                          # and a drawn initial field: the same on both handles
    return dict(out=out, drawn=nd.download_noise())

  _both(monkeypatch, "sample with churn", case)


@pytest.mark.parametrize("graphs", ["on", "off"])
def test_sample_with_graph_replay_on_and_off(graphs, monkeypatch):
  """The same three-level sample three times: with graphs on the second is captured and the third replayed."""
  gr, dims, params, x, lat, lon, slots, noise, _ = SC.setup("T")
  ref, calls, _ = SC.sample_oracle(PLAIN3)

  def case(new):
    nd = new.native(gr, dims, params, x.shape[1])
    nd.set_option("graphs", graphs)
    nd.set_noisy_slots(slots)
    outs = []
    for _ in range(3):
      out, st = nd.sample(x, noise, np.asarray(PLAIN3.sigmas), skip_dead_call=True)
      assert st["denoiser_calls"] == calls
      outs.append(out)
    assert (nd.counter("graph_replays") >= 1) == (graphs == "on")
    err = float(np.abs(outs[0] - ref).max() / max(1.0, np.abs(ref).max()))
    assert err < SC.TOL
    assert outs[1].tobytes() == outs[0].tobytes() and outs[2].tobytes() == outs[0].tobytes()
    return dict(out=outs[0], replay=outs[2])

  _both(monkeypatch, f"sample graphs {graphs}", case)


def test_edge_terms_small_fixture(monkeypatch):
  """The SMALL case of tests/test_gpu_edge_terms.py (19 x 36 grid, latent 256, batch 1): the per-noise-level edge-term
  caches, every stage the two edge updates feed within that test's bound against the oracle."""
  s = ET._setup(1, 19, 36)
  ref, inter = ET._last_call_oracle(s, ET.SIG)

  def case(new):
    nd = new.native(s["gr"], s["dims"], s["params"], 1)
    nd.set_noisy_slots(s["slots"])
    out = ET._sample(nd, s)
    assert nd.counter("edge_term_samples") == 1 and nd.counter("edge_term_cache_bytes") > 0
    stages = ET._fetch(nd)
    ET._within_bound(stages, inter, "poison: terms vs oracle")
    assert np.abs(out - ref).max() < 1e-4 * max(1.0, np.abs(ref).max())
    return dict(out=out, **stages)

  _both(monkeypatch, "edge terms", case)


def test_loss_tiny(monkeypatch):
  """gc_loss on the tiny case of tests/test_gpu_loss.py, inside that test's derived bound."""
  gr, dims, params, cond, targets, noise = TL._tiny_case()
  weights = TL._tiny_weights()
  ref_loss, ref_pg, _ = TL._reference(weights, cond, targets, noise, TL.SIGMA_ENDS, TL._slots(dims),
                                      TL._network(params, gr, dims, attention="dense"))

  def case(new):
    nd = new.native(gr, dims, params, 2)
    TL._ready(nd, dims, weights)
    loss, per_group = nd.loss(cond, targets, noise, TL.SIGMA_ENDS)
    TL._assert_within_bound("poison loss", loss, per_group, ref_loss, ref_pg, TL.SIGMA_ENDS, weights[3], TL.TOL)
    assert nd.counter("loss_evaluations") == 1 and nd.counter("range_fallbacks") == 0
    return dict(loss=loss, per_group=per_group)

  _both(monkeypatch, "loss", case)


def test_rollout_advance(monkeypatch):
  """One gc_rollout_advance after a resident sample against oracle/rollout_oracle.apply_plan, the bound of
  tests/test_gpu_host_api.py::test_rollout_advance_matches_the_rollout_oracle, on that test's model (9 x 16 grid, 262 -> 82
  channels, batch 2) and its plan with the normalisation wrapper (kinds 1, 2, 3)."""
  from gencast_flax_nnx_amd import rollout
  from oracle import rollout_oracle as RO
  from tests import test_gpu_host_api as HA
  from tests.test_rollout import _stats
  from gencast_flax_nnx_amd import GenCast, config, datasets, synthetic, weights
  arch = HA._small_arch()
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=2, seed=6)
  sc = config.SamplerConfig(num_noise_levels=3, stochastic_churn_rate=0.0)
  params = weights.random_params(HA.dims_from_arch(arch, 262, 82), seed=3)

  def case(new):
    gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=1)
    tmpl = datasets.zeros_like(tgt)
    den = gc.denoiser
    cond, _, slots = den.init_for(inp, tmpl, frc)
    nd = new(den.native)
    nd.set_noisy_slots(slots)
    Gs = cond.shape[0]
    sig = np.asarray(gc._sampler.noise_levels, np.float32)
    plan, _ = rollout.build_rollout_plan(rollout.isel_time(inp, slice(-2, None)), frc, tmpl, config.TASK,
                                         rollout.InputsAndResiduals(gc, *_stats(config.TASK)))
    nd.rollout_plan(**plan)
    nd.upload_cond(cond)
    r = np.random.default_rng(9)
    nd.upload_noise(r.standard_normal((Gs, 2, 82)).astype(np.float32))
    nd.sample_resident(sig, skip_dead_call=True, want_stats=False)
    sample = nd.download_sample()
    forc = r.standard_normal((Gs, 2, plan["n_forcing"])).astype(np.float32)
    nd.rollout_advance(forc)
    got = nd.download_cond()
    want = RO.apply_plan(cond.astype(np.float64), sample.astype(np.float64), forc.astype(np.float64), plan)
    keep = np.ones(cond.shape[-1], bool)
    keep[slots] = False                                     # the sampler rewrites the noisy-target slots
    scale = max(1.0, float(np.abs(want[..., keep]).max()))
    assert np.abs(got[..., keep] - want[..., keep]).max() < 2e-6 * scale
    return dict(sample=sample, cond=got[..., keep])

  _both(monkeypatch, "rollout advance", case)
