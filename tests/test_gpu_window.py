"""Time-window ensemble fields on the device (gc_ens_window_*) against the definition restated in
tests/window_reference.py.  The device performs the same IEEE operations in the same order as the float64 restatement, so
every comparison of fields is bit equality (a NaN matches any NaN: its payload is free).

Sizes: the 13 x 24 grid (G = 312) and the 11 x 15 grid (G = 165), handles with set_graph only.  (B, C, M) = (2, 6, 9):
(M + 1) field = 37440 floats, 37 blocks; (1, 82, 2): 76752 floats, M field = 51168 divisible by four; (1, 7, 2) on the odd
grid: field = 1155, so M field = 2310 is no multiple of four -- the float4 of one thread lies across the seam between the
member store and the truth buffer -- and the slot is padded by three floats.

`device_allocations` counts buffers, and the ring is one buffer whatever L is: when L changes the ring is freed and made
again, which the count cannot show.  What changes once is "ens_window_ring_bytes"; the count is held flat throughout."""
import functools

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, losses
from tests import derive_reference as DR
from tests import helpers
from tests import window_reference as R
from tests.helpers import graph_handle as _handle

pytestmark = pytest.mark.gpu

GRIDS = {"even": (13, 24), "odd": (11, 15)}
SHAPES = [("even", 2, 6, 9), ("even", 1, 82, 2), ("odd", 1, 7, 2)]           # grid, B, C, M
LENGTHS = (1, 2, 3, 5)
FORMS = [("sum", None), ("mean", None), ("change", None), ("linear", "zero and negative"), ("max", None), ("min", None)]


@functools.lru_cache(maxsize=None)
def _graph(which):
  n_lat, n_lon = GRIDS[which]
  gr = helpers.small_graph(n_lat, n_lon)
  assert gr.num_grid_nodes == n_lat * n_lon
  return gr


def _linear_coef(L):
  """A zero, a negative and otherwise uneven coefficients (none of them a power of two: the products round)."""
  a = np.array([0.3, -1.7, 0.0, 2.1, -0.9])[:L].copy()
  if L == 1:
    a[0] = -1.7
  return a


def _plan(form, L):
  kind, _ = form
  coef = _linear_coef(L) if kind == "linear" else None
  return R.coefficients(kind, L, coef)


def _fields(which, B, C, M, n, seed):
  """n pushes, each [M + 1, G, B, C]: M members, then the truth, with what the window must turn into NaN, ties and zeros
  of both signs for the extremes, and values whose sums leave float32 range."""
  n_lat, n_lon = GRIDS[which]
  G = n_lat * n_lon
  rng = np.random.default_rng(seed)
  f = (rng.standard_normal((n, M + 1, G, B, C)) * np.logspace(-2, 3, C)).astype(np.float32)
  k = 12 * n

  def scatter(c, value):
    f[rng.integers(0, n, k), rng.integers(0, M + 1, k), rng.integers(0, G, k), rng.integers(0, B, k), c] = value

  scatter(0, np.nan)                                        # scattered NaN, +inf, -inf: in members and in the truth
  scatter(1, np.inf)
  scatter(1, -np.inf)
  f[:, :, :, 0, 2] = rng.integers(-2, 3, (n, M + 1, G)).astype(np.float32)     # ties
  f[:, :, :, B - 1, 2] = np.where(rng.integers(0, 2, (n, M + 1, G)) == 1, np.float32(0.0), np.float32(-0.0))   # +0 and -0
  f[:, :, :, B - 1, 3] = np.nan                             # a whole NaN column
  f[:, :, :, 0, 4] = np.float32(7.25)                       # a constant field
  f[:, :, :, B - 1, 5] = (rng.uniform(1.0, 3.0, (n, M + 1, G)) * 1e38).astype(np.float32)   # sums beyond float32 range
  f[n - 1, M, 5, 0, C - 1] = np.nan                         # one NaN in the newest truth only
  return f


def _push_all(nd, members):
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _members(nd, M):
  return np.stack([nd.ens_download_member(i) for i in range(M)])


def _assert_bits(got, want, tag):
  assert R.same_bits(got, want), f"{tag}: {int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {got.size} words differ"


def _reference(pushes, L, kind, coef):
  return R.window(R.last(pushes, L), kind, coef)


# ---- 1. every kind, every length, wrapped ring starts; 3a. the truth by rotation ---------------------------------------------
@pytest.mark.parametrize("which,B,C,M", SHAPES)
def test_every_kind_equals_the_definition_bit_for_bit(which, B, C, M):
  gr = _graph(which)
  G = gr.num_grid_nodes
  n_max = 2 * max(LENGTHS) + 2
  f = _fields(which, B, C, M, n_max, seed=C + M)
  src = _handle(gr, B, C)
  wins = {form: _handle(gr, B, C) for form in FORMS}
  try:
    src.ens_reserve(M)
    for w in wins.values():
      w.ens_reserve(M)
    checked = nan_out = 0
    for rotate in (False, True):                            # rotated: the former truth lies in a slot (once per shape, L = 3)
      for L in ((3,) if rotate else LENGTHS):
        stops = {L, L + 1, 2 * L + 2}
        forms = [fm for fm in FORMS if not (fm[0] == "change" and L < 2)]
        for fm in forms:
          kind, coef = _plan(fm, L)
          wins[fm].ens_window_set(kind, L, coef)
        pushes = []
        for i in range(max(stops)):
          x = np.roll(f[i], -1, axis=0) if rotate else f[i]
          pushes.append(x)
          _push_all(src, x[:M])
          for j, fm in enumerate(forms):
            wins[fm].ens_window_push(src, x[M] if j == 0 else None)      # the first uploads the truth into src, the rest find it
          if i + 1 not in stops:
            continue
          for fm in forms:
            kind, coef = _plan(fm, L)
            w = wins[fm]
            w.ens_window_emit()
            want = _reference(pushes, L, kind, coef)
            got = _members(w, M)
            _assert_bits(got, want[:M], f"{fm[0]} L={L} n={i + 1} rotate={rotate}")
            assert w.counter("ens_window_pushes") == i + 1
            checked += 1
            nan_out += int(np.isnan(got).sum())
            if fm[0] == "sum" and L > 1:
              assert np.isinf(got[..., B - 1, 5]).any()     # a finite double beyond float32 range: +inf, and it stays
            if fm[0] in ("max", "min"):                     # one of the inputs' bits
              stack = R.last(pushes, L)[:, :M]
              hit = (stack.view(np.uint32) == got.view(np.uint32)[None]).any(axis=0) | np.isnan(got)
              assert hit.all()
    assert checked == (len(LENGTHS) * len(FORMS) - 1 + len(FORMS)) * 3 and nan_out > 0
    w = wins[FORMS[0]]
    stride = ((M + 1) * G * B * C + 3) // 4 * 4
    assert w.counter("ens_window_ring_bytes") == 3 * stride * 4
    print(f"{which} ({B}, {C}, {M}): ens_window_device_us {w.counter('ens_window_device_us')}, emits {w.counter('ens_window_emits')}")
  finally:
    src.close()
    for w in wins.values():
      w.close()


# ---- 2. sliding windows; 6. the same emit twice -------------------------------------------------------------------------------
def test_an_emit_after_every_push_gives_sliding_windows_and_twice_the_same_bytes():
  which, B, C, M = SHAPES[0]
  gr, L, n = _graph(which), 3, 9
  f = _fields(which, B, C, M, n, seed=21)
  src, wmax, wmean = _handle(gr, B, C), _handle(gr, B, C), _handle(gr, B, C)
  try:
    for h in (src, wmax, wmean):
      h.ens_reserve(M)
    wmax.ens_window_set(R.MAX, L)
    wmean.ens_window_set(*R.coefficients("mean", L)[:1], L, R.coefficients("mean", L)[1])
    for i in range(n):
      _push_all(src, f[i, :M])
      wmax.ens_window_push(src, f[i, M])
      wmean.ens_window_push(src)
      if i + 1 < L:
        with pytest.raises(_lib.GencastHipError, match=f"needs {L} pushes, the ring holds {i + 1}"):
          wmax.ens_window_emit()
        continue
      for w, (kind, coef) in ((wmax, (R.MAX, None)), (wmean, R.coefficients("mean", L))):
        w.ens_window_emit()
        first = _members(w, M)
        _assert_bits(first, _reference(list(f[:i + 1]), L, kind, coef)[:M], f"sliding kind {kind} after push {i + 1}")
        w.ens_window_emit()                                 # the ring is unchanged: the same bytes again
        assert _members(w, M).tobytes() == first.tobytes()
    assert wmax.counter("ens_window_emits") == 2 * (n - L + 1) and wmax.counter("ens_window_pushes") == n
  finally:
    for h in (src, wmax, wmean):
      h.close()


# ---- 3b. the truth through the scorers of the window handle --------------------------------------------------------------------
@pytest.mark.parametrize("which,B,C,M", SHAPES)
def test_the_scorers_of_the_window_handle_see_the_windowed_members_and_truth(which, B, C, M):
  gr, L = _graph(which), 2
  G = gr.num_grid_nodes
  f = _fields(which, B, C, M, L + 1, seed=31 + C)
  w_node = np.random.default_rng(3).uniform(0.1, 2.0, G).astype(np.float32)
  src, win, plain = _handle(gr, B, C), _handle(gr, B, C), _handle(gr, B, C)
  try:
    for h in (src, win, plain):
      h.ens_reserve(M)
    for h in (win, plain):
      h.ens_set_node_weight(w_node)
    kind, coef = R.coefficients("sum", L)
    win.ens_window_set(kind, L, coef)
    for i in range(L + 1):
      _push_all(src, f[i, :M])
      win.ens_window_push(src, f[i, M])
    win.ens_window_emit()
    want = _reference(list(f), L, kind, coef)
    _push_all(plain, want[:M])
    sums_ref, hist_ref = plain.ens_score(want[M])
    sums, hist = win.ens_score(None)                        # the windowed truth is on the device
    assert sums.tobytes() == sums_ref.tobytes() and hist.tobytes() == hist_ref.tobytes()
    assert np.isfinite(sums[..., 0]).all() and sums[0, 0, 0] > 0
    # an emit leaves mean / variance fields of the store before as not computed
    win.ens_score(None, want_fields=True)
    win.ens_window_emit()
    with pytest.raises(_lib.GencastHipError, match="no mean / variance"):
      win.ens_download_fields()
  finally:
    for h in (src, win, plain):
      h.close()


# ---- 4. the ring is a copy -----------------------------------------------------------------------------------------------------
def test_the_ring_is_a_copy_and_the_source_is_left_alone():
  which, B, C, M = SHAPES[0]
  gr, L = _graph(which), 2
  G = gr.num_grid_nodes
  f = _fields(which, B, C, M, 3, seed=41)
  src, win = _handle(gr, B, C), _handle(gr, B, C)
  try:
    src.ens_reserve(M)
    win.ens_reserve(M)
    src.ens_set_node_weight(np.ones(G, np.float32))
    win.ens_window_set(R.MIN, L)
    for i in range(L):
      _push_all(src, f[i, :M])
      win.ens_window_push(src, f[i, M])
    _push_all(src, f[2, :M])                                # the source moves on; the ring holds the old values
    before_members = _members(src, M)
    before = src.ens_score(f[2, M])
    win.ens_window_emit()
    _assert_bits(_members(win, M), _reference(list(f[:2]), L, R.MIN, None)[:M], "the old values")
    after = src.ens_score(None)
    assert _members(src, M).tobytes() == before_members.tobytes() == f[2, :M].tobytes()
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    win.ens_window_push(src)                                # ... and the next push takes the new ones, truth included
    win.ens_window_emit()
    _assert_bits(_members(win, M), _reference(list(f[:3]), L, R.MIN, None)[:M], "after the next push")
  finally:
    src.close()
    win.close()


# ---- 5. a derived view as the source ---------------------------------------------------------------------------------------------
def test_a_window_over_a_derived_view_is_the_composition_of_the_two_definitions():
  which, B, C, M = SHAPES[0]
  gr, L, n = _graph(which), 3, 4
  n_lat, n_lon = GRIDS[which]
  rng = np.random.default_rng(51)
  f = rng.standard_normal((n, M + 1, n_lat * n_lon, B, C)).astype(np.float32)
  f[1, 2, 40, 0, 0] = np.nan
  f[2, M, 77, 1, 1] = np.inf
  lat = np.linspace(-90, 90, n_lat)
  plan = dict(c_src=C, op=np.array([1, 0], np.int32), src_a=np.array([0, 4], np.int32), src_b=np.array([1, 0], np.int32),
              affine=np.array([[3.7, -12.5, 0.9, 4.0], [1.0, 0.0, 1.0, 0.0]]), pool=DR.MAX, n_lat=n_lat, n_lon=n_lon, r_lat=1,
              r_lon=np.full(n_lat, 2, np.int32), row_weight=np.asarray(losses.normalized_latitude_weights(lat), np.float64))
  src, view, win = _handle(gr, B, C), _handle(gr, B, 2), _handle(gr, B, 2)
  try:
    for h in (src, view, win):
      h.ens_reserve(M)
    view.ens_derive_set(**plan)
    win.ens_window_set(R.MAX, L)
    derived, device_derived = [], []
    for i in range(n):
      _push_all(src, f[i, :M])
      view.ens_derive(src, f[i, M])
      win.ens_window_push(view)                             # the derived truth is on the view
      derived.append(DR.apply(f[i], plan))
      device_derived.append(_members(view, M))
    win.ens_window_emit()
    got = _members(win, M)
    _assert_bits(got, R.window(np.stack(device_derived[-L:]), R.MAX), "the window of the device's own derived members")
    _assert_bits(got, _reference(derived, L, R.MAX, None)[:M], "the composition of the two references")
    assert np.isnan(got).any() and np.isfinite(got).any()
  finally:
    for h in (src, view, win):
      h.close()


# ---- 7. device allocations ---------------------------------------------------------------------------------------------------
def test_device_allocations_stay_flat_and_the_ring_is_made_again_only_when_its_size_changes():
  which, B, C, M = SHAPES[2]
  gr = _graph(which)
  G = gr.num_grid_nodes
  f = _fields(which, B, C, M, 3, seed=61)
  stride_bytes = ((M + 1) * G * B * C + 3) // 4 * 4 * 4
  src, win = _handle(gr, B, C), _handle(gr, B, C)
  try:
    src.ens_reserve(M)
    win.ens_reserve(M)
    _push_all(src, f[0, :M])
    assert win.counter("ens_window_ring_bytes") == 0

    def round_trip(L):
      for i in range(L):
        win.ens_window_push(src, f[i % 3, M])
      win.ens_window_emit()
      win.ens_window_reset()
      assert win.counter("ens_window_pushes") == 0

    win.ens_window_set(R.LINEAR, 2, [1.0, 1.0])
    round_trip(2)
    base = win.counter("device_allocations")
    for r in range(20):
      if r % 5 == 4:
        win.ens_window_set(R.MAX if r % 2 else R.LINEAR, 2, None if r % 2 else [0.5, 0.5])      # a new plan of the same length
      round_trip(2)
      assert win.counter("device_allocations") == base and win.counter("ens_window_ring_bytes") == 2 * stride_bytes
    win.ens_window_set(R.MAX, 5)
    assert win.counter("ens_window_ring_bytes") == 2 * stride_bytes      # the old ring, until the first push
    round_trip(5)
    assert win.counter("ens_window_ring_bytes") == 5 * stride_bytes      # changed once: one buffer freed, one made
    assert win.counter("device_allocations") == base
    for _ in range(20):
      round_trip(5)
      assert win.counter("device_allocations") == base and win.counter("ens_window_ring_bytes") == 5 * stride_bytes
    src.ens_reserve(M + 1)                                               # another M: the ring is sized by the first push again
    win.ens_reserve(M + 1)
    _push_all(src, f[0, :M + 1])
    round_trip(5)
    assert win.counter("ens_window_ring_bytes") == 5 * (((M + 2) * G * B * C + 3) // 4 * 4 * 4)
  finally:
    src.close()
    win.close()


# ---- 8. every documented error ---------------------------------------------------------------------------------------------------
def test_every_documented_error():
  gr = _graph("even")
  G, B, C, M = gr.num_grid_nodes, 2, 6, 2
  f = _fields("even", B, C, M, 2, seed=71)
  dp = _lib.ctypes.POINTER(_lib.ctypes.c_double)
  INV, STATE, UNSUP, OK = _lib.GC_ERR_INVALID_ARGUMENT, _lib.GC_ERR_STATE, _lib.GC_ERR_UNSUPPORTED, _lib.GC_OK
  ones = np.ones(64)

  def c_set(h, kind, length, coef=ones):
    return h._lib.gc_ens_window_set(h._h, kind, length, None if coef is None else coef.ctypes.data_as(dp))

  def message(h):
    return h._lib.gc_last_error(h._h).decode()

  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  src, win, other_b, other_c = _handle(gr, B, C), _handle(gr, B, C), _handle(gr, B + 1, C), _handle(gr, B, C + 1)
  small = _handle(_graph("odd"), B, C)
  lib = win._lib
  try:
    # ---- gc_ens_window_set
    assert c_set(bare, 0, 2) == STATE and "gc_set_graph" in message(bare)
    assert lib.gc_ens_window_push(bare._h, src._h, None) == STATE and lib.gc_ens_window_emit(bare._h) == STATE
    for kind, length, coef, code, word in ((0, 0, ones, INV, "at least 1"), (1, -3, None, INV, "at least 1"), (0, 2, None, INV, "coefficients"),
                                           (0, 2, np.array([1.0, np.nan]), INV, "coef[1]"), (0, 3, np.array([np.inf, 1.0, 1.0]), INV, "coef[0]"),
                                           (0, 2, np.array([1.0, -np.inf]), INV, "coef[1]"), (3, 2, ones, UNSUP, "kind"), (-1, 2, ones, UNSUP, "kind"),
                                           (0, 65, np.ones(65), UNSUP, "at most 64"), (2, 1000, None, UNSUP, "at most 64")):
      assert c_set(win, kind, length, coef) == code, (kind, length)
      assert word in message(win), (kind, length, message(win))
    assert c_set(win, 1, 2, np.array([np.nan, np.nan])) == OK            # the coefficients of an extreme are not read
    assert c_set(win, 0, 64) == OK and c_set(win, 2, 1, None) == OK
    for args in ((3, 2), (0, 0, [1.0]), (1, 65), (0, 2), (0, 2, [1.0]), (0, 2, [1.0, np.inf]), (1, 2, [1.0, 1.0])):
      with pytest.raises(ValueError):
        win.ens_window_set(*args)
    # ---- gc_ens_window_push / _emit before a plan
    fresh = _handle(gr, B, C)
    try:
      assert lib.gc_ens_window_push(fresh._h, src._h, None) == STATE and "no plan" in message(fresh)
      assert lib.gc_ens_window_emit(fresh._h) == STATE and "no plan" in message(fresh)
      assert lib.gc_ens_window_reset(fresh._h) == OK
      with pytest.raises(_lib.GencastHipError, match="no plan"):
        fresh.ens_window_push(src)
      with pytest.raises(_lib.GencastHipError, match="no plan"):
        fresh.ens_window_emit()
    finally:
      fresh.close()
    win.ens_window_set(R.MAX, 2)
    assert lib.gc_ens_window_push(win._h, win._h, None) == INV and lib.gc_ens_window_push(win._h, None, None) == INV
    for bad in (win, None, "src"):
      with pytest.raises(ValueError, match="another NativeDenoiser"):
        win.ens_window_push(bad)
    for h in (bare, other_b, other_c, small):                 # no graph; another batch; another c_out; another G
      assert lib.gc_ens_window_push(win._h, h._h, None) == INV
      with pytest.raises(ValueError, match="other dimensions"):
        win.ens_window_push(h)
    with pytest.raises(_lib.GencastHipError, match="no member store on the source"):
      win.ens_window_push(src, f[0, M])
    src.ens_reserve(M)
    src.ens_push_host(0, f[0, 0])
    with pytest.raises(_lib.GencastHipError, match="source member slot 1 has not been pushed"):
      win.ens_window_push(src, f[0, M])
    src.ens_push_host(1, f[0, 1])
    with pytest.raises(_lib.GencastHipError, match="no truth on the source"):
      win.ens_window_push(src)
    assert lib.gc_ens_window_push(win._h, src._h, None) == STATE
    with pytest.raises(ValueError, match="truth must be"):
      win.ens_window_push(src, f[0, M][..., :C - 1])
    assert win.counter("ens_window_pushes") == 0
    win.ens_window_push(src, f[0, M])
    with pytest.raises(_lib.GencastHipError, match="needs 2 pushes, the ring holds 1"):
      win.ens_window_emit()
    win.ens_window_push(src)                                  # the truth stays in the source
    with pytest.raises(_lib.GencastHipError, match="no member store"):       # on win
      win.ens_window_emit()
    win.ens_reserve(M + 1)
    with pytest.raises(_lib.GencastHipError, match="the member store holds 3 members, the ring 2"):
      win.ens_window_emit()
    src.ens_reserve(M + 1)
    _push_all(src, np.concatenate([f[1, :M], f[0, :1]]))
    with pytest.raises(_lib.GencastHipError, match="the source holds 3 members, the ring 2"):
      win.ens_window_push(src)
    assert win.counter("ens_window_pushes") == 2 and win.counter("ens_window_emits") == 0
    win.ens_window_reset()                                    # ... reset first: then the ring takes the new M
    win.ens_window_push(src)
    win.ens_window_push(src)
    win.ens_window_emit()
    assert win.counter("ens_window_emits") == 1
    with pytest.raises(ValueError):
      win.counter("ens_window_no_such_counter")
  finally:
    for h in (bare, src, win, other_b, other_c, small):
      h.close()
