"""Time windows without a GPU: `WindowSpec` (validation, coefficients, lead times, the affine map to physical units), the
float64 definition (tests/window_reference.py) on hand-made cases, the argument checks of the binding, the call sequence of
a rollout with `windows=` on handles that record, and the results' merges."""
import os
import re

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, datasets, rollout, verification
from gencast_flax_nnx_amd.verification import EnsembleScores, EventScores, EventSpec, WindowSpec
from tests import window_reference as R
from tests.helpers import RecordingHandle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["gc_ens_window_set", "gc_ens_window_push", "gc_ens_window_emit", "gc_ens_window_reset"]


# ---- WindowSpec -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,kw,match", [
    (("median", 2), {}, "kind must be"), (("sum", 0), {}, "1 .. 64"), (("sum", 65), {}, "1 .. 64"), (("sum", 2.5), {}, "1 .. 64"),
    (("sum", True), {}, "1 .. 64"), (("change", 1), {}, "steps >= 2"), (("sum", 2), dict(stride=0), "stride"),
    (("sum", 2), dict(stride=1.5), "stride"), (("sum", 2), dict(source=3), "source"), (("linear", 3), {}, "needs coef"),
    (("linear", 3), dict(coef=[1.0, 2.0]), "3 entries"), (("linear", 2), dict(coef=[1.0, np.inf]), "finite"),
    (("linear", 2), dict(coef=[np.nan, 1.0]), "finite"), (("max", 2), dict(coef=[1.0, 1.0]), "only kind 'linear'"),
    (("sum", 2), dict(coef=[1.0, 1.0]), "only kind 'linear'")])
def test_window_spec_refuses_what_the_device_would_refuse(args, kw, match):
  with pytest.raises(ValueError, match=match):
    WindowSpec(*args, **kw)


def test_the_coefficients_of_every_kind():
  np.testing.assert_array_equal(WindowSpec("sum", 3).coefficients(), [1.0, 1.0, 1.0])
  m = WindowSpec("mean", 3).coefficients()
  assert m.dtype == np.float64 and np.all(m == 1.0 / 3)                  # the double nearest 1 / 3, three times
  np.testing.assert_array_equal(WindowSpec("change", 4).coefficients(), [-1.0, 0.0, 0.0, 1.0])
  np.testing.assert_array_equal(WindowSpec("change", 2).coefficients(), [-1.0, 1.0])
  np.testing.assert_array_equal(WindowSpec("linear", 3, coef=[0.5, 0.0, -2.0]).coefficients(), [0.5, 0.0, -2.0])
  assert WindowSpec("max", 3).coefficients() is None and WindowSpec("min", 1).coefficients() is None
  for kind, steps, coef in (("sum", 5, None), ("mean", 7, None), ("change", 3, None), ("linear", 2, [3.0, -1.0]), ("max", 4, None),
                            ("min", 2, None)):
    spec = WindowSpec(kind, steps, coef=coef)
    k, a = R.coefficients(kind, steps, coef)
    plan = spec.plan()
    assert plan["kind"] == k and plan["length"] == steps and sorted(plan) == ["coef", "kind", "length"]
    if a is None:
      assert plan["coef"] is None
    else:
      np.testing.assert_array_equal(plan["coef"], a)
  one = WindowSpec("sum", 1)                                             # the window of one lead time: the field itself
  np.testing.assert_array_equal(one.coefficients(), [1.0])


def test_leads_of_tumbling_sliding_and_strided_windows():
  assert WindowSpec("sum", 2).leads(5) == [1, 3]                         # tumbling: stride = steps
  assert WindowSpec("sum", 2).stride == 2
  assert WindowSpec("max", 3, stride=1).leads(5) == [2, 3, 4]            # sliding
  assert WindowSpec("mean", 3, stride=2).leads(8) == [2, 4, 6]
  assert WindowSpec("mean", 2, stride=3).leads(8) == [1, 4, 7]
  assert WindowSpec("sum", 6).leads(5) == []                             # longer than the rollout: no window
  assert WindowSpec("sum", 5).leads(5) == [4]
  assert WindowSpec("sum", 1).leads(3) == [0, 1, 2]
  for spec in (WindowSpec("sum", 2), WindowSpec("max", 3, stride=1), WindowSpec("mean", 3, stride=2)):
    for k in spec.leads(20):
      assert k + 1 >= spec.steps and (k + 1 - spec.steps) % spec.stride == 0


def test_channel_stats_map_a_windowed_value_to_physical_units():
  scale, loc = np.array([2.0, 0.5, 8.0]), np.array([1.0, -3.0, 0.25])
  for spec, factor in ((WindowSpec("sum", 4), 4.0), (WindowSpec("change", 3), 0.0), (WindowSpec("linear", 2, coef=[0.5, -2.0]), -1.5),
                       (WindowSpec("max", 4), 1.0), (WindowSpec("min", 2), 1.0)):
    s, l = spec.channel_stats(scale, loc)
    np.testing.assert_array_equal(s, scale)
    np.testing.assert_array_equal(l, loc * factor)
  s, l = WindowSpec("mean", 3).channel_stats(scale, loc)
  np.testing.assert_allclose(l, loc, rtol=1e-15)
  # the map is the one it claims to be: the window of x = scale n + loc is scale (the window of n) + loc_w
  rng = np.random.default_rng(0)
  n = rng.integers(-8, 9, (4, 5, 3)).astype(np.float32)                  # small integers, dyadic statistics: all exact
  x = (n * scale + loc).astype(np.float32)
  for spec in (WindowSpec("sum", 4), WindowSpec("change", 4), WindowSpec("max", 4), WindowSpec("min", 4),
               WindowSpec("linear", 4, coef=[1.0, 0.0, -2.0, 0.5])):
    k, a = R.coefficients(spec.kind, 4, spec.coef)
    s, l = spec.channel_stats(scale, loc)
    np.testing.assert_array_equal(R.window(x, k, a), (R.window(n, k, a) * s + l).astype(np.float32))
  with pytest.raises(ValueError, match="same shape"):
    WindowSpec("sum", 2).channel_stats(scale, loc[:2])


# ---- the definition on hand-made cases ---------------------------------------------------------------------------------------
def test_the_reference_is_the_definition_on_cases_done_by_hand():
  f = np.float32
  x = np.array([[1.0, np.nan, 3.0, -0.0, 1e38], [2.0, 1.0, np.inf, 0.0, 3e38], [4.0, 5.0, 1.0, -0.0, 3e38]], f)
  s = R.window(x, R.LINEAR, np.ones(3))
  assert s[0] == 7.0 and np.isnan(s[1]) and np.isnan(s[2]) and s[3] == 0.0 and s[4] == np.inf    # beyond float32: +inf, kept
  z = R.window(x, R.LINEAR, np.array([1.0, 0.0, 1.0]))
  assert z[0] == 5.0 and np.isnan(z[2])                                  # a zero coefficient does not hide a missing step
  mx, mn = R.window(x, R.MAX), R.window(x, R.MIN)
  assert mx[0] == 4.0 and mn[0] == 1.0 and np.isnan(mx[1]) and np.isnan(mn[2]) and mx[4] == f(3e38)
  assert np.signbit(mx[3]) and np.signbit(mn[3])                         # a tie keeps the older value: -0 came first
  assert not np.signbit(R.window(x[1:, 3:4], R.MAX)[0])                  # ... and here +0 did
  # rounded product, then rounded sum: not a fused multiply-add
  a = np.array([1.0 + 2.0 ** -30, -1.0])
  y = np.array([[1.0 + 2.0 ** -23], [1.0 + 2.0 ** -23]], f)
  p = (1.0 + 2.0 ** -30) * float(y[0, 0])
  assert R.window(y, R.LINEAR, a)[0] == f(p - float(y[1, 0]))
  assert R.same_bits(np.array([np.nan, 1.0], f), np.array([-np.nan, 1.0], f)) and not R.same_bits(np.array([0.0], f), np.array([-0.0], f))
  assert R.last([1, 2, 3, 4], 2).tolist() == [3, 4]


# ---- the binding ----------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_entries_and_the_package_binds_them():
  import gencast_flax_nnx_amd as pkg
  text = open(os.path.join(ROOT, "include", "gencast_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  for name in ENTRIES:
    assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert name in _lib.SIGNATURES
  listed = [l.strip() for l in open(os.path.join(ROOT, "gencast-flax-nnx_amd", "csrc", "SOURCES"))]
  assert "gc_window.hip" in listed
  assert pkg.WindowSpec is WindowSpec and "WindowSpec" in pkg.__all__ and "WindowRolloutResult" in pkg.__all__
  for owner, name in ((pkg.Denoiser, "window_handle"), (_lib.NativeDenoiser, "ens_window_set"), (_lib.NativeDenoiser, "ens_window_push"),
                      (_lib.NativeDenoiser, "ens_window_emit"), (_lib.NativeDenoiser, "ens_window_reset")):
    assert callable(getattr(owner, name)), name
  assert not hasattr(pkg.GenCast, "ensemble_window")                     # a window needs several lead times
  if os.path.exists(_lib.LIB_PATH):
    lib = _lib.load_library()
    for name in ENTRIES:
      assert hasattr(lib, name), name


def test_the_binding_checks_its_arguments_before_the_call():
  nd, other = object.__new__(_lib.NativeDenoiser), object.__new__(_lib.NativeDenoiser)
  nd._window_length = 0
  for args, match in (((3, 2), "kind must be"), ((0, 0, [1.0]), "1 .. 64"), ((1, 65), "1 .. 64"), ((0, 2), "needs its coefficients"),
                      ((0, 2, [1.0]), "shape"), ((0, 2, [1.0, np.nan]), "finite"), ((1, 2, [1.0, 1.0]), "only a linear")):
    with pytest.raises(ValueError, match=match):
      nd.ens_window_set(*args)
  with pytest.raises(_lib.GencastHipError, match="ens_window_set"):
    nd.ens_window_push(other)
  with pytest.raises(_lib.GencastHipError, match="ens_window_set"):
    nd.ens_window_emit()
  nd._window_length = 2
  with pytest.raises(ValueError, match="another NativeDenoiser"):
    nd.ens_window_push(nd)
  with pytest.raises(ValueError, match="another NativeDenoiser"):
    nd.ens_window_push("not a handle")


# ---- a rollout on handles that record ----------------------------------------------------------------------------------------
G, B, C, M = 6, 1, 2, 3


def _FakeHandle(name, log):
  return RecordingHandle(name, log, M=M, B=B, C=C, G=G, Q=1)      # (the hand-made main store and view are never set up)


def _targets(horizon):
  dims = ("batch", "time", "lat", "lon")
  rng = np.random.default_rng(1)
  return datasets.Dataset({"a": datasets.Variable(dims, rng.standard_normal((B, horizon, 2, 3)).astype(np.float32)),
                           "b": datasets.Variable(dims, rng.standard_normal((B, horizon, 2, 3)).astype(np.float32))},
                          {"lat": np.array([-45.0, 45.0]), "lon": np.array([0.0, 120.0, 240.0])})


def _run(horizon, windows, log, order=None, keep_members=True):
  """The state `EnsembleRollout._setup` would have made, on handles that record: a main store, one derived view "view" and
  the window entries."""
  w = np.ones(G, np.float32)
  wq = verification.quantize_node_weights(w)
  run = rollout._EnsembleRun()
  main, view = _FakeHandle("main", log), _FakeHandle("view", log)
  run.native, run.M, run.scale, run.loc, run.shape, run.normalized = main, M, np.ones(C), np.zeros(C), (G, B, C), False
  run.main = rollout._StoreSeries(verification.ScoredStore(main, M, w, order=order), np.ones(C), None, keep_members=keep_members)
  run.scores = run.main.scores                           # (the tests below read the main store's scores as `run.scores`)
  run.want_fields = run.want_spectra = False
  vstore = verification.ScoredStore(view, M, w, plan={"op": [0, 0]}, source=main, order=order)
  run.views["view"] = rollout._StoreSeries(vstore, np.ones(C), None, keep_members=keep_members)
  template = rollout.isel_time(_targets(1), slice(0, 1))
  for name, entry in windows.items():
    spec, ev = entry if isinstance(entry, tuple) else (entry, None)
    source = main if spec.source is None else view
    store = verification.ScoredStore(_FakeHandle(name, log), M, w, events=ev, weight_q=wq, order=order,
                                     thresholds=None if ev is None else ev.packed(template))
    series = rollout._StoreSeries(store, np.ones(C), template, keep_members=keep_members)
    run.windows[name] = rollout._WindowEntry(spec, series, source, horizon)
    run.windows[name].start()
  return run


def test_a_rollout_pushes_at_every_lead_and_emits_at_the_window_leads():
  horizon, log = 5, []
  ev = EventSpec({"a": np.array([0.5]), "b": np.array([0.5])}, [1])
  windows = {"acc": WindowSpec("sum", 2), "gust": (WindowSpec("max", 3, stride=1, source="view"), ev),
             "none": WindowSpec("mean", 6)}
  run = _run(horizon, windows, log)
  # the start of a run: every entry's store, its plan, and ONE reset
  for name, plan in (("acc", (0, 2, (1.0, 1.0))), ("gust", (1, 3, None)), ("none", (0, 6, (1.0 / 6,) * 6))):
    mine = [c[1:] for c in log if c[0] == name]
    assert mine[:2] == [("reserve", M), ("weight",)] and mine[-2:] == [("window_set",) + plan, ("window_reset",)]
    assert ("event_set" in [c[0] for c in mine]) == (name == "gust")
  targets = _targets(horizon)
  for k in range(horizon):
    del log[:]
    rollout.EnsembleRollout._score_lead(run, k, targets)
    names = [c[:2] for c in log]
    # every entry pushes once, from its source, the truth already there -- and only after the source has been scored
    for name, src in (("acc", "main"), ("gust", "view"), ("none", "main")):
      assert [c for c in log if c[:2] == (name, "window_push")] == [(name, "window_push", src, True)]
      assert names.index((name, "window_push")) > names.index((src, "score"))
    assert names.index(("gust", "window_push")) > names.index(("view", "derive"))
    for name, spec in (("acc", windows["acc"]), ("gust", windows["gust"][0]), ("none", windows["none"])):
      mine = [c[1:] for c in log if c[0] == name]
      if k in spec.leads(horizon):
        want = [("window_push", "main" if spec.source is None else "view", True), ("window_emit",), ("score", True)]
        if name == "gust":
          want.append(("event_score", True))
        assert mine == want + [("download", m) for m in range(M)], (name, k)
      else:
        assert [c[0] for c in mine] == ["window_push"], (name, k)
    assert not any(c[1] in ("window_reset", "window_set") for c in log)   # reset once per run, not per lead
  res = {k: v.result() for k, v in run.windows.items()}
  assert res["acc"].leads == [1, 3] and res["acc"].steps == 2 and len(res["acc"].scores) == len(res["acc"].members) == 2
  assert res["gust"].leads == [2, 3, 4] and len(res["gust"].events) == 3 and isinstance(res["gust"].events[0], EventScores)
  assert res["none"].leads == [] and res["none"].scores == [] and res["none"].members == []
  assert res["acc"].events is None and res["acc"].order is None
  assert len(res["acc"].members[0]) == M and res["acc"].members[0][2].shape == (G, B, C)
  assert isinstance(res["acc"].scores[0], EnsembleScores) and res["acc"].template is not None


def test_order_statistics_reach_the_windows_and_members_are_optional():
  log = []
  run = _run(2, {"acc": WindowSpec("sum", 2)}, log, order=[0.5], keep_members=False)
  assert ("acc", "order_set", (0.5,)) in log
  targets = _targets(2)
  for k in range(2):
    rollout.EnsembleRollout._score_lead(run, k, targets)
  mine = [c[1:] for c in log if c[0] == "acc" and c[1] not in ("reserve", "weight", "order_set", "window_set", "window_reset")]
  assert mine == [("window_push", "main", True), ("window_push", "main", True), ("window_emit",), ("score", True), ("order_score", True)]
  res = run.windows["acc"].result()
  assert res.members is None and len(res.order) == len(res.order_normalized) == 1
  assert isinstance(res.order[0], verification.OrderScores)


def test_without_windows_a_lead_makes_the_calls_it_made_before():
  with_log, without_log = [], []
  a, b = _run(3, {"acc": WindowSpec("sum", 2)}, with_log), _run(3, {}, without_log)
  del with_log[:], without_log[:]
  targets = _targets(3)
  for k in range(3):
    rollout.EnsembleRollout._score_lead(a, k, targets)
    rollout.EnsembleRollout._score_lead(b, k, targets)
  strip = lambda log: [c for c in log if c[0] in ("main", "view") and c[1] != "window_push"]
  assert [repr(c) for c in strip(with_log)] == [repr(c) for c in without_log]      # main and view: untouched by the windows
  assert not any(c[0] == "acc" for c in without_log) and b.windows == {}
  for k in range(3):
    assert a.scores[k].sums.tobytes() == b.scores[k].sums.tobytes()


def test_a_source_that_names_no_derived_entry_is_refused_before_anything_runs():
  er = rollout.EnsembleRollout.__new__(rollout.EnsembleRollout)
  er.world_size = 1
  with pytest.raises(ValueError, match="names no entry of `derived`"):
    er.run(None, None, None, 2, 3, windows={"gust": WindowSpec("max", 2, source="wind")})
  with pytest.raises(ValueError, match="names no entry of `derived`"):
    er.run(None, None, None, 2, 3, derived={"other": None}, windows={"gust": (WindowSpec("max", 2, source="wind"), None)})
  er.world_size = 2                                                      # more than one rank keeps raising
  with pytest.raises(ValueError, match="world_size == 1"):
    er.run(None, None, None, 2, 3, windows={"acc": WindowSpec("sum", 2)})


# ---- results ----------------------------------------------------------------------------------------------------------------
def _ens(seed=0):
  rng = np.random.default_rng(seed)
  return EnsembleScores(rng.uniform(1, 2, (B, C, 6)), rng.integers(0, 9, (B, C, M + 1)).astype(np.uint64), M)


def _events(seed=0):
  rng = np.random.default_rng(seed)
  t = rng.integers(0, 9, (1, B, C, 2, M + 1)).astype(np.uint64)
  return EventScores(t, t.copy(), M, [1], 0.5, np.zeros(1, np.uint64))


def _win(seed, leads=(1, 3), steps=2, events=True, members=None):
  n = len(leads)
  return rollout.WindowRolloutResult(leads, steps, [_ens(seed + i) for i in range(n)], [_ens(seed + 10 + i) for i in range(n)],
                                     [_events(seed + i) for i in range(n)] if events else None, members=members, template="t")


def test_window_results_merge_and_refuse_what_does_not_match():
  a, b = _win(0, members=[["m"], ["m"]]), _win(100)
  m = a.merge(b)
  assert m.leads == [1, 3] and m.steps == 2 and m.members is None and m.template == "t" and m.order is None
  for i in range(2):
    np.testing.assert_array_equal(m.scores[i].sums, a.scores[i].sums + b.scores[i].sums)
    np.testing.assert_array_equal(m.scores_normalized[i].rank_histogram, a.scores_normalized[i].rank_histogram + b.scores_normalized[i].rank_histogram)
    np.testing.assert_array_equal(m.events[i].weighted, a.events[i].weighted + b.events[i].weighted)
  with pytest.raises(ValueError, match="windows differ"):
    a.merge(_win(0, leads=(1, 2)))
  with pytest.raises(ValueError, match="windows differ"):
    a.merge(_win(0, steps=3))
  with pytest.raises(ValueError, match="events"):
    a.merge(_win(0, events=False))
  with pytest.raises(ValueError, match="one score per window"):
    rollout.WindowRolloutResult([1, 3], 2, [_ens()], [_ens()])
  empty = _win(0, leads=())
  assert empty.merge(_win(5, leads=())).scores == []

  def whole(windows):
    return rollout.EnsembleRolloutResult([_ens(k) for k in range(4)], n_members=M, windows=windows)

  r = whole({"acc": a, "gust": _win(7, leads=(2, 3), steps=3)})
  s = whole({"acc": b, "gust": _win(9, leads=(2, 3), steps=3)})
  rs = r.merge(s)
  assert sorted(rs.windows) == ["acc", "gust"]
  np.testing.assert_array_equal(rs.windows["acc"].scores[1].sums, a.scores[1].sums + b.scores[1].sums)
  np.testing.assert_array_equal(rs.windows["gust"].events[0].counts, r.windows["gust"].events[0].counts + s.windows["gust"].events[0].counts)
  plain = whole(None)
  assert plain.windows is None and plain.merge(plain).windows is None
  with pytest.raises(ValueError, match="carries windows"):
    r.merge(plain)
  with pytest.raises(ValueError, match="carries windows"):
    plain.merge(r)
  with pytest.raises(ValueError, match="window names differ"):
    r.merge(whole({"acc": b}))
  with pytest.raises(ValueError, match="windows differ"):
    r.merge(whole({"acc": b, "gust": _win(9, leads=(2, 4), steps=3)}))


def test_results_without_windows_are_what_they_were():
  """`windows=None` adds an attribute that is None and changes nothing else of a result or of its merge."""
  r = rollout.EnsembleRolloutResult([_ens(k) for k in range(2)], n_members=M, scores_normalized=[_ens(k + 5) for k in range(2)])
  m = r.merge(r)
  for k in range(2):
    assert m.scores[k].sums.tobytes() == (2 * r.scores[k].sums).tobytes()
    assert m.scores_normalized[k].rank_histogram.tobytes() == (2 * r.scores_normalized[k].rank_histogram).tobytes()
  others = {k: v for k, v in vars(m).items() if k not in ("scores", "scores_normalized", "n_members")}
  assert all(v is None for v in others.values()), others
