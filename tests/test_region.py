"""Regional ensemble scores, the host side: `RegionSpec` and its boxes, `RegionScores`, the calls a
`ScoredStore` and a rollout make on handles that record, the two ABI entries, and the yardstick's own check: over a partition
the reference sums of tests/region_reference.py add up to the global reference of tests/verification_reference.py."""
import ctypes

import numpy as np
import pytest

import gencast_flax_nnx_amd as pkg
from gencast_flax_nnx_amd import _lib, datasets, rollout, verification
from gencast_flax_nnx_amd.verification import EnsembleScores, RegionScores, RegionSpec
from tests import region_reference as R
from tests import verification_reference as VR
from tests.helpers import RecordingHandle


def _template(n_lat=13, n_lon=24, channels=1):
  lat, lon = np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)
  dims = ("batch", "time", "lat", "lon")
  return datasets.Dataset({f"v{i}": datasets.Variable(dims, np.zeros((1, 1, n_lat, n_lon), np.float32)) for i in range(channels)},
                          {"lat": lat, "lon": lon})


# ---- RegionSpec ---------------------------------------------------------------------------------------------------------------
def test_from_bounds_is_inclusive_and_wraps_through_zero():
  t = _template()                                                  # lat -90, -75, .., 90; lon 0, 15, .., 345
  lat, lon = t.coords["lat"], t.coords["lon"]
  spec = RegionSpec.from_bounds(t, {"tropics": dict(lat=(-15, 15)), "europe": dict(lat=(30, 75), lon=(-15, 45)),
                                    "east": dict(lon=(0, 180)), "all": dict(), "circle": dict(lon=(0, 360)),
                                    "dateline": dict(lat=(-90, 0), lon=(150, -150))})
  assert spec.names == ("tropics", "europe", "east", "all", "circle", "dateline") and spec.n_regions == 6
  m = spec.masks
  assert all(v.shape == (13, 24) and v.dtype == np.bool_ for v in m.values())
  np.testing.assert_array_equal(m["tropics"], np.repeat(((lat >= -15) & (lat <= 15))[:, None], 24, 1))
  assert m["tropics"].sum() == 3 * 24                              # -15, 0 and 15: both bounds belong
  # -15 is 345 after the modulo: 345, 0, 15, 30, 45 -- through 0 degrees, both bounds inclusive
  np.testing.assert_array_equal(lon[m["europe"][10]], [0.0, 15.0, 30.0, 45.0, 345.0])
  np.testing.assert_array_equal(lat[m["europe"].any(1)], [30.0, 45.0, 60.0, 75.0])
  np.testing.assert_array_equal(lon[m["east"][0]], np.arange(13) * 15.0)
  assert m["all"].all() and m["circle"].all()
  # a box over the date line: 150, 165, 180, 195, 210
  np.testing.assert_array_equal(lon[m["dateline"][0]], [150.0, 165.0, 180.0, 195.0, 210.0])
  assert not m["dateline"][7:].any() and m["dateline"][:7].any(1).all()
  with pytest.raises(ValueError, match="ascending"):
    RegionSpec.from_bounds(t, {"bad": dict(lat=(20, -20))})
  with pytest.raises(ValueError, match="'lat' and 'lon'"):
    RegionSpec.from_bounds(t, {"bad": dict(latitude=(0, 1))})


def test_masks_as_lat_lon_and_as_nodes_give_the_same_bits():
  t = _template()
  rng = np.random.default_rng(0)
  a, b = rng.random((13, 24)) < 0.5, rng.random((13, 24)) < 0.2
  two_d, flat = RegionSpec({"a": a, "b": b}), RegionSpec({"a": a.reshape(-1), "b": b.reshape(-1)})
  bits = two_d.node_bits(t)
  assert bits.dtype == np.uint32 and bits.shape == (312,)
  np.testing.assert_array_equal(bits, flat.node_bits(t))
  np.testing.assert_array_equal(bits, a.reshape(-1) * 1 + b.reshape(-1) * 2)     # node = lat_i * n_lon + lon_j
  assert bits[5 * 24 + 7] == int(a[5, 7]) + 2 * int(b[5, 7])
  # the masks are plain arrays: combined with a land-sea mask they make another spec
  land = rng.random((13, 24)) < 0.3
  both = RegionSpec({"a_land": two_d.masks["a"] & land, "a_sea": two_d.masks["a"] & ~land})
  np.testing.assert_array_equal(both.node_bits(t) != 0, a.reshape(-1))


def test_a_33rd_region_a_wrong_grid_and_a_wrong_mask_are_refused():
  t = _template()
  one = np.ones((13, 24), bool)
  RegionSpec({str(i): one for i in range(32)})
  with pytest.raises(ValueError, match="1..32"):
    RegionSpec({str(i): one for i in range(33)})
  with pytest.raises(ValueError, match="1..32"):
    RegionSpec({})
  with pytest.raises(ValueError, match="boolean"):
    RegionSpec({"a": np.ones((13, 24), np.float32)})
  with pytest.raises(ValueError, match="different sizes"):
    RegionSpec({"a": one, "b": np.ones(311, bool)})
  with pytest.raises(ValueError, match="does not fit"):
    RegionSpec({"a": one}).node_bits(_template(12, 26))             # 312 nodes too, but another grid
  with pytest.raises(ValueError, match="does not fit"):
    RegionSpec({"a": np.ones(100, bool)}).node_bits(t)
  with pytest.raises(ValueError, match="'lat' and 'lon'"):
    RegionSpec({"a": one}).node_bits(datasets.Dataset({"x": datasets.Variable(("batch",), np.zeros(2))}))


def test_bit_31_gives_a_uint32_above_two_to_the_31():
  t = _template()
  masks = {str(i): np.zeros(312, bool) for i in range(32)}
  masks["31"][7] = masks["0"][7] = True
  bits = RegionSpec(masks).node_bits(t)
  assert bits.dtype == np.uint32 and int(bits[7]) == 2 ** 31 + 1 and int(bits[7]) > 2 ** 31 and not bits[:7].any()


# ---- RegionScores ---------------------------------------------------------------------------------------------------------------
def _scores(rng, names=("a", "b", "c"), M=4, B=2, C=3):
  R_ = len(names)
  return RegionScores(names, rng.uniform(1, 2, (R_, B, C, 6)), rng.integers(0, 9, (R_, B, C, M + 1)).astype(np.uint64), M,
                      rng.integers(0, 5, R_).astype(np.uint64))


def test_a_region_is_an_ensemble_scores_and_merge_adds():
  rng = np.random.default_rng(1)
  x, y = _scores(rng), _scores(rng)
  assert len(x) == 3 and list(x) == ["a", "b", "c"] and [k for k, _ in x.items()] == ["a", "b", "c"]
  b = x["b"]
  assert isinstance(b, EnsembleScores) and b.n_members == 4
  np.testing.assert_array_equal(b.sums, x.sums[1])
  np.testing.assert_array_equal(b.rank_histogram, x.rank_histogram[1])
  np.testing.assert_array_equal(b.crps, (x.sums[1, ..., 4] - 0.5 * x.sums[1, ..., 5]) / x.sums[1, ..., 0])
  with pytest.raises(KeyError):
    x["nope"]
  m = RegionScores.merge([x, y])
  np.testing.assert_array_equal(m.sums, x.sums + y.sums)
  np.testing.assert_array_equal(m.rank_histogram, x.rank_histogram + y.rank_histogram)
  np.testing.assert_array_equal(m.invalid, x.invalid + y.invalid)
  assert m.names == x.names and m.n_members == 4
  np.testing.assert_array_equal(m["c"].sums, EnsembleScores.merge([x["c"], y["c"]]).sums)
  np.testing.assert_array_equal(RegionScores.merge([x]).sums, x.sums)
  with pytest.raises(ValueError, match="differ"):
    RegionScores.merge([x, _scores(rng, names=("a", "b", "d"))])
  with pytest.raises(ValueError, match="differ"):
    RegionScores.merge([x, _scores(rng, M=5)])
  with pytest.raises(ValueError, match="nothing"):
    RegionScores.merge([])
  with pytest.raises(ValueError, match="distinct"):
    _scores(rng, names=("a", "a", "b"))
  with pytest.raises(ValueError, match="sums must be"):
    RegionScores(("a",), np.zeros((2, 2, 3, 6)), np.zeros((2, 2, 3, 5)), 4)
  with pytest.raises(ValueError, match="hist must be"):
    RegionScores(("a",), np.zeros((1, 2, 3, 6)), np.zeros((1, 2, 3, 4)), 4)


def test_scaled_is_ensemble_scores_scaled_per_region_and_per_variable_splits_the_channels():
  rng = np.random.default_rng(2)
  x = _scores(rng)
  a = np.array([4.0, -1.0, 0.25])
  s = x.scaled(a)
  for name in x.names:
    want = x[name].scaled(a)
    np.testing.assert_array_equal(s[name].sums, want.sums)
    np.testing.assert_array_equal(s[name].rank_histogram, want.rank_histogram)
  np.testing.assert_array_equal(s.invalid, x.invalid)
  with pytest.raises(ValueError, match="channel_scale"):
    x.scaled(np.ones(4))
  pv = x.per_variable(_template(channels=3))
  assert sorted(pv) == ["a", "b", "c"] and sorted(pv["a"]["crps"]) == ["v0", "v1", "v2"]
  np.testing.assert_array_equal(pv["b"]["rmse"]["v1"], x["b"].rmse[:, 1:2])


def test_an_empty_region_gives_nan_scores_and_no_exception():
  x = RegionScores(("full", "empty"), np.stack([np.ones((2, 3, 6)), np.zeros((2, 3, 6))]),
                   np.stack([np.ones((2, 3, 5), np.uint64), np.zeros((2, 3, 5), np.uint64)]), 4, [0, 0])
  with np.errstate(invalid="ignore", divide="ignore"):
    e = x["empty"]
    for name in ("crps", "crps_ensemble", "rmse", "spread", "spread_skill_ratio", "bias"):
      assert np.isnan(getattr(e, name)).all(), name
    assert not e.valid_points.any() and not e.valid_weight.any()
    assert np.isfinite(x["full"].crps).all()
    assert np.isnan(x.scaled(np.ones(3))["empty"].crps).all()
    assert np.isnan(RegionScores.merge([x, x])["empty"].rmse).all()


# ---- ScoredStore and the rollout on handles that record -------------------------------------------------------------------------
G, B, C, M = 6, 1, 2, 3


class _Handle(RecordingHandle):
  """`RecordingHandle` with the two region calls: the plan's bits and R are logged, the results are filled with the number of
  the call as every other result of the class is."""

  def ens_region_set(self, node_bits, n_regions):
    self.R = int(n_regions)
    self._log("region_set", tuple(int(b) for b in node_bits), int(n_regions))

  def ens_region_score(self, truth):
    self._log("region_score", truth is None, full=(truth,))
    return (self._filled("region_score", (self.R, self.B, self.C, 6)),
            self._filled("region_score", (self.R, self.B, self.C, self.M + 1), np.uint64), np.full(self.R, 7, np.uint64))


def _handle(name, log):
  return _Handle(name, log, M=M, B=B, C=C, G=G, Q=0)


def _spec():
  return RegionSpec({"south": np.array([1, 1, 1, 0, 0, 0], bool), "east": np.array([0, 0, 1, 0, 0, 1], bool)})


BITS = (1, 1, 3, 0, 0, 2)


def _targets(horizon):
  dims = ("batch", "time", "lat", "lon")
  rng = np.random.default_rng(1)
  return datasets.Dataset({"a": datasets.Variable(dims, rng.standard_normal((B, horizon, 2, 3)).astype(np.float32)),
                           "b": datasets.Variable(dims, rng.standard_normal((B, horizon, 2, 3)).astype(np.float32))},
                          {"lat": np.array([-45.0, 45.0]), "lon": np.array([0.0, 120.0, 240.0])})


def test_scored_store_sets_the_plan_once_and_scores():
  log = []
  t = rollout.isel_time(_targets(1), slice(0, 1))
  spec = _spec()
  assert tuple(int(b) for b in spec.node_bits(t)) == BITS
  st = verification.ScoredStore(_handle("h", log), M, np.ones(G, np.float32), regions=spec, region_bits=spec.node_bits(t))
  st.setup()
  assert [c[1:] for c in log] == [("reserve", M), ("weight",), ("region_set", BITS, 2)]
  got = st.score_regions("truth")
  assert log[-1][1:] == ("region_score", False)
  assert isinstance(got, RegionScores) and got.names == ("south", "east") and got.n_members == M
  np.testing.assert_array_equal(got.invalid, [7, 7])
  np.testing.assert_array_equal(got["east"].sums, 1.0)
  st.score_regions(None)
  assert log[-1][1:] == ("region_score", True) and [c[1] for c in log].count("region_set") == 1
  # without regions no call is made on the handle
  log2 = []
  plain = verification.ScoredStore(_handle("p", log2), M, np.ones(G, np.float32))
  plain.setup()
  plain.configure()
  assert plain.score_regions(None) is None and plain.regions is None
  assert [c[1] for c in log2] == ["reserve", "weight"]
  # set per score: the plan is set again by every scoring call, not by setup
  log3 = []
  per = verification.ScoredStore(_handle("s", log3), M, np.ones(G, np.float32), regions=spec, region_bits=spec.node_bits(t),
                                 set_per_score=True)
  per.setup()
  assert [c[1] for c in log3] == ["reserve", "weight"]
  per.score_regions(None)
  per.score_regions(None)
  assert [c[1] for c in log3[2:]] == ["region_set", "region_score"] * 2
  with pytest.raises(ValueError, match="node bits"):
    verification.ScoredStore(_handle("x", []), M, np.ones(G, np.float32), regions=spec)


def _run(log, main_regions, view_regions, window_regions):
  """The state `EnsembleRollout._setup` would have made, on handles that record: a main store, one derived view "view" and
  one window "acc" over two lead times."""
  t = rollout.isel_time(_targets(1), slice(0, 1))
  args = lambda s: {} if s is None else {"regions": s, "region_bits": s.node_bits(t)}
  w = np.ones(G, np.float32)
  run = rollout._EnsembleRun()
  main, view = _handle("main", log), _handle("view", log)
  run.native, run.M, run.scale, run.loc, run.shape, run.normalized = main, M, np.ones(C), np.zeros(C), (G, B, C), False
  scale = np.array([2.0, 0.5])
  mstore = verification.ScoredStore(main, M, w, **args(main_regions))
  mstore.setup()
  run.main = rollout._StoreSeries(mstore, scale, None)
  run.scores = run.main.scores
  run.want_fields = run.want_spectra = False
  vstore = verification.ScoredStore(view, M, w, plan={"op": [0, 0]}, source=main, **args(view_regions))
  vstore.setup()
  run.views["view"] = rollout._StoreSeries(vstore, np.ones(C), None)
  wstore = verification.ScoredStore(_handle("acc", log), M, w, **args(window_regions))
  run.windows["acc"] = rollout._WindowEntry(verification.WindowSpec("sum", 2), rollout._StoreSeries(wstore, np.ones(C), t), main, 2)
  run.windows["acc"].start()
  return run, scale


def test_a_rollout_scores_the_regions_after_the_other_scorers_at_every_lead():
  log = []
  run, scale = _run(log, _spec(), None, _spec())
  sets = [c for c in log if c[1] == "region_set"]
  assert sets == [("main", "region_set", BITS, 2), ("acc", "region_set", BITS, 2)]        # once per store, before the first lead
  targets = _targets(2)
  for k in range(2):
    del log[:]
    rollout.EnsembleRollout._score_lead(run, k, targets)
    assert [c[1:] for c in log if c[0] == "main" and c[1] in ("score", "region_score")] == [("score", False), ("region_score", True)]
    assert not any(c[1] in ("region_set", "region_score") for c in log if c[0] == "view")
    acc = [c[1:] for c in log if c[0] == "acc"]
    assert acc == ([("window_push", "main", True)] if k == 0 else
                   [("window_push", "main", True), ("window_emit",), ("score", True), ("region_score", True)])
  main = run.main
  assert len(main.regions) == len(main.raw_regions) == 2
  np.testing.assert_array_equal(main.raw_regions[1].sums, 2.0)                            # in the order of the calls
  for r, name in enumerate(("south", "east")):                                            # physical = `scaled` of the raw
    np.testing.assert_array_equal(main.regions[0][name].sums, main.raw_regions[0][name].scaled(scale).sums)
  d = run.views["view"].derived_result()
  assert d.regions is None and "regions" not in vars(d) and "regions_normalized" not in vars(d)
  w = run.windows["acc"].result()
  assert len(w.regions) == len(w.regions_normalized) == 1 and isinstance(w.regions[0], RegionScores)
  res = rollout.EnsembleRolloutResult(main.scores, n_members=M, scores_normalized=main.raw, regions=main.regions,
                                      regions_normalized=main.raw_regions)
  assert res.regions[1]["east"].n_members == M
  both = res.merge(res)
  np.testing.assert_array_equal(both.regions_normalized[0].sums, 2 * main.raw_regions[0].sums)
  np.testing.assert_array_equal(both.regions[1].invalid, [14, 14])


def test_regions_exist_on_a_result_only_when_they_were_asked_for():
  with_log, without_log = [], []
  a, _ = _run(with_log, None, None, None)
  b, _ = _run(without_log, None, None, None)
  assert with_log == without_log and not any("region" in c[1] for c in with_log)
  targets = _targets(2)
  for k in range(2):
    rollout.EnsembleRollout._score_lead(a, k, targets)
  assert not any("region" in c[1] for c in with_log)
  assert a.main.regions is None and a.main.raw_regions is None
  rng = np.random.default_rng(0)
  ens = lambda: EnsembleScores(rng.uniform(1, 2, (B, C, 6)), rng.integers(0, 9, (B, C, M + 1)).astype(np.uint64), M)
  without = rollout.EnsembleRolloutResult([ens() for _ in range(2)], n_members=M)
  assert without.regions is None and without.regions_normalized is None
  assert "regions" not in vars(without) and "regions_normalized" not in vars(without)
  assert sorted(vars(without)) == sorted(["scores", "scores_normalized", "spectra", "spectra_normalized", "events", "order",
                                          "order_normalized", "climatology", "climatology_normalized", "derived", "windows",
                                          "mean", "variance", "members", "quantiles", "n_members"])
  assert "regions" not in vars(without.merge(without))
  rs = [_scores(rng, names=("south", "east"), M=M, B=B, C=C) for _ in range(2)]
  with_r = rollout.EnsembleRolloutResult([ens() for _ in range(2)], n_members=M, regions=rs, regions_normalized=rs)
  with pytest.raises(ValueError, match="region scores"):
    with_r.merge(without)
  with pytest.raises(ValueError, match="lead times"):
    rollout.EnsembleRolloutResult([ens()], n_members=M, regions=rs, regions_normalized=rs)
  for cls, lead in ((rollout.DerivedRolloutResult, ()), (rollout.WindowRolloutResult, ([1, 3], 2))):
    plain = cls(*lead, [ens() for _ in range(2)], [ens() for _ in range(2)])
    assert plain.regions is None and "regions" not in vars(plain)
    part = cls(*lead, [ens() for _ in range(2)], [ens() for _ in range(2)], regions=rs, regions_normalized=rs)
    np.testing.assert_array_equal(part.merge(part).regions[1].sums, 2 * rs[1].sums)


def test_rollout_refuses_a_regions_key_that_names_no_store():
  from gencast_flax_nnx_amd import synthetic
  lat, lon = np.linspace(-90, 90, 5), np.arange(8) * 45.0
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  spec = RegionSpec.from_bounds(tgt, {"tropics": dict(lat=(-45, 45))})
  runner = rollout.EnsembleRollout(model=None)                    # (the check comes before anything touches the model)
  with pytest.raises(ValueError, match="nope"):
    runner.run(inp, tgt, frc, 1, 3, regions={None: spec, "nope": spec})
  with pytest.raises(ValueError, match="wind"):
    runner.run(inp, tgt, frc, 1, 3, regions={"wind": spec}, windows=None, derived=None)


def test_sampler_refuses_more_than_one_rank_and_the_wrappers_pass_regions_through():
  from gencast_flax_nnx_amd import NaNCleaner, config, ensemble, synthetic

  class _S:
    _denoiser = None
  with pytest.raises(ValueError, match="one rank"):
    ensemble.EnsembleSampler(_S(), rank=0, world_size=2).regions(None, None, None, 4, _spec())
  lat, lon = np.linspace(-90, 90, 5), np.arange(8) * 45.0
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  rng = np.random.default_rng(1)
  raw = _scores(rng, names=("south", "east"), M=4, B=1, C=82)
  seen = {}

  class _Predictor:
    def ensemble_regions(self, inputs, targets, forcings=None, **kwargs):
      seen.update(inputs=inputs, targets=targets, kwargs=kwargs)
      return raw

  def stats(v):
    names = set(config.TASK.input_variables) | set(config.TASK.target_variables) | set(frc.keys())
    return datasets.Dataset({n: (datasets.Variable(("level",), np.full(13, v, np.float32)) if n in config.ALL_ATMOSPHERIC_VARS
                                 else datasets.Variable((), np.float32(v))) for n in names})
  norm = rollout.InputsAndResiduals(_Predictor(), stats(2.0), stats(0.5), stats(0.25))
  spec = RegionSpec.from_bounds(tgt, {"south": dict(lat=(-90, 0)), "east": dict(lon=(0, 180))})
  got = norm.ensemble_regions(inp, tgt, frc, num_members=4, spec=spec)
  assert seen["kwargs"] == {"num_members": 4, "spec": spec}
  k = "2m_temperature"
  np.testing.assert_array_equal(seen["targets"][k].data, (tgt[k].data - inp[k].data[:, -1:]) / np.float32(0.25))
  want = raw.scaled(np.full(82, 0.25))                             # every target is a residual variable: scale 0.25
  np.testing.assert_array_equal(got.sums, want.sums)
  np.testing.assert_array_equal(got.invalid, raw.invalid)
  dirty_in = datasets.Dataset({n: datasets.Variable(v.dims, np.array(v.data, copy=True)) for n, v in inp.items()}, inp.coords)
  dirty_tg = datasets.Dataset({n: datasets.Variable(v.dims, np.array(v.data, copy=True)) for n, v in tgt.items()}, tgt.coords)
  dirty_in[k].data[..., 0, 0] = np.nan
  dirty_tg[k].data[..., 1, 1] = np.nan
  stack = NaNCleaner(norm, k, datasets.Dataset({k: datasets.Variable((), np.float32(0))}))
  again = stack.ensemble_regions(dirty_in, dirty_tg, frc, num_members=4, spec=spec)
  np.testing.assert_array_equal(again.sums, got.sums)
  assert not np.isnan(seen["inputs"][k].data).any() and np.isnan(seen["targets"][k].data).any()


# ---- the ABI and the binding -----------------------------------------------------------------------------------------------------
def test_the_two_entries_are_declared_bound_and_exported():
  u32, u64, f64 = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double)
  f32 = ctypes.POINTER(ctypes.c_float)
  assert _lib.SIGNATURES["gc_ens_region_set"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, u32])
  assert _lib.SIGNATURES["gc_ens_region_score"] == (ctypes.c_int, [ctypes.c_void_p, f32, f64, u64, u64])
  lib = _lib.load_library()
  assert lib.gc_ens_region_set.argtypes == [ctypes.c_void_p, ctypes.c_int32, u32] and lib.gc_ens_region_score.restype is ctypes.c_int
  assert pkg.RegionSpec is RegionSpec and pkg.RegionScores is RegionScores
  assert "RegionSpec" in pkg.__all__ and "RegionScores" in pkg.__all__


def test_the_binding_checks_its_arguments_before_the_call():
  class _Cfg:
    batch, c_out = 2, 3
  nd = _lib.NativeDenoiser.__new__(_lib.NativeDenoiser)
  nd.cfg, nd.num_grid_nodes, nd._regions, nd._ens_members = _Cfg(), 6, 0, 0
  with pytest.raises(ValueError, match="1..32"):
    nd.ens_region_set(np.zeros(6, np.uint32), 33)
  with pytest.raises(ValueError, match="1..32"):
    nd.ens_region_set(np.zeros(6, np.uint32), 0)
  with pytest.raises(ValueError, match="shape"):
    nd.ens_region_set(np.zeros(5, np.uint32), 2)
  with pytest.raises(ValueError, match="below 2\\^2"):
    nd.ens_region_set(np.array([0, 1, 2, 3, 4, 0], np.uint32), 2)
  with pytest.raises(ValueError, match="unsigned integers"):
    nd.ens_region_set(np.zeros(6, np.float32), 2)
  with pytest.raises(_lib.GencastHipError, match="ens_region_set"):
    nd.ens_region_score(None)
  nd._regions = 2
  with pytest.raises(_lib.GencastHipError, match="ens_reserve"):
    nd.ens_region_score(None)


# ---- the yardstick's own check ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [3, 8])
def test_over_a_partition_the_reference_sums_add_up_to_the_global_reference(M):
  """S0 (dyadic weights) and the histograms bit for bit; the other sums are float64 sums of non-dyadic terms taken in a
  different order, so they agree within the two bounds added, not bit for bit."""
  G_, B_, C_ = 312, 2, 4
  rng = np.random.default_rng(M)
  scale = np.logspace(-2, 3, C_)
  members = (rng.standard_normal((M, G_, B_, C_)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G_, B_, C_)) * scale).astype(np.float32)
  w = (np.arange(G_) % 7 + 1).astype(np.float32) / 8.0
  truth[[3, 150, 300]] = np.nan
  members[1, 40:44] = members[0, 40:44]
  members[M // 2, 9, 1, 2] = np.nan
  members[0, 120, 0, 1] = np.inf
  bits = (np.uint32(1) << rng.integers(0, 4, G_).astype(np.uint32)).astype(np.uint32)      # every node in exactly one of 4
  ref = R.reference(members, truth, w, bits, 4)
  whole = VR.reference(members, truth, w)
  assert ref["sums"].shape == (4, B_, C_, 6) and ref["hist"].shape == (4, B_, C_, M + 1) and ref["invalid"].shape == (4,)
  np.testing.assert_array_equal(ref["hist"].sum(0), whole["hist"])
  assert int(ref["invalid"].sum()) == whole["invalid"] == 3 * B_ * C_ + 2
  assert ref["sums"][..., 0].sum(0).tobytes() == whole["sums"][..., 0].tobytes()
  err = np.abs(ref["sums"].sum(0) - whole["sums"])
  bound = R.sum_tolerance(ref, G_, M).sum(0) + VR.sum_tolerance(whole, G_, M)
  assert np.all(err <= bound)
  # a node with no bit is in no region, an empty region is zeros, and overlap counts a node in each of its regions
  bits2 = bits.copy()
  bits2[:100] = 0
  bits2[200:] |= np.uint32(16)
  ref2 = R.reference(members, truth, w, bits2, 6)
  assert not ref2["sums"][5].any() and not ref2["hist"][5].any() and ref2["invalid"][5] == 0
  np.testing.assert_array_equal(ref2["hist"][4], VR.reference(members[:, 200:], truth[200:], w[200:])["hist"])
  assert int(ref2["invalid"][:4].sum()) == int((~(np.isfinite(truth[100:]) & np.isfinite(members[:, 100:]).all(0))).sum())
