"""Multivariate ensemble scores without a device: the float64 reference of
tests/multivar_reference.py against closed forms, the host formulas of `verification.EnergyScores` / `VariogramScores`
(merge, scaled, per_variable), the specs' validation, the binding's own checks and `ScoredStore(energy=, variogram=)`."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, datasets, verification
from gencast_flax_nnx_amd.verification import EnergyScores, EnergySpec, VariogramScores, VariogramSpec
from tests import multivar_reference as R

N_LAT, N_LON = 5, 8
G = N_LAT * N_LON


def _random(M, B, C, seed):
  rng = np.random.default_rng(seed)
  members = rng.standard_normal((M, G, B, C)).astype(np.float32)
  truth = rng.standard_normal((G, B, C)).astype(np.float32)
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  return members, truth, w


# ---- the reference against closed forms ---------------------------------------------------------------------------------------
def test_reference_energy_of_constant_fields_is_exact():
  M, B, C = 4, 2, 3
  c = np.array([0.5, -1.25, 3.0, 0.0, 2.5])                       # the M members, then the truth: dyadic
  members = np.broadcast_to(c[:M, None, None, None], (M, G, B, C)).astype(np.float32).copy()
  truth = np.full((G, B, C), c[M], np.float32)
  w = (np.arange(G) % 4 + 1).astype(np.float32) / 4.0
  group, scale = np.array([0, 1, 0]), np.array([2.0, 0.5, 1.0])
  ref = R.energy(members, truth, w, group, scale)
  s0 = np.array([w.sum() * 3.0, w.sum() * 0.5])
  np.testing.assert_array_equal(ref["s0"], np.broadcast_to(s0, (B, 2)))
  for p, (i, j) in enumerate(R.pairs(M)):
    assert R.pair_index(i, j) == p
    np.testing.assert_array_equal(ref["d2"][:, :, p], np.broadcast_to(s0 * (c[i] - c[j]) ** 2, (B, 2)))
  assert ref["invalid"] == 0 and list(ref["n"]) == [2 * G, G]
  # an invalid point leaves the sums of its group and nothing else; a channel in no group is not counted
  truth[3, 1, 0] = np.nan
  members[1, 4, 0, 1] = np.inf
  cut = R.energy(members, truth, w, group, scale)
  assert cut["invalid"] == 2
  np.testing.assert_array_equal(cut["s0"], [[s0[0], s0[1] - 0.5 * w[4]], [s0[0] - 2.0 * w[3], s0[1]]])
  assert R.energy(members, truth, w, np.array([0, -1, 0]), scale)["invalid"] == 1
  # D = |c_i - c_j| for every pair, so the scores are those of the scalar ensemble
  sc = R.energy_scores(ref["d2"], ref["s0"], M)
  err = np.mean(np.abs(c[:M] - c[M]))
  pair = np.mean([abs(c[i] - c[j]) for j in range(M) for i in range(j)])
  np.testing.assert_allclose(sc["fair"], err - 0.5 * pair, rtol=1e-14)
  np.testing.assert_allclose(sc["ensemble"], err - 0.5 * (M - 1) / M * pair, rtol=1e-14)


def test_reference_variogram_of_a_field_linear_in_longitude():
  M, B, C = 3, 1, 2
  slope = np.array([0.5, 1.0, 2.0, 0.25])                         # the members, then the truth
  lon = np.tile(np.arange(N_LON, dtype=np.float64), N_LAT)
  fields = (slope[:, None] * lon[None, :]).astype(np.float32)[:, :, None, None] * np.ones((1, 1, B, C), np.float32)
  members, truth = fields[:M].copy(), fields[M].copy()
  w = np.ones(G, np.float32)
  offsets = [(0, 1), (1, 0), (0, -2), (N_LAT - 1, 3)]
  for p in (0.5, 1.0, 2.0):
    ref = R.variogram(members, truth, w, N_LAT, N_LON, offsets, p)
    for o, (di, dj) in enumerate(offsets):
      rows = N_LAT - abs(di)
      assert np.all(ref["counts"][:, :, o] == rows * N_LON)
      np.testing.assert_array_equal(ref["sums"][0, :, :, o], float(rows * N_LON))
      # |dj| columns of a row pair across the seam, at a distance of n_lon - |dj| columns; the others at |dj|
      near, far = N_LON - abs(dj), abs(dj)
      v = lambda s: (near * (abs(s) * abs(dj)) ** p + far * (abs(s) * (N_LON - abs(dj))) ** p) * rows   # noqa: E731
      vx, vy = np.mean([v(s) for s in slope[:M]]), v(slope[M])
      np.testing.assert_allclose(ref["sums"][2, :, :, o], vx, rtol=1e-13, atol=0.0)
      np.testing.assert_allclose(ref["sums"][3, :, :, o], vy, rtol=1e-13, atol=0.0)
    sc = VariogramScores(ref["sums"], ref["counts"], M, offsets, p)
    assert np.all(sc.ensemble_variogram[..., 1] == 0.0) and np.all(sc.variogram_score[..., 1] == 0.0)   # (1, 0): no difference
    with np.errstate(invalid="ignore"):                           # (0 / 0 at the offset without a difference)
      np.testing.assert_allclose(sc.roughness_ratio[..., 0], np.mean(slope[:M] ** p) / slope[M] ** p, rtol=1e-13)
  # a pair with an invalid end leaves every sum of its column and offset, and nothing else
  truth[0, 0, 1] = np.nan                                         # node (0, 0)
  cut = R.variogram(members, truth, w, N_LAT, N_LON, offsets, 1.0)
  full = R.variogram(members, np.where(np.isnan(truth), 0, truth), w, N_LAT, N_LON, offsets, 1.0)
  np.testing.assert_array_equal(cut["counts"][0, 0], full["counts"][0, 0])
  np.testing.assert_array_equal(full["counts"][0, 1] - cut["counts"][0, 1], [2, 1, 2, 1])


# ---- host formulas --------------------------------------------------------------------------------------------------------------
def test_energy_scores_from_sums_merge_and_names():
  M, B, C = 5, 2, 4
  members, truth, w = _random(M, B, C, seed=3)
  group, scale = np.array([0, 0, 1, -1]), np.array([1.0, 2.0, 0.5, 1.0])
  ref = R.energy(members, truth, w, group, scale)
  want = R.energy_scores(ref["d2"], ref["s0"], M)
  sc = EnergyScores.from_sums(ref["d2"], ref["s0"], M, ("uv", "z"), invalid=3)
  np.testing.assert_allclose(sc.err, want["err"], rtol=1e-14)
  np.testing.assert_allclose(sc.pair, want["pair"], rtol=1e-14)
  np.testing.assert_allclose(sc.per_forecast, want["fair"], rtol=1e-14)
  np.testing.assert_allclose(sc.per_forecast_ensemble, want["ensemble"], rtol=1e-14)
  np.testing.assert_allclose(sc.energy_score, want["fair"].mean(axis=0), rtol=1e-14)
  assert sc.n_forecasts == B and sc.names == ("uv", "z") and sc.invalid == 3
  assert set(sc.per_group()) == {"energy_score", "energy_score_ensemble", "error_term", "pair_term"}
  assert sc.per_group()["energy_score"]["z"] == sc.energy_score[1]
  # a single-channel group at one point: the energy score is the CRPS of the scalar ensemble
  one = R.energy(members[:, :1], truth[:1], w[:1], np.array([-1, -1, 0, -1]), np.ones(C))
  got = EnergyScores.from_sums(one["d2"], one["s0"], M)
  x, y = members[:, 0, :, 2].astype(np.float64), truth[0, :, 2].astype(np.float64)
  crps = np.abs(x - y).mean(axis=0) - 0.5 * np.mean([np.abs(x[i] - x[j]) for j in range(M) for i in range(j)], axis=0)
  np.testing.assert_allclose(got.per_forecast[:, 0], crps, rtol=1e-12)
  # merge: the forecasts of the parts, one after the other; the scores are means over all of them
  other = EnergyScores(sc.err * 2.0, sc.pair * 3.0, M, ("uv", "z"), invalid=1)
  both = EnergyScores.merge([sc, other])
  assert both.n_forecasts == 2 * B and both.invalid == 4
  np.testing.assert_array_equal(both.err, np.concatenate([sc.err, other.err]))
  np.testing.assert_allclose(both.energy_score, 0.5 * (sc.energy_score + other.energy_score), rtol=1e-14)
  for bad in (EnergyScores(sc.err, sc.pair, M + 1, ("uv", "z")), EnergyScores(sc.err, sc.pair, M, ("a", "b"))):
    with pytest.raises(ValueError, match="merge"):
      EnergyScores.merge([sc, bad])
  with pytest.raises(ValueError, match="merge"):
    EnergyScores.merge([])
  # a group without a valid point is NaN, without a warning
  import warnings
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    empty = EnergyScores.from_sums(np.zeros((1, 2, 3)), np.array([[0.0, 1.0]]), 2)
  assert np.isnan(empty.energy_score[0]) and empty.energy_score[1] == 0.0
  for args in ((ref["d2"], ref["s0"], M + 1), (ref["d2"], ref["s0"][:, :1], M), (ref["d2"][0], ref["s0"], M)):
    with pytest.raises(ValueError):
      EnergyScores.from_sums(*args)
  with pytest.raises(ValueError):
    EnergyScores(sc.err, sc.pair, 1)
  with pytest.raises(ValueError):
    EnergyScores(sc.err, sc.pair, M, ("one",))
  assert EnergyScores.pair_index(0, 1) == 0 and EnergyScores.pair_index(2, 4) == 8
  with pytest.raises(ValueError):
    EnergyScores.pair_index(2, 2)


def test_variogram_scores_scaled_merge_and_per_variable():
  M, B, C = 4, 2, 3
  members, truth, w = _random(M, B, C, seed=5)
  offsets = [(0, 1), (2, -3)]
  a = np.array([0.5, -4.0, 1024.0])                               # powers of two: the scaled inputs are exact
  af = a.astype(np.float32)
  for p in (0.5, 1.0, 2.0):
    base = R.variogram(members, truth, w, N_LAT, N_LON, offsets, p)
    moved = R.variogram(members * af, truth * af, w, N_LAT, N_LON, offsets, p)
    sc = VariogramScores(base["sums"], base["counts"], M, offsets, p)
    got = sc.scaled(a)
    np.testing.assert_allclose(got.sums, moved["sums"], rtol=1e-12, atol=0.0)
    np.testing.assert_array_equal(got.counts, moved["counts"])
    np.testing.assert_allclose(got.variogram_score, sc.variogram_score * (np.abs(a) ** (2 * p))[None, :, None], rtol=1e-12)
    np.testing.assert_allclose(got.roughness_ratio, sc.roughness_ratio, rtol=1e-12)
    np.testing.assert_allclose(sc.variogram_score, base["sums"][1] / base["sums"][0])
    np.testing.assert_allclose(sc.ensemble_variogram, base["sums"][2] / base["sums"][0])
    np.testing.assert_allclose(sc.truth_variogram, base["sums"][3] / base["sums"][0])
    np.testing.assert_array_equal(sc.valid_pairs, base["counts"])
  for bad in ([1.0, 2.0], [1.0, 0.0, 1.0], [1.0, np.nan, 1.0]):
    with pytest.raises(ValueError):
      sc.scaled(bad)
  other = VariogramScores(2.0 * sc.sums, sc.counts + np.uint64(1), M, offsets, 2.0)
  both = VariogramScores.merge([sc, other])
  np.testing.assert_array_equal(both.sums, 3.0 * sc.sums)
  np.testing.assert_array_equal(both.counts, 2 * sc.counts + np.uint64(1))
  for bad in (VariogramScores(sc.sums, sc.counts, M + 1, offsets, 2.0), VariogramScores(sc.sums, sc.counts, M, offsets, 1.0),
              VariogramScores(sc.sums, sc.counts, M, offsets[::-1], 2.0)):
    with pytest.raises(ValueError, match="merge"):
      VariogramScores.merge([sc, bad])
  with pytest.raises(ValueError):
    VariogramScores(sc.sums[:3], sc.counts, M, offsets, 2.0)
  with pytest.raises(ValueError):
    VariogramScores(sc.sums, sc.counts[..., :1], M, offsets, 2.0)
  dims = ("batch", "time", "level", "lat", "lon")
  template = datasets.Dataset({"a": datasets.Variable(dims, np.zeros((2, 1, 2, N_LAT, N_LON), np.float32)),
                               "b": datasets.Variable(("batch", "time", "lat", "lon"), np.zeros((2, 1, N_LAT, N_LON), np.float32))},
                              {"lat": np.linspace(-90, 90, N_LAT), "lon": np.arange(N_LON) * 45.0, "level": np.array([500, 850])})
  out = sc.per_variable(template)
  assert out["variogram_score"]["a"].shape == (2, 2, 2) and out["roughness_ratio"]["b"].shape == (2, 1, 2)
  np.testing.assert_array_equal(out["valid_pairs"]["b"], sc.counts[:, 2:3])
  with pytest.raises(ValueError, match="channels"):
    sc.per_variable(datasets.Dataset({"b": template["b"]}, template.coords))


# ---- the specs ------------------------------------------------------------------------------------------------------------------
def _template():
  dims = ("batch", "time", "level", "lat", "lon")
  flat = ("batch", "time", "lat", "lon")
  z2 = np.zeros((2, 1, N_LAT, N_LON), np.float32)
  return datasets.Dataset({"z": datasets.Variable(dims, np.zeros((2, 1, 3, N_LAT, N_LON), np.float32)),
                           "u10": datasets.Variable(flat, z2), "v10": datasets.Variable(flat, z2),
                           "t2m": datasets.Variable(flat, z2)},
                          {"lat": np.linspace(-90, 90, N_LAT), "lon": np.arange(N_LON) * 45.0, "level": np.array([300, 500, 850])})


def test_energy_spec_maps_names_to_channels():
  template = _template()
  layout = {name: (off, n) for name, off, n in datasets.channel_layout(template)}
  spec = EnergySpec({"wind10": ["u10", "v10"], "z": ["z"]}, weights={"z": [1.0, 2.0, 4.0], "u10": 0.5})
  plan = spec.plan(template)
  assert plan["n_groups"] == 2 and plan["names"] == ("wind10", "z") and spec.names == ("wind10", "z")
  group, scale = plan["group"], plan["scale"]
  assert group.dtype == np.int32 and scale.dtype == np.float64 and group.shape == scale.shape == (6,)
  for name, k in (("u10", 0), ("v10", 0), ("z", 1), ("t2m", -1)):
    off, n = layout[name]
    assert np.all(group[off:off + n] == k), name
  off, n = layout["z"]
  np.testing.assert_array_equal(scale[off:off + n], [1.0, 2.0, 4.0])
  assert scale[layout["u10"][0]] == 0.5 and scale[layout["v10"][0]] == 1.0
  with pytest.raises(ValueError, match="not a target variable"):
    EnergySpec({"g": ["nope"]}).plan(template)
  with pytest.raises(ValueError, match="scalar or have 3"):
    EnergySpec({"g": ["z"]}, weights={"z": [1.0, 2.0]}).plan(template)
  for bad in (dict(groups={}), dict(groups={"g": []}), dict(groups={"a": ["u10"], "b": ["u10"]}),
              dict(groups={str(k): [f"v{k}"] for k in range(33)}), dict(groups={"g": ["z"]}, weights={"t2m": 1.0}),
              dict(groups={"g": ["z"]}, weights={"z": 0.0}), dict(groups={"g": ["z"]}, weights={"z": np.nan})):
    with pytest.raises(ValueError):
      EnergySpec(**bad)


def test_variogram_spec_checks_offsets_and_order():
  spec = VariogramSpec([(0, 1), (1, 0), (0, 4), (4, 0)], p=0.5)
  plan = spec.plan(_template())
  assert (plan["n_lat"], plan["n_lon"], plan["p"]) == (N_LAT, N_LON, 0.5)
  assert plan["offsets"].dtype == np.int32 and plan["offsets"].tolist() == [[0, 1], [1, 0], [0, 4], [4, 0]]
  assert VariogramSpec([(0, 1)]).p == 0.5
  for bad in ([], [(0, 0)], [(0, 1, 2)], [(0.5, 1)], [(0, 1)] * 17):
    with pytest.raises(ValueError):
      VariogramSpec(bad)
  for p in (0.25, 3, np.nan):
    with pytest.raises(ValueError):
      VariogramSpec([(0, 1)], p=p)
  for bad in ([(N_LAT, 0)], [(0, -N_LON)]):
    with pytest.raises(ValueError, match="beyond"):
      VariogramSpec(bad).plan(_template())
  with pytest.raises(ValueError, match="lat"):
    VariogramSpec([(0, 1)]).plan(datasets.Dataset({"x": datasets.Variable(("batch",), np.zeros(2, np.float32))}, {}))


# ---- the ABI and the binding's own checks: before the C call, so without a device -----------------------------------------------
def test_the_entries_are_declared_exported_and_bound():
  import gencast_flax_nnx_amd as pkg
  lib = _lib.load_library()
  for name in ("gc_ens_energy_set", "gc_ens_energy_score", "gc_ens_variogram_set", "gc_ens_variogram_score"):
    assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert hasattr(_lib.NativeDenoiser, name[3:])
  for name in ("EnergySpec", "EnergyScores", "VariogramSpec", "VariogramScores"):
    assert getattr(pkg, name) is getattr(verification, name) and name in pkg.__all__
  assert lib.gc_abi_version() == 1 and lib.gc_num_kernel_classes() == 13


class _NoCall:
  def __getattr__(self, name):
    raise AssertionError(f"{name} must not be reached")


def _bare_binding():
  nd = object.__new__(_lib.NativeDenoiser)
  nd._lib, nd._h = _NoCall(), None
  nd.cfg = _lib.GcConfig(128, 128, 2, 256, 1, 10, 6, 2, 32, 32, 16.0)
  nd.num_grid_nodes, nd._ens_members, nd._energy_groups, nd._variogram_offsets = 312, 0, None, None
  return nd


def test_binding_rejects_bad_plans_before_the_c_call():
  nd = _bare_binding()
  group, scale = np.array([0, 0, 1, 1, 1, -1]), np.ones(6)
  for K, g, a in ((0, group, scale), (33, group, scale), (3, group, scale), (2, group[:5], scale[:5]), (2, group, scale[:5]),
                  (2, np.array([0, 0, 1, 1, 2, -1]), scale), (2, np.array([0, 0, 1, 1, -2, -1]), scale),
                  (2, group, np.array([1, 1, 0, 1, 1, 1.0])), (2, group, np.array([1, 1, np.inf, 1, 1, 1.0]))):
    with pytest.raises(ValueError):
      nd.ens_energy_set(K, g, a)
  for n_lat, n_lon, o, p in ((13, 24, [(0, 0)], 0.5), (13, 24, [(13, 0)], 0.5), (13, 24, [(0, -24)], 0.5), (13, 24, [(0, 1)], 0.75),
                             (13, 25, [(0, 1)], 0.5), (13, 24, [(0, 1)] * 17, 0.5), (13, 24, [], 0.5), (13, 24, [0, 1], 0.5)):
    with pytest.raises(ValueError):
      nd.ens_variogram_set(n_lat, n_lon, o, p)
  with pytest.raises(_lib.GencastHipError, match="ens_energy_set"):
    nd.ens_energy_score(None)
  with pytest.raises(_lib.GencastHipError, match="ens_variogram_set"):
    nd.ens_variogram_score(None)
  nd._energy_groups, nd._variogram_offsets = 2, 4
  for call in (nd.ens_energy_score, nd.ens_variogram_score):
    with pytest.raises(_lib.GencastHipError, match="ens_reserve"):
      call(None)
  nd._ens_members = 8
  for call in (nd.ens_energy_score, nd.ens_variogram_score):
    with pytest.raises(ValueError, match="truth must be"):
      call(np.zeros((312, 2, 5), np.float32))


# ---- ScoredStore(energy=, variogram=) with a handle that records ----------------------------------------------------------------
class _Handle:
  def __init__(self, M, B=2, K=2, C=3, O=2):
    self.calls, self.M, self.B, self.K, self.C, self.O = [], M, B, K, C, O

  def ens_reserve(self, n):
    self.calls.append(("reserve", n))

  def ens_set_node_weight(self, w):
    self.calls.append(("weight",))

  def ens_energy_set(self, K, group, scale):
    self.calls.append(("energy_set", K, tuple(group), tuple(scale)))

  def ens_variogram_set(self, n_lat, n_lon, offsets, p):
    self.calls.append(("variogram_set", n_lat, n_lon, np.asarray(offsets).tolist(), p))

  def ens_energy_score(self, truth):
    self.calls.append(("energy_score", truth is None))
    return np.ones((self.B, self.K, self.M * (self.M + 1) // 2)), np.full((self.B, self.K), 4.0), 7

  def ens_variogram_score(self, truth):
    self.calls.append(("variogram_score", truth is None))
    return np.ones((4, self.B, self.C, self.O)), np.full((self.B, self.C, self.O), 5, np.uint64)


def test_scored_store_sets_the_plans_and_scores():
  eplan = {"n_groups": 2, "group": np.array([0, 1, -1], np.int32), "scale": np.ones(3), "names": ("a", "b")}
  vplan = VariogramSpec([(0, 1), (1, 0)], 2.0).grid_plan(4, 6)
  h = _Handle(4)
  st = verification.ScoredStore(h, 4, np.ones(4, np.float32), energy=eplan, variogram=vplan)
  st.setup()
  assert h.calls == [("reserve", 4), ("weight",), ("energy_set", 2, (0, 1, -1), (1.0, 1.0, 1.0)),
                     ("variogram_set", 4, 6, [[0, 1], [1, 0]], 2.0)]
  en, vg = st.score_energy("truth"), st.score_variogram(None)
  assert h.calls[-2:] == [("energy_score", False), ("variogram_score", True)]
  assert isinstance(en, EnergyScores) and en.names == ("a", "b") and en.invalid == 7 and en.n_members == 4
  np.testing.assert_allclose(en.err, 0.5)                          # sqrt(1 / 4)
  np.testing.assert_allclose(en.energy_score, 0.25)
  assert isinstance(vg, VariogramScores) and vg.offsets == ((0, 1), (1, 0)) and vg.p == 2.0 and vg.n_members == 4
  # without the plans nothing of them is touched
  h2 = _Handle(4)
  plain = verification.ScoredStore(h2, 4, np.ones(4, np.float32))
  plain.setup()
  assert plain.score_energy(None) is None and plain.score_variogram(None) is None
  assert h2.calls == [("reserve", 4), ("weight",)]
  # set per score: the plans are set again by every scoring call, not by setup
  h3 = _Handle(4)
  per = verification.ScoredStore(h3, 4, np.ones(4, np.float32), energy=eplan, variogram=vplan, set_per_score=True)
  per.setup()
  assert h3.calls == [("reserve", 4), ("weight",)]
  per.score_energy(None)
  per.score_variogram(None)
  assert [c[0] for c in h3.calls[2:]] == ["energy_set", "energy_score", "variogram_set", "variogram_score"]


# ---- the rollout's series and results -------------------------------------------------------------------------------------------
def test_energy_spec_restricted_to_the_variables_of_a_store():
  spec = EnergySpec({"uv": ["u10", "v10"], "speed": ["wind10"], "t": ["t2m"]}, weights={"u10": 2.0, "wind10": 3.0})
  main = spec.restricted(_template())
  assert main.names == ("uv", "t") and set(main.weights) == {"u10"}
  flat = ("batch", "time", "lat", "lon")
  z2 = np.zeros((2, 1, N_LAT, N_LON), np.float32)
  view = datasets.Dataset({"wind10": datasets.Variable(flat, z2), "t2m": datasets.Variable(flat, z2)}, _template().coords)
  part = spec.restricted(view)
  assert part.names == ("speed", "t") and part.plan(view)["n_groups"] == 2 and set(part.weights) == {"wind10"}
  assert EnergySpec({"uv": ["u10", "v10"]}).restricted(view) is None


def test_store_series_appends_the_new_scores_after_the_others():
  from gencast_flax_nnx_amd import rollout

  class _Scored(_Handle):
    def ens_score(self, truth, want_fields=False):
      self.calls.append(("score", truth is None))
      return np.ones((self.B, self.C, 6)), np.ones((self.B, self.C, self.M + 1), np.uint64)

  eplan = {"n_groups": 2, "group": np.array([0, 1, -1], np.int32), "scale": np.ones(3), "names": ("a", "b")}
  vplan = VariogramSpec([(0, 1), (1, 0)], 0.5).grid_plan(4, 6)
  h = _Scored(4)
  store = verification.ScoredStore(h, 4, np.ones(4, np.float32), energy=eplan, variogram=vplan)
  store.setup()
  series = rollout._StoreSeries(store, np.array([4.0, 1.0, 0.25]), None)
  series.score_lead("truth")
  series.score_lead("truth")
  assert [c[0] for c in h.calls[4:]] == ["score", "energy_score", "variogram_score"] * 2
  assert h.calls[5] == ("energy_score", True) and h.calls[6] == ("variogram_score", True)   # on the truth already there
  assert len(series.energy) == len(series.variogram) == len(series.raw_variogram) == 2
  np.testing.assert_array_equal(series.variogram[0].sums[2], series.raw_variogram[0].sums[2] * np.array([2.0, 1.0, 0.5])[None, :, None])
  np.testing.assert_array_equal(series.variogram[0].sums[1], series.raw_variogram[0].sums[1] * np.array([4.0, 1.0, 0.25])[None, :, None])
  plain = rollout._StoreSeries(verification.ScoredStore(_Scored(4), 4, np.ones(4, np.float32)), np.ones(3), None)
  assert plain.energy is None and plain.variogram is None and plain.raw_variogram is None
  d = series.derived_result()
  assert d.energy is series.energy or d.energy == series.energy
  assert len(d.variogram_normalized) == 2


def test_rollout_results_merge_with_and_without_the_new_series():
  from gencast_flax_nnx_amd import rollout
  rng = np.random.default_rng(0)
  M, B, C, O = 4, 2, 3, 2
  ens = lambda: verification.EnsembleScores(rng.uniform(1, 2, (B, C, 6)), rng.integers(0, 9, (B, C, M + 1)).astype(np.uint64), M)
  en = lambda: EnergyScores(rng.uniform(1, 2, (B, 2)), rng.uniform(0, 1, (B, 2)), M, ("a", "b"))
  vg = lambda: VariogramScores(rng.uniform(1, 2, (4, B, C, O)), rng.integers(1, 9, (B, C, O)).astype(np.uint64), M, [(0, 1), (1, 0)], 0.5)
  e, v = [[en() for _ in range(2)] for _ in range(2)], [[vg() for _ in range(2)] for _ in range(2)]
  with_mv = [rollout.EnsembleRolloutResult([ens() for _ in range(2)], n_members=M, energy=e[d], variogram=v[d],
                                           variogram_normalized=v[d]) for d in range(2)]
  merged = with_mv[0].merge(with_mv[1])
  for k in range(2):
    np.testing.assert_array_equal(merged.variogram[k].sums, v[0][k].sums + v[1][k].sums)
    np.testing.assert_array_equal(merged.variogram_normalized[k].counts, v[0][k].counts + v[1][k].counts)
    np.testing.assert_array_equal(merged.energy[k].err, np.concatenate([e[0][k].err, e[1][k].err]))
  without = rollout.EnsembleRolloutResult([ens() for _ in range(2)], n_members=M)
  assert without.energy is None and without.variogram is None and without.variogram_normalized is None
  assert "energy" not in vars(without) and "variogram" not in vars(without)      # a result that was not asked for them is as it was
  assert without.merge(without).energy is None
  with pytest.raises(ValueError, match="energy"):
    with_mv[0].merge(without)
  with pytest.raises(ValueError, match="variogram"):
    rollout.EnsembleRolloutResult([ens() for _ in range(2)], n_members=M, variogram=v[0], variogram_normalized=v[0]).merge(without)
  with pytest.raises(ValueError, match="lead times"):
    rollout.EnsembleRolloutResult([ens()], n_members=M, energy=e[0])
  d = [rollout.DerivedRolloutResult([ens() for _ in range(2)], [ens() for _ in range(2)], energy=e[i], variogram=v[i],
                                    variogram_normalized=v[i]) for i in range(2)]
  assert d[0].merge(d[1]).energy[1].n_forecasts == 2 * B
  w = [rollout.WindowRolloutResult([1, 3], 2, [ens() for _ in range(2)], [ens() for _ in range(2)], energy=e[i], variogram=v[i],
                                   variogram_normalized=v[i]) for i in range(2)]
  np.testing.assert_array_equal(w[0].merge(w[1]).variogram[0].sums, v[0][0].sums + v[1][0].sums)
  plain = rollout.WindowRolloutResult([1, 3], 2, [ens() for _ in range(2)], [ens() for _ in range(2)])
  assert plain.merge(plain).energy is None
  with pytest.raises(ValueError, match="energy"):
    w[0].merge(plain)


def test_sampler_refuses_more_than_one_rank_and_an_empty_request():
  from gencast_flax_nnx_amd import ensemble

  class _S:
    _denoiser = None
  with pytest.raises(ValueError, match="one rank"):
    ensemble.EnsembleSampler(_S(), rank=0, world_size=2).multivariate(None, None, None, 4, EnergySpec({"g": ["z"]}))
  with pytest.raises(ValueError, match="EnergySpec"):
    ensemble.EnsembleSampler(_S()).multivariate(None, None, None, 4)


# ---- the one-step wrappers ----------------------------------------------------------------------------------------------------------
def test_wrappers_scale_the_variogram_and_leave_the_energy_score():
  """`InputsAndResiduals.ensemble_multivariate` hands the wrapped predictor normalised inputs and residual-normalised targets,
  scales the variogram sums back with the residual scale of every target channel and returns the energy score as it came;
  `NaNCleaner` cleans inputs and forcings and lets the targets' NaNs through."""
  from gencast_flax_nnx_amd import NaNCleaner, config, rollout, synthetic
  lat, lon = np.linspace(-90, 90, 5), np.arange(8) * 45.0
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  C, M, O, p = 82, 4, 2, 0.5
  rng = np.random.default_rng(1)
  en = EnergyScores(rng.uniform(1, 2, (1, 2)), rng.uniform(0, 1, (1, 2)), M, ("a", "b"))
  vg = VariogramScores(rng.uniform(1, 2, (4, 1, C, O)), rng.integers(1, 9, (1, C, O)).astype(np.uint64), M, [(0, 1), (1, 0)], p)
  seen = {}

  class _Predictor:
    def ensemble_multivariate(self, inputs, targets, forcings=None, **kwargs):
      seen.update(inputs=inputs, targets=targets, forcings=forcings, kwargs=kwargs)
      return (en if kwargs.get("energy") else None), (vg if kwargs.get("variogram") else None)

  def stats(v):
    names = set(config.TASK.input_variables) | set(config.TASK.target_variables) | set(frc.keys())
    return datasets.Dataset({n: (datasets.Variable(("level",), np.full(13, v, np.float32)) if n in config.ALL_ATMOSPHERIC_VARS
                                 else datasets.Variable((), np.float32(v))) for n in names})
  norm = rollout.InputsAndResiduals(_Predictor(), stats(2.0), stats(0.5), stats(0.25))
  got_en, got_vg = norm.ensemble_multivariate(inp, tgt, frc, num_members=M, energy="E", variogram="V")
  assert seen["kwargs"] == dict(num_members=M, energy="E", variogram="V")
  k = "2m_temperature"
  np.testing.assert_array_equal(seen["inputs"][k].data, (inp[k].data - np.float32(0.5)) / np.float32(2.0))
  np.testing.assert_array_equal(seen["targets"][k].data, (tgt[k].data - inp[k].data[:, -1:]) / np.float32(0.25))
  assert got_en is en                                            # normalised units: nothing to scale
  assert set(tgt.keys()) <= set(inp.keys())                      # every target is a residual variable: scale 0.25
  np.testing.assert_array_equal(got_vg.sums[1], vg.sums[1] * 0.25)          # |a|^(2p) = 0.25
  np.testing.assert_array_equal(got_vg.sums[2], vg.sums[2] * 0.5)           # |a|^p = 0.5
  np.testing.assert_array_equal(got_vg.sums[3], vg.sums[3] * 0.5)
  np.testing.assert_array_equal(got_vg.sums[0], vg.sums[0])
  np.testing.assert_array_equal(got_vg.counts, vg.counts)
  only_en, no_vg = norm.ensemble_multivariate(inp, tgt, frc, num_members=M, energy="E")
  assert only_en is en and no_vg is None
  # NaNCleaner around it: a NaN in the inputs is filled, one in the targets reaches the predictor
  dirty_in = datasets.Dataset({n: datasets.Variable(v.dims, np.array(v.data, copy=True)) for n, v in inp.items()}, inp.coords)
  dirty_tg = datasets.Dataset({n: datasets.Variable(v.dims, np.array(v.data, copy=True)) for n, v in tgt.items()}, tgt.coords)
  dirty_in[k].data[..., 0, 0] = np.nan
  dirty_tg[k].data[..., 1, 1] = np.nan
  stack = NaNCleaner(norm, k, datasets.Dataset({k: datasets.Variable((), np.float32(0))}))
  s_en, s_vg = stack.ensemble_multivariate(dirty_in, dirty_tg, frc, num_members=M, energy="E", variogram="V")
  assert s_en is en and np.array_equal(s_vg.sums, got_vg.sums)
  assert np.isfinite(seen["inputs"][k].data).all() and np.isnan(seen["targets"][k].data[..., 1, 1]).all()
