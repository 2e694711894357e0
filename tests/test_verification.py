"""Ensemble verification, host side: the float64 reference against itself, `EnsembleScores` arithmetic, the new C-ABI
entries, and the argument errors that need no GPU.  The device side is tests/test_gpu_verification.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from gencast_flax_nnx_amd import (EnsembleSampler, EnsembleScores, GenCast, NaNCleaner, _lib, config, datasets, losses,
                                  rollout, synthetic, verification)
from tests import verification_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(M, G=40, B=2, C=3, seed=0, scale=None):
  rng = np.random.default_rng(seed)
  scale = np.ones(C) if scale is None else np.asarray(scale)
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  w = rng.uniform(0.2, 2.0, G).astype(np.float32)
  return members, truth, w


# ---- the reference against itself ---------------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 3, 8, 50, 64])
def test_pair_sum_brute_force_equals_the_sorted_form(M):
  x = np.random.default_rng(M).standard_normal((M, 500)) * np.logspace(-3, 5, 500)
  brute, srt = R.pair_sum_brute(x), R.pair_sum_sorted(x)
  assert np.all(np.abs(brute - srt) <= 1e-12 * brute)


def test_two_members_closed_form():
  members, truth, w = _case(2, seed=1)
  ref = R.reference(members, truth, w)
  x0, x1, y = (a.astype(np.float64) for a in (members[0], members[1], truth))
  point = 0.5 * (np.abs(x0 - y) + np.abs(x1 - y)) - 0.5 * np.abs(x0 - x1)
  want = (w.astype(np.float64)[:, None, None] * point).sum(0) / w.astype(np.float64).sum()
  np.testing.assert_allclose(R.scores(ref, 2)["crps"], want, rtol=1e-13, atol=1e-15)
  # fair and M^2-normalised forms: crps_ensemble - crps = S5 / (2 M S0)
  s = R.scores(ref, 2)
  np.testing.assert_allclose(s["crps_ensemble"] - s["crps"], ref["sums"][..., 5] / (2 * 2 * ref["sums"][..., 0]), rtol=1e-12)


def test_reference_is_invariant_under_member_permutation_and_a_common_shift():
  members, truth, w = _case(8, seed=2)
  ref = R.reference(members, truth, w)
  perm = np.random.default_rng(0).permutation(8)
  other = R.reference(members[perm], truth, w)
  np.testing.assert_array_equal(other["hist"], ref["hist"])
  np.testing.assert_allclose(other["sums"], ref["sums"], rtol=0, atol=1e-12 * ref["abs_sums"].max())
  # +4 is exact on these float32 values' scale only approximately: compare with the float32 rounding it causes
  shifted = R.reference(members + np.float32(4.0), truth + np.float32(4.0), w)
  for k, name in enumerate(R.SUM_NAMES):
    np.testing.assert_allclose(shifted["sums"][..., k], ref["sums"][..., k], rtol=0,
                               atol=40 * 2.0 ** -22 * max(1.0, ref["abs_sums"][..., k].max()), err_msg=name)


def test_histogram_adds_up_to_the_valid_points_and_invalid_points_are_skipped():
  members, truth, w = _case(8, seed=3)
  truth[3, 0, 1] = np.nan
  members[2, 7, 1, 2] = np.inf
  ref = R.reference(members, truth, w)
  want = np.full((2, 3), 40)
  want[0, 1] -= 1
  want[1, 2] -= 1
  np.testing.assert_array_equal(ref["hist"].sum(-1), want)
  assert ref["invalid"] == 2
  assert np.isnan(ref["mean"][7, 1, 2]) and np.isfinite(ref["mean"][3, 0, 1])
  assert np.isfinite(ref["sums"]).all()
  sc = EnsembleScores(ref["sums"], ref["hist"], 8)
  np.testing.assert_array_equal(sc.valid_points, want)


# ---- EnsembleScores ---------------------------------------------------------------------------------------------
def test_scores_from_hand_made_sums():
  sums = np.zeros((1, 2, 6))
  sums[0, 0] = [2.0, 1.0, 8.0, 18.0, 6.0, 4.0]
  sums[0, 1] = [4.0, -2.0, 4.0, 1.0, 2.0, 1.0]
  hist = np.zeros((1, 2, 5), np.uint64)
  hist[0, :, 0] = 3
  sc = EnsembleScores(sums, hist, 4)
  np.testing.assert_array_equal(sc.valid_weight, [[2.0, 4.0]])
  np.testing.assert_array_equal(sc.bias, [[0.5, -0.5]])
  np.testing.assert_array_equal(sc.rmse, [[2.0, 1.0]])
  np.testing.assert_array_equal(sc.spread, [[3.0, 0.5]])
  np.testing.assert_allclose(sc.spread_skill_ratio, [[np.sqrt(1.25) * 1.5, np.sqrt(1.25) * 0.5]], rtol=1e-15)
  np.testing.assert_array_equal(sc.crps, [[(6.0 - 2.0) / 2.0, (2.0 - 0.5) / 4.0]])
  np.testing.assert_array_equal(sc.crps_ensemble, [[(6.0 - 0.75 * 2.0) / 2.0, (2.0 - 0.75 * 0.5) / 4.0]])
  with pytest.raises(ValueError):
    EnsembleScores(sums, hist, 1)
  with pytest.raises(ValueError):
    EnsembleScores(sums[..., :5], hist, 4)
  with pytest.raises(ValueError):
    EnsembleScores(sums, hist[..., :4], 4)


def test_scores_match_the_reference_formulas():
  members, truth, w = _case(8, seed=4)
  ref = R.reference(members, truth, w)
  sc = EnsembleScores(ref["sums"], ref["hist"], 8)
  for name, want in R.scores(ref, 8).items():
    np.testing.assert_allclose(getattr(sc, name), want, rtol=1e-15, err_msg=name)


def test_scaled_equals_the_reference_on_rescaled_data():
  members, truth, w = _case(8, seed=5)
  a = np.array([4.0, 0.125, -2.0])                       # powers of two: a x is exact in float32
  ref = R.reference(members, truth, w)
  ref_a = R.reference(members * a.astype(np.float32), truth * a.astype(np.float32), w)
  sc = EnsembleScores(ref["sums"], ref["hist"], 8).scaled(a)
  np.testing.assert_allclose(sc.sums, ref_a["sums"], rtol=0, atol=1e-12 * ref_a["abs_sums"].max())
  np.testing.assert_array_equal(sc.rank_histogram, ref_a["hist"])      # mirrored where a < 0 (no ties in this data)
  np.testing.assert_array_equal(sc.rank_histogram[:, :2], ref["hist"][:, :2])
  with pytest.raises(ValueError):
    EnsembleScores(ref["sums"], ref["hist"], 8).scaled([1.0, 2.0])
  with pytest.raises(ValueError):
    EnsembleScores(ref["sums"], ref["hist"], 8).scaled([1.0, 0.0, 2.0])


def test_merge_of_two_halves_of_the_nodes_is_the_whole():
  members, truth, w = _case(8, G=60, seed=6)
  whole = R.reference(members, truth, w)
  parts = [R.reference(members[:, s], truth[s], w[s]) for s in (slice(0, 25), slice(25, 60))]
  merged = EnsembleScores.merge([EnsembleScores(p["sums"], p["hist"], 8) for p in parts])
  np.testing.assert_array_equal(merged.rank_histogram, whole["hist"])
  np.testing.assert_allclose(merged.sums, whole["sums"], rtol=0, atol=1e-13 * whole["abs_sums"].max())
  with pytest.raises(ValueError):
    EnsembleScores.merge([])
  with pytest.raises(ValueError):
    EnsembleScores.merge([merged, EnsembleScores(np.zeros((2, 3, 6)), np.zeros((2, 3, 5), np.uint64), 4)])


def test_per_variable_follows_channel_layout_and_node_weights_follow_losses():
  lat, lon = np.linspace(-90, 90, 13), np.arange(24) * 15.0
  _, tgt, _ = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=1)
  layout = datasets.channel_layout(tgt)
  C = sum(n for _, _, n in layout)
  sums = np.ones((1, C, 6))
  sums[0, :, 2] = np.arange(1, C + 1) ** 2               # rmse = the channel index + 1
  sc = EnsembleScores(sums, np.zeros((1, C, 3), np.uint64), 2)
  pv = sc.per_variable(tgt)
  assert sorted(pv["rmse"].keys()) == sorted(tgt.keys())
  for name, off, n in layout:
    np.testing.assert_array_equal(pv["rmse"][name], np.arange(off + 1, off + n + 1, dtype=np.float64)[None])
    assert pv["rank_histogram"][name].shape == (1, n, 3)
  assert pv["rmse"]["temperature"].shape == (1, 13)       # (batch, level)
  with pytest.raises(ValueError):
    EnsembleScores(sums[:, :5], np.zeros((1, 5, 3), np.uint64), 2).per_variable(tgt)
  nw = verification.node_weights(tgt)
  assert nw.dtype == np.float32 and nw.shape == (13 * 24,)
  np.testing.assert_array_equal(nw.reshape(13, 24), np.repeat(losses.normalized_latitude_weights(lat).astype(np.float32)[:, None], 24, 1))
  assert abs(float(nw.astype(np.float64).mean()) - 1.0) < 1e-6
  np.testing.assert_array_equal(EnsembleScores.node_weights(tgt), nw)
  with pytest.raises(ValueError):
    verification.node_weights(datasets.Dataset({"a": datasets.Variable(("batch",), np.zeros(1))}))


# ---- the C ABI --------------------------------------------------------------------------------------------------
ENTRIES = {
    "gc_ens_reserve": [ctypes.c_void_p, ctypes.c_int32],
    "gc_ens_set_node_weight": [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)],
    "gc_ens_push": [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p],
    "gc_ens_push_host": [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_float)],
    "gc_ens_score": [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int32, ctypes.POINTER(ctypes.c_double),
                     ctypes.POINTER(ctypes.c_uint64)],
    "gc_ens_download_fields": [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)],
}


def test_new_entries_are_declared_bound_and_exported():
  header = open(os.path.join(ROOT, "include", "gencast_hip.h")).read()
  lib = _lib.load_library()
  for name, args in ENTRIES.items():
    assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    res, bound = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and bound == args, name
    assert getattr(lib, name) is not None
  assert "#define GC_ABI_VERSION 1" in header or lib.gc_abi_version() == 1
  for method in ("ens_reserve", "ens_set_node_weight", "ens_push", "ens_push_host", "ens_score", "ens_download_fields"):
    assert callable(getattr(_lib.NativeDenoiser, method))
  assert list(inspect.signature(_lib.NativeDenoiser.ens_push).parameters) == ["self", "slot", "src"]
  assert list(inspect.signature(_lib.NativeDenoiser.ens_score).parameters) == ["self", "truth", "want_fields"]
  sig = inspect.signature(EnsembleSampler.scores)
  assert list(sig.parameters) == ["self", "inputs", "targets", "forcings", "num_members", "fields"]
  assert sig.parameters["fields"].kind is inspect.Parameter.KEYWORD_ONLY
  sig = inspect.signature(GenCast.ensemble_scores)
  assert [p for p, v in sig.parameters.items() if v.kind is inspect.Parameter.KEYWORD_ONLY] == \
      ["num_members", "rngs", "concurrent_members", "fields"]
  assert callable(rollout.InputsAndResiduals.ensemble_scores) and callable(NaNCleaner.ensemble_scores)
  # the new translation unit is in both build lists, and the product does not import the tests' reference
  assert "gc_ensemble.hip" in open(os.path.join(ROOT, "gencast-flax-nnx_amd/csrc/SOURCES")).read().split()
  for script in ("gencast-flax-nnx_amd/csrc/build.sh", "tools/build_variant.sh"):
    assert "< <(grep -v '^#' SOURCES)" in open(os.path.join(ROOT, script)).read(), script
  assert "verification_reference" not in open(os.path.join(ROOT, "gencast-flax-nnx_amd", "verification.py")).read()


# ---- the host path of EnsembleSampler.scores, on a recording stand-in for the handle ---------------------------------
class _RecordingNative:
  def __init__(self, log, name):
    self.log, self.name = log, name

  def set_noisy_slots(self, s):
    pass

  def upload_cond(self, c):
    self.shape = (c.shape[0], c.shape[1], 82)

  def upload_noise(self, z):
    pass

  def sync(self):
    pass

  def cond_device_ptr(self):
    return 0, 0

  def upload_cond_dev(self, ptr):
    self.shape = None

  def sample_resident(self, sigmas, skip_dead_call=True, want_stats=True):
    self.log.append(("sample", self.name))

  def download_sample(self):
    raise AssertionError("scores() must not download a member")

  def ens_reserve(self, n):
    self.log.append(("reserve", n))

  def ens_set_node_weight(self, w):
    self.weight = np.asarray(w)

  def ens_push(self, slot, src=None):
    self.log.append(("push", slot, src.name))

  def ens_score(self, truth=None, want_fields=False):
    self.truth, self.want_fields = truth, want_fields
    return np.ones(self.shape[1:] + (6,)), np.zeros(self.shape[1:] + (5,), np.uint64)

  def ens_download_fields(self):
    return np.full(self.shape, 2.0, np.float32), np.full(self.shape, 3.0, np.float32)


def _host_sampler(log):
  import dataclasses
  from gencast_flax_nnx_amd import Denoiser, weights

  class HostOnlyDenoiser(Denoiser):
    def _maybe_init(self, shape, lat, lon):
      self.dims = weights.ModelDims(c_in=shape[2], c_out=82, latent=128, d_model=128, num_heads=2, ffw_hidden=128, num_layers=1)
      self.native = self.native or _RecordingNative(log, "lane0")
      self._batch, self._initialized = shape[1], True

    def member_lanes(self, count):
      return [_RecordingNative(log, f"lane{i + 1}") for i in range(count)]

  arch = dataclasses.replace(config.nano_architecture(mesh_size=2, d_model=128, num_layers=1, num_heads=2), node_output_size=82)
  gc = GenCast(config.TASK, arch, config.SamplerConfig(num_noise_levels=4, stochastic_churn_rate=0.0), config.NoiseConfig(), None, rngs=3)
  gc.denoiser = HostOnlyDenoiser(None, arch)
  gc._sampler._denoiser = gc.denoiser
  return gc


def test_sampler_scores_pushes_every_member_from_its_lane_and_downloads_none():
  lat, lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
  inp, tgt, frc = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=2)
  log = []
  gc = _host_sampler(log)
  sc = EnsembleSampler(gc._sampler, base_seed=1).scores(inp, tgt, frc, 4)
  assert isinstance(sc, EnsembleScores) and sc.n_members == 4 and sc.sums.shape == (1, 82, 6)
  assert log[0] == ("reserve", 4)
  assert [e for e in log if e[0] == "push"] == [("push", m, "lane0") for m in range(4)]
  native = gc.denoiser.native
  np.testing.assert_array_equal(native.weight, verification.node_weights(tgt))
  want_truth = np.transpose(datasets.dataset_to_stacked(tgt, tgt.sizes), (1, 2, 0, 3)).reshape(9 * 16, 1, 82)
  np.testing.assert_array_equal(native.truth, want_truth)
  assert native.want_fields is False
  # two members in flight: member m is pushed from the lane that sampled it
  del log[:]
  out = EnsembleSampler(gc._sampler, base_seed=1, concurrent_members=2).scores(inp, tgt, frc, 4, fields=True)
  assert [e for e in log if e[0] == "push"] == [("push", 0, "lane0"), ("push", 1, "lane1"), ("push", 2, "lane0"), ("push", 3, "lane1")]
  scores, mean, var = out
  assert isinstance(mean, datasets.Dataset) and sorted(mean.keys()) == sorted(tgt.keys())
  assert mean["temperature"].data.shape == tgt["temperature"].data.shape and float(var["temperature"].data.mean()) == 3.0
  # through GenCast and the wrappers: scaled to physical units, fields un-normalised
  def stats(v):
    names = set(config.TASK.input_variables) | set(config.TASK.target_variables)
    return datasets.Dataset({n: (datasets.Variable(("level",), np.full(13, v, np.float32)) if n in config.ALL_ATMOSPHERIC_VARS
                                 else datasets.Variable((), np.float32(v))) for n in names})
  norm = rollout.InputsAndResiduals(gc, stats(2.0), stats(0.5), stats(0.25))
  stack = NaNCleaner(norm, "2m_temperature", datasets.Dataset({"2m_temperature": datasets.Variable((), np.float32(0))}))
  plain = gc.ensemble_scores(inp, tgt, frc, num_members=4)
  phys, pmean, pvar = stack.ensemble_scores(inp, tgt, frc, num_members=4, fields=True)
  assert set(tgt.keys()) <= set(inp.keys())              # every target is a residual variable: scale 0.25
  np.testing.assert_array_equal(phys.sums, plain.sums * np.array([1.0, 0.25, 0.0625, 0.0625, 0.25, 0.25]))
  np.testing.assert_array_equal(pvar["geopotential"].data, np.full(tgt["geopotential"].data.shape, 3.0 * 0.0625, np.float32))
  k = "2m_temperature"
  np.testing.assert_array_equal(pmean[k].data, np.float32(2.0 * 0.25) + inp[k].data[:, -1:])


def test_argument_errors_that_need_no_gpu():
  log = []
  gc = _host_sampler(log)
  with pytest.raises(ValueError, match="ens_push_host"):
    EnsembleSampler(gc._sampler, rank=0, world_size=2).scores(None, None, None, 4)
  assert log == []
