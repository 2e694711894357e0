"""Host side of the denoising loss: the weights of common/losses.py restated on this package's Dataset, the flat
plan the device takes, and the new C-ABI entries as far as they can be exercised without a GPU."""
import ctypes

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib, config, losses, synthetic
from gencast_flax_nnx_amd.datasets import Dataset, Variable


# ---- latitude / level weights ---------------------------------------------------------------------------
def test_latitude_weights_without_poles_are_unit_mean_cosines():
  lat = np.arange(-89.0, 90.0, 2.0)
  w = losses.normalized_latitude_weights(lat)
  assert w.shape == lat.shape and w.mean() == pytest.approx(1.0, abs=1e-15)
  c = np.cos(np.deg2rad(lat))
  np.testing.assert_allclose(w, c / c.mean(), rtol=1e-14)
  np.testing.assert_allclose(losses.normalized_latitude_weights(lat[::-1]), w[::-1], rtol=1e-14)       # descending too
  np.testing.assert_allclose(losses.normalized_latitude_weights(Dataset({}, dict(lat=lat))), w, rtol=1e-14)


def test_latitude_weights_with_poles():
  d = 2.5
  lat = np.arange(-90.0, 90.0 + 1e-9, d)
  w = losses.normalized_latitude_weights(lat)
  assert w.mean() == pytest.approx(1.0, abs=1e-15)
  raw = np.cos(np.deg2rad(lat)) * np.sin(np.deg2rad(d / 2))
  raw[[0, -1]] = np.sin(np.deg2rad(d / 4)) ** 2
  np.testing.assert_allclose(w, raw / raw.mean(), rtol=1e-14)
  assert w[0] == pytest.approx(w[-1]) and 0 < w[0] < w[1]
  # the reference docstring's property (losses.py:132-135): in the small-angle limit a pole point covers 1/8 of the
  # area of its nearest non-pole neighbour
  fine = losses.normalized_latitude_weights(np.arange(-90.0, 90.0 + 1e-9, 0.25))
  assert fine[0] / fine[1] == pytest.approx(1.0 / 8.0, rel=1e-4)
  assert fine[-1] / fine[-2] == pytest.approx(1.0 / 8.0, rel=1e-4)


def test_latitude_weights_reject_what_the_reference_rejects():
  with pytest.raises(ValueError, match="not uniformly spaced"):
    losses.normalized_latitude_weights(np.array([-90.0, -45.0, 10.0, 45.0, 90.0]))
  with pytest.raises(ValueError, match=r"does not start/end at \+- 90 degrees"):
    losses.normalized_latitude_weights(np.arange(-90.0, 89.0, 2.0))                  # one pole only
  with pytest.raises(ValueError, match=r"\(90 - delta_latitude/2\)"):
    losses.normalized_latitude_weights(np.arange(-88.0, 89.0, 2.0))                  # stops a whole spacing short


def test_level_weights_are_level_over_mean():
  level = np.array(config.PRESSURE_LEVELS_WEATHERBENCH_13, dtype=np.float64)
  w = losses.normalized_level_weights(Dataset({}, dict(level=level)))
  np.testing.assert_allclose(w, level / level.mean(), rtol=1e-15)
  assert w.mean() == pytest.approx(1.0)
  with pytest.raises(ValueError, match="level"):
    losses.normalized_level_weights(Dataset({}, dict(lat=np.arange(3.0))))


# ---- weighted_mse_per_level ----------------------------------------------------------------------------------
def _scrambled(seed=0, batch=3, n_lat=5, n_lon=8, levels=(100.0, 500.0, 850.0), n_time=2):
  """Surface and level variables, each with its dims in another order."""
  rng = np.random.default_rng(seed)
  coords = dict(lat=np.linspace(-90, 90, n_lat), lon=np.arange(n_lon) * (360.0 / n_lon), level=np.asarray(levels))
  L = len(levels)
  def pair(dims, shape):
    return (Variable(dims, rng.standard_normal(shape)), Variable(dims, rng.standard_normal(shape)))
  vars_ = {
      "t2m": pair(("batch", "time", "lat", "lon"), (batch, n_time, n_lat, n_lon)),
      "msl": pair(("lon", "batch", "lat", "time"), (n_lon, batch, n_lat, n_time)),
      "z": pair(("batch", "time", "level", "lat", "lon"), (batch, n_time, L, n_lat, n_lon)),
      "q": pair(("lat", "level", "lon", "time", "batch"), (n_lat, L, n_lon, n_time, batch)),
  }
  return (Dataset({k: v[0] for k, v in vars_.items()}, coords), Dataset({k: v[1] for k, v in vars_.items()}, coords))


def test_weighted_mse_per_level_against_a_brute_force_loop():
  pred, tgt = _scrambled()
  weights = {"msl": 0.1, "q": 2.0}
  loss, diag = losses.weighted_mse_per_level(pred, tgt, weights)
  assert loss.dims == ("batch",) and loss.data.shape == (3,)
  latw = losses.normalized_latitude_weights(tgt.coords["lat"])
  levw = tgt.coords["level"] / tgt.coords["level"].mean()
  want_total = np.zeros(3)
  for name in tgt.keys():
    v, p = tgt[name], pred[name]
    acc, cnt = np.zeros(3), 0
    for idx in np.ndindex(*v.data.shape):
      where = dict(zip(v.dims, idx))
      w = latw[where["lat"]] * (levw[where["level"]] if "level" in where else 1.0)
      acc[where["batch"]] += w * (p.data[idx] - v.data[idx]) ** 2
      cnt += 1
    want = acc / (cnt / 3)
    assert diag[name].dims == ("batch",)
    np.testing.assert_allclose(diag[name].data, want, rtol=1e-12)
    want_total += weights.get(name, 1.0) * want
  np.testing.assert_allclose(loss.data, want_total, rtol=1e-12)


def test_sum_per_variable_losses_rejects_a_weight_without_a_variable():
  pred, tgt = _scrambled()
  with pytest.raises(ValueError, match="does not correspond to any variable"):
    losses.weighted_mse_per_level(pred, tgt, {"nope": 1.0})
  per = {"a": Variable(("batch",), np.array([1.0, 2.0])), "b": Variable(("batch",), np.array([10.0, 20.0]))}
  total, same = losses.sum_per_variable_losses(per, {"b": 0.5})
  np.testing.assert_allclose(total.data, [6.0, 12.0])
  assert same is per
  with pytest.raises(ValueError, match="does not correspond to any variable"):
    losses.loss_plan(tgt, {"nope": 1.0})


# ---- loss_plan -------------------------------------------------------------------------------------------------
def test_loss_plan_for_the_task_on_the_2p5_degree_grid():
  _, targets, _ = synthetic.make_example()
  plan = losses.loss_plan(targets)
  assert plan.names == tuple(sorted(config.TASK.target_variables)) and len(plan.names) == 10
  assert plan.node_weight.shape == (73 * 144,) and plan.node_weight.dtype == np.float32
  assert plan.channel_weight.shape == (82,) and plan.channel_group.shape == (82,) and plan.channel_group.dtype == np.int32
  assert (np.diff(plan.channel_group) >= 0).all() and plan.channel_group[0] == 0 and plan.channel_group[-1] == 9
  for g in range(10):
    assert plan.channel_weight[plan.channel_group == g].astype(np.float64).sum() == pytest.approx(1.0, abs=1e-6)
  assert plan.node_weight.astype(np.float64).sum() == pytest.approx(1.0, abs=1e-6)
  by_name = dict(zip(plan.names, plan.group_weight))
  for name in plan.names:
    light = name in ("10m_u_component_of_wind", "10m_v_component_of_wind", "mean_sea_level_pressure")
    assert by_name[name] == np.float32(0.1 if light else 1.0), name
  level = np.array(config.TASK.pressure_levels, dtype=np.float64)
  z = plan.channel_weight[plan.channel_group == plan.names.index("geopotential")]
  np.testing.assert_allclose(z, level / level.mean() / 13, rtol=1e-6)
  # node = lat_i * n_lon + lon_j: constant along a latitude row, the pole rows lightest
  rows = plan.node_weight.reshape(73, 144)
  assert (rows == rows[:, :1]).all() and rows[0, 0] == rows[-1, 0] < rows[1, 0] < rows[36, 0]


def test_loss_plan_flat_evaluation_equals_weighted_mse_per_level():
  from gencast_flax_nnx_amd import datasets
  pred, tgt = _scrambled(seed=3, batch=2, n_lat=7, n_lon=12, levels=(50.0, 250.0, 500.0, 1000.0), n_time=1)
  weights = {"msl": 0.1, "t2m": 0.3}
  want_loss, want_diag = losses.weighted_mse_per_level(pred, tgt, weights)
  plan = losses.loss_plan(tgt, weights, dtype=np.float64)
  assert plan.names == ("msl", "q", "t2m", "z")
  flat = lambda ds: np.transpose(datasets.dataset_to_stacked(ds, ds.sizes), (1, 2, 0, 3)).reshape(7 * 12, 2, -1)
  loss, per_group = plan.evaluate((flat(pred) - flat(tgt)) ** 2)
  np.testing.assert_allclose(loss, want_loss.data, rtol=1e-12)
  for g, name in enumerate(plan.names):
    np.testing.assert_allclose(per_group[:, g], want_diag[name].data, rtol=1e-12)
  # two time steps: a channel's level is found through the variable's own dim order
  pred2, tgt2 = _scrambled(seed=4, batch=2, n_lat=7, n_lon=12, n_time=2)
  plan2 = losses.loss_plan(tgt2, {}, dtype=np.float64)
  flat2 = lambda ds: np.transpose(datasets.dataset_to_stacked(ds, ds.sizes), (1, 2, 0, 3)).reshape(7 * 12, 2, -1)
  loss2, _ = plan2.evaluate((flat2(pred2) - flat2(tgt2)) ** 2)
  np.testing.assert_allclose(loss2, losses.weighted_mse_per_level(pred2, tgt2, {})[0].data, rtol=1e-12)


# ---- ABI ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("gc_loss_set_weights", "gc_upload_targets", "gc_loss_resident", "gc_download_denoised", "gc_loss")


def test_new_symbols_are_exported_and_bound():
  lib = _lib.load_library()
  for name in NEW_SYMBOLS:
    assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert getattr(lib, name).restype is ctypes.c_int
  for method in ("loss_set_weights", "upload_targets", "loss_resident", "download_denoised", "loss"):
    assert callable(getattr(_lib.NativeDenoiser, method))


def test_argument_errors_that_need_no_gpu():
  lib = _lib.load_library()
  f = (ctypes.c_float * 4)()
  i = (ctypes.c_int32 * 4)()
  assert lib.gc_loss_set_weights(None, f, f, i, 1, f) == _lib.GC_ERR_INVALID_ARGUMENT        # no handle
  assert lib.gc_upload_targets(None, f) == _lib.GC_ERR_INVALID_ARGUMENT
  assert lib.gc_loss_resident(None, f, 1, 0, f, f) == _lib.GC_ERR_INVALID_ARGUMENT
  assert lib.gc_download_denoised(None, f) == _lib.GC_ERR_INVALID_ARGUMENT
  assert lib.gc_loss(None, f, f, f, f, f, f, None) == _lib.GC_ERR_INVALID_ARGUMENT


def test_gencast_loss_still_raises_and_points_to_the_new_methods():
  from gencast_flax_nnx_amd import GenCast, NaNCleaner, create_gencast_model
  gc = create_gencast_model(mesh_size=2, d_model=128, num_layers=1, num_heads=2)
  with pytest.raises(NotImplementedError, match="denoising_loss"):
    gc.loss()
  with pytest.raises(NotImplementedError, match="denoising_loss"):
    gc.loss_and_predictions()
  nc = NaNCleaner(gc, "sst", Dataset({"sst": Variable((), np.float32(0))}))
  with pytest.raises(NotImplementedError, match="denoising_loss"):
    nc.loss()
  assert callable(GenCast.denoising_loss) and callable(GenCast.denoising_loss_and_predictions)
  inp, tgt, frc = synthetic.make_example(lat=np.linspace(-90, 90, 5), lon=np.arange(8) * 45.0)
  bare = GenCast(config.TASK, config.nano_architecture(mesh_size=1), config.SamplerConfig(stochastic_churn_rate=0.0))
  with pytest.raises(ValueError, match="Noise config must be specified"):                        # before any GPU work
    bare.denoising_loss(inp, tgt, frc, rngs=1)


# ---- the wrappers around a predictor's denoising_loss (no GPU: a recording stand-in plays GenCast) ---------------
class _InnerLoss:
  """Returns package types whatever it is given, like GenCast called from a wrapper; records its arguments."""

  def denoising_loss(self, inputs, targets, forcings=None, **kw):
    self.seen = (inputs, targets, forcings, kw)
    return Variable(("batch",), np.array([1.5], np.float32)), Dataset({"sst": Variable(("batch",), np.array([0.5], np.float32))})

  def denoising_loss_and_predictions(self, inputs, targets, forcings=None, **kw):
    self.seen = (inputs, targets, forcings, kw)
    preds = Dataset({k: Variable(v.dims, np.full(np.shape(v.data), 2.0, np.float32)) for k, v in targets.items()}, targets.coords)
    return self.denoising_loss(inputs, targets, forcings, **kw), preds


def _sst_case():
  rng = np.random.default_rng(0)
  dims = ("batch", "time", "lat", "lon")
  coords = dict(lat=np.linspace(-90, 90, 3), lon=np.arange(4) * 90.0)
  sst_in = rng.standard_normal((1, 2, 3, 4)).astype(np.float32)
  sst_in[0, 0, 1, 2] = np.nan                                  # a "land" point in one input frame
  sst_tg = rng.standard_normal((1, 1, 3, 4)).astype(np.float32)
  sst_tg[0, 0, 2, 3] = np.nan
  return dims, coords, sst_in, sst_tg


def test_nan_cleaner_loss_cleans_targets_and_reintroduces_nans_in_the_predictions():
  from gencast_flax_nnx_amd import NaNCleaner
  dims, coords, sst_in, sst_tg = _sst_case()
  inputs, targets = Dataset({"sst": Variable(dims, sst_in)}, coords), Dataset({"sst": Variable(dims, sst_tg)}, coords)
  fill = Dataset({"sst": Variable((), np.float32(-7.0))})
  for reintroduce in (False, True):
    inner = _InnerLoss()
    nc = NaNCleaner(inner, "sst", fill, reintroduce_nans=reintroduce)
    loss, diag = nc.denoising_loss(inputs, targets, None, noise_levels=[1.0])
    got_in, got_tg, _, kw = inner.seen
    assert kw == {"noise_levels": [1.0]} and loss.dims == ("batch",) and "sst" in diag.keys()
    assert got_in["sst"].data[0, 0, 1, 2] == -7.0 and got_tg["sst"].data[0, 0, 2, 3] == -7.0
    assert not np.isnan(got_in["sst"].data).any() and not np.isnan(got_tg["sst"].data).any()
    assert np.isnan(targets["sst"].data).sum() == 1                               # the caller's data is untouched
    (loss2, _), preds = nc.denoising_loss_and_predictions(inputs, targets, None)
    assert not np.isnan(inner.seen[1]["sst"].data).any() and float(loss2.data[0]) == 1.5
    mask = np.isnan(preds["sst"].data[0, 0])
    if reintroduce:                                                               # NaN where ANY input frame was NaN
      want = np.zeros((3, 4), bool)
      want[1, 2] = True
      np.testing.assert_array_equal(mask, want)
      assert (preds["sst"].data[0, 0][~mask] == 2.0).all()
    else:
      assert not mask.any()


def test_wrapper_stack_returns_xarray_for_xarray_arguments(monkeypatch):
  import sys
  from gencast_flax_nnx_amd import NaNCleaner, rollout
  from tests import fake_xarray
  monkeypatch.setitem(sys.modules, "xarray", fake_xarray)
  dims, coords, sst_in, sst_tg = _sst_case()
  stat = lambda v: Dataset({"sst": Variable((), np.float32(v))})
  inner = _InnerLoss()
  stack = NaNCleaner(rollout.InputsAndResiduals(inner, stat(2.0), stat(0.5), stat(0.25)), "sst", stat(-7.0))
  x_in = fake_xarray.Dataset({"sst": (dims, sst_in)}, coords)
  x_tg = fake_xarray.Dataset({"sst": (dims, sst_tg)}, coords)
  for model in (stack, stack.predictor):
    loss, diag = model.denoising_loss(x_in, x_tg, None)
    assert isinstance(loss, fake_xarray.DataArray) and loss.dims == ("batch",) and loss.values.tolist() == [1.5]
    assert isinstance(diag, fake_xarray.Dataset) and diag["sst"].dims == ("batch",)
    (loss2, diag2), preds = model.denoising_loss_and_predictions(x_in, x_tg, None)
    assert isinstance(loss2, fake_xarray.DataArray) and isinstance(diag2, fake_xarray.Dataset)
    assert isinstance(preds, fake_xarray.Dataset) and preds["sst"].dims == dims
  # package Datasets in: package types out
  loss, diag = stack.denoising_loss(Dataset({"sst": Variable(dims, sst_in)}, coords), Dataset({"sst": Variable(dims, sst_tg)}, coords), None)
  assert isinstance(loss, Variable) and isinstance(diag, Dataset)
  # the residual normalisation the inner predictor saw, written out: (target - last input frame) / diffs_stddev
  clean_in, clean_tg = np.where(np.isnan(sst_in), -7.0, sst_in), np.where(np.isnan(sst_tg), -7.0, sst_tg)
  np.testing.assert_allclose(inner.seen[1]["sst"].data, (clean_tg - clean_in[:, -1:]) / 0.25, rtol=1e-6)
  np.testing.assert_allclose(inner.seen[0]["sst"].data, (clean_in - 0.5) / 2.0, rtol=1e-6)
  # ... and the predictions come back un-normalised with the last input frame added: 2.0 * 0.25 + last
  _, preds = stack.denoising_loss_and_predictions(Dataset({"sst": Variable(dims, sst_in)}, coords),
                                                  Dataset({"sst": Variable(dims, sst_tg)}, coords), None)
  np.testing.assert_allclose(preds["sst"].data, 0.5 + clean_in[:, -1:], rtol=1e-6)
