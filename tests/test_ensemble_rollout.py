"""Ensemble rollout, the parts that need no GPU: which conditioning channel holds a member's state
(`rollout.state_channels`), the noise a member draws over a rollout, the result's `merge`, the one-rank limit."""
import types

import numpy as np
import pytest

from gencast_flax_nnx_amd import config as cfg
from gencast_flax_nnx_amd import datasets, rollout, verification
from gencast_flax_nnx_amd.datasets import Dataset, Variable
from gencast_flax_nnx_amd.ensemble import member_seed
from gencast_flax_nnx_amd.sampler import Sampler
from gencast_flax_nnx_amd.spectra import EnsembleSpectra
from oracle import rollout_oracle as RO
from tests.test_rollout import _example


def _dyadic_stats(task, seed=5):
  """Scales, locations and residual scales whose quotient rs / s is a power of two: the plan's `a` is float32 by
  contract (gc_rollout_plan), so only then is apply_plan in float64 the float64 composition to rounding error."""
  rng = np.random.default_rng(seed)
  nlev = len(task.pressure_levels)

  def mk(draw):
    out = {}
    for name in sorted(set(task.input_variables) | set(task.target_variables)):
      if name in cfg.ALL_ATMOSPHERIC_VARS:
        out[name] = Variable(("level",), draw(nlev).astype(np.float32))
      else:
        out[name] = Variable((), np.float32(draw(1)[0]))
    return Dataset(out)

  return (mk(lambda n: 2.0 ** rng.integers(-1, 2, n)), mk(lambda n: rng.uniform(-1.0, 1.0, n)),
          mk(lambda n: 2.0 ** rng.integers(-3, 0, n)))


def _f64(ds):
  return Dataset({k: Variable(v.dims, np.asarray(v.data, np.float64)) for k, v in ds.items()}, ds.coords)


def _pack64(ctx, fo_merged):
  """`Denoiser.pack_inputs` without its cast to float32."""
  sizes = dict(fo_merged.sizes)
  sizes.update(ctx.sizes)
  st = np.concatenate([datasets.dataset_to_stacked(ctx, sizes), datasets.dataset_to_stacked(fo_merged, sizes)], axis=-1)
  a = np.transpose(st, (1, 2, 0, 3))
  assert a.dtype == np.float64
  return a.reshape((a.shape[0] * a.shape[1],) + a.shape[2:]), a.shape[:2]


@pytest.mark.parametrize("with_norm", [True, False])
def test_state_channels_pick_the_new_frame_out_of_the_advanced_context(with_norm):
  """apply_plan(cond, sample, forcings)[..., state_src] is the frame `compose_next_frame` appends -- with the wrapper
  normalised with (x - l) / s, without it raw -- in float64 to 1e-12 of scale."""
  from gencast_flax_nnx_amd.denoiser import Denoiser
  task, inputs, targets, forcings = _example(2, batch=2, seed=3)
  inputs, targets, forcings = _f64(inputs), _f64(targets), _f64(forcings)
  stats = tuple(_f64(s) for s in _dyadic_stats(task))
  norm = rollout.InputsAndResiduals(None, *stats) if with_norm else None
  context = rollout.isel_time(inputs, slice(-2, None))
  template = rollout.isel_time(targets, slice(0, 1)).map(np.zeros_like)
  forc0, forc1 = rollout.isel_time(forcings, slice(0, 1)), rollout.isel_time(forcings, slice(1, 2))
  plan, forcing_cols = rollout.build_rollout_plan(context, forc0, template, task, norm)
  c_out = sum(n for _, _, n in datasets.channel_layout(template))
  state_src = rollout.state_channels(plan, c_out)
  assert state_src.dtype == np.int32 and state_src.shape == (c_out,)
  assert (state_src >= 0).all() and len(set(state_src.tolist())) == c_out      # every TASK target is also an input
  assert set(plan["kind"][state_src].tolist()) == ({2} if with_norm else {4})
  np.testing.assert_array_equal(plan["sidx"][state_src], np.arange(c_out))

  n_ctx, n_f0 = (rollout.normalize(context, stats[0], stats[1]), rollout.normalize(forc0, stats[0], stats[1])) \
      if with_norm else (context, forc0)
  cond0, grid_shape = _pack64(n_ctx, n_f0.assign(datasets.zeros_like(template)))
  rng = np.random.default_rng(9)
  sample = rng.standard_normal((cond0.shape[0], cond0.shape[1], c_out))
  norm_pred = Denoiser.unpack_outputs(sample, grid_shape, template)
  pred = norm_pred if norm is None else Dataset(
      {k: norm._unnormalize_prediction_and_add_input(context, k, v) for k, v in norm_pred.items()}, norm_pred.coords)
  frame = rollout.compose_next_frame(pred, forc0, context, task)
  new = Dataset({k: frame[k] for k in template.keys()}, frame.coords)
  if with_norm:
    new = rollout.normalize(new, stats[0], stats[1])
  want = np.transpose(datasets.dataset_to_stacked(new, new.sizes), (1, 2, 0, 3)).reshape(sample.shape)
  assert want.dtype == np.float64

  sizes = dict(forc0.sizes)
  sizes.update(context.sizes)
  frows = rollout.DeviceRollout(None, norm, task)._forcing_rows(forc1, forcing_cols, sizes, grid_shape)
  got = RO.apply_plan(cond0, sample, frows.astype(np.float64), plan)[..., state_src]
  assert got.dtype == np.float64
  scale = max(1.0, float(np.abs(want).max()))
  assert np.abs(got - want).max() <= 1e-12 * scale
  assert np.abs(got - sample).max() > 1e-3 or not with_norm                   # (the state is not the residual sample)


def test_state_channels_of_a_hand_made_plan():
  kind = np.array([1, 2, 0, 3, 4, 0], np.int32)
  sidx = np.array([0, 2, 0, 0, 0, 0], np.int32)
  np.testing.assert_array_equal(rollout.state_channels(dict(kind=kind, sidx=sidx), 4), [4, -1, 1, -1])   # 1, 3: target only
  with pytest.raises(ValueError, match="both take target channel 2"):
    rollout.state_channels(dict(kind=np.array([2, 4], np.int32), sidx=np.array([2, 2], np.int32)), 3)
  with pytest.raises(ValueError, match="outside"):
    rollout.state_channels(dict(kind=np.array([2], np.int32), sidx=np.array([3], np.int32)), 3)


class _StubSampler:
  """`draw_noise` and `seed_from` with `Sampler`'s use of the generator; no denoiser behind it."""
  noise_levels = np.array([1.0, 0.0])
  seed_from = staticmethod(Sampler.seed_from)

  def __init__(self, churn):
    self._stochastic_churn = churn

  def draw_noise(self, rngs, shape, template):
    del template
    assert isinstance(rngs, np.random.Generator)
    return rngs.standard_normal(shape, dtype=np.float32)


def _device_rollout_draws(sampler, rngs, horizon, shape, device_noise, given):
  """What `DeviceRollout.run(..., rngs=rngs)` takes from its generator, in its order: the Philox key first when
  anything is drawn on the device, then one host field per step unless the initial states are drawn there or given."""
  gen = np.random.default_rng(rngs)
  on_device = device_noise and not given
  key = sampler.seed_from(gen) if (on_device or sampler._stochastic_churn) else None
  fields = [None if (on_device or given) else sampler.draw_noise(gen, shape, None) for _ in range(horizon)]
  return key, fields


@pytest.mark.parametrize("device_noise", [False, True])
@pytest.mark.parametrize("churn", [False, True])
@pytest.mark.parametrize("given", [False, True])
def test_a_members_noise_is_the_single_member_rollouts_noise(device_noise, churn, given):
  sampler = _StubSampler(churn)
  model = types.SimpleNamespace(_sampler=sampler, denoiser=None)
  er = rollout.EnsembleRollout(model, base_seed=7, concurrent_members=3, device_noise=device_noise)
  shape, horizon, M = (5, 2, 3), 4, 5
  sources = [er.member_noise(m, given=given) for m in range(M)]
  # consumed step by step across the members, as the driver does: the order between members must not matter
  got = [[src.host_field(shape, None) for src in sources] for _ in range(horizon)]
  keys = set()
  for m in range(M):
    key, fields = _device_rollout_draws(sampler, member_seed(7, m), horizon, shape, device_noise, given)
    assert sources[m].key == key and sources[m].stream == 0
    keys.add(key)
    for k in range(horizon):
      if fields[k] is None:
        assert got[k][m] is None
      else:
        np.testing.assert_array_equal(got[k][m], fields[k])
  assert len(keys) == (M if (churn or (device_noise and not given)) else 1)


def _result(M, horizon, seed, with_spectra=True):
  rng = np.random.default_rng(seed)
  scores = [verification.EnsembleScores(rng.uniform(1, 2, (2, 3, 6)), rng.integers(0, 9, (2, 3, M + 1)).astype(np.uint64), M)
            for _ in range(horizon)]
  spec = [EnsembleSpectra(rng.uniform(1, 2, (2, 3, 4, 6)), M) for _ in range(horizon)] if with_spectra else None
  return rollout.EnsembleRolloutResult([s.scaled(np.full(3, 2.0)) for s in scores], spec, mean="m", variance="v",
                                       members=[[0] * M] * horizon, n_members=M, scores_normalized=scores,
                                       spectra_normalized=spec)


def test_result_merge_adds_lead_time_by_lead_time():
  a, b = _result(4, 3, 1), _result(4, 3, 2)
  m = a.merge(b)
  assert m.horizon == 3 and m.n_members == 4 and m.mean is None and m.variance is None and m.members is None
  for k in range(3):
    np.testing.assert_array_equal(m.scores[k].sums, a.scores[k].sums + b.scores[k].sums)
    np.testing.assert_array_equal(m.scores[k].rank_histogram, a.scores[k].rank_histogram + b.scores[k].rank_histogram)
    np.testing.assert_array_equal(m.scores_normalized[k].sums, a.scores_normalized[k].sums + b.scores_normalized[k].sums)
    np.testing.assert_array_equal(m.spectra[k].sums, a.spectra[k].sums + b.spectra[k].sums)
    assert m.spectra[k].n_dates == 2
  with pytest.raises(ValueError, match="horizons differ"):
    a.merge(_result(4, 2, 3))
  with pytest.raises(ValueError, match="member counts differ"):
    a.merge(_result(5, 3, 3))
  with pytest.raises(ValueError, match="spectra"):
    a.merge(_result(4, 3, 3, with_spectra=False))


def test_ensemble_rollout_is_one_rank_only():
  model = types.SimpleNamespace(_sampler=_StubSampler(False), denoiser=None)
  er = rollout.EnsembleRollout(model, world_size=2)
  with pytest.raises(ValueError, match=r"all members on one rank \(world_size == 1\)"):
    er.run(None, None, None, 2, 4)
  with pytest.raises(ValueError, match="concurrent_members"):
    rollout.EnsembleRollout(model, concurrent_members=0)


def test_forcing_frame_after_the_last_step():
  _, _, _, forcings = _example(3)
  name = next(iter(forcings.keys()))
  frame = lambda ds, k, h: rollout.EnsembleRollout.next_forcings(ds, k, h)[name].data
  at = lambda t: rollout.isel_time(forcings, slice(t, t + 1))[name].data
  np.testing.assert_array_equal(frame(forcings, 0, 3), at(1))
  np.testing.assert_array_equal(frame(forcings, 1, 3), at(2))
  np.testing.assert_array_equal(frame(forcings, 2, 3), at(2))                  # no frame 3: frame 2 again
  np.testing.assert_array_equal(frame(forcings, 1, 2), at(2))                  # horizon 2 and a frame 2: it is used
