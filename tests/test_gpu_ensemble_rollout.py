"""Ensemble rollouts resident on the device (gc_ctx_*, gc_ens_push_state, rollout.EnsembleRollout).

Every entry the feature adds is a copy or a gather, and the context update stays gc_rollout_advance: so a member is
compared with the single-member path for EQUAL bits, not within a tolerance.  The scores are compared with the float64
definition on the device's own members within the section 8c bound (G + M^2 + 8) 2^-53 A_k.  Size: the 9 x 16 grid
(G = 144), batch 2, latent 128, 2 layers, 4 noise levels, horizon 3."""

import numpy as np
import pytest

from gencast_flax_nnx_amd import GenCast, _lib, config, datasets, rollout, synthetic, verification, weights
from gencast_flax_nnx_amd.denoiser import Denoiser, dims_from_arch
from gencast_flax_nnx_amd.ensemble import member_seed
from gencast_flax_nnx_amd.sampler import Sampler
from tests import verification_reference as R
from tests.test_gpu_host_api import _small_arch
from tests.test_gpu_verification import _check_sums
from tests.test_rollout import _stats

pytestmark = pytest.mark.gpu

HORIZON, B, C = 3, 2, 82


class _Setup:

  def __init__(self, churn_rate=0.0):
    arch = _small_arch()
    self.lat, self.lon = np.linspace(-90, 90, 9), np.arange(16) * 22.5
    self.inp, tgt1, frc1 = synthetic.make_example(lat=self.lat, lon=self.lon, batch=B, seed=4)
    rng = np.random.default_rng(5)

    def stretch(ds, nt):
      out = {}
      for k, v in ds.items():
        shape = list(v.data.shape)
        shape[v.dims.index("time")] = nt
        out[k] = datasets.Variable(v.dims, rng.standard_normal(shape).astype(np.float32))
      return datasets.Dataset(out, ds.coords)

    self.targets, self.forcings = stretch(tgt1, HORIZON), stretch(frc1, HORIZON)
    sc = config.SamplerConfig(num_noise_levels=4, stochastic_churn_rate=churn_rate)
    params = weights.random_params(dims_from_arch(arch, 262, C), seed=3)
    self.gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=1)
    self.wrapper = rollout.InputsAndResiduals(self.gc, *_stats(config.TASK))
    self.G = len(self.lat) * len(self.lon)
    self.noises = [[rng.standard_normal((self.G, B, C)).astype(np.float32) for _ in range(HORIZON)] for _ in range(4)]
    self.template0 = rollout.isel_time(self.targets, slice(0, 1)).map(np.zeros_like)
    self._single = {}

  def norm(self, which):
    return self.wrapper if which == "wrapper" else None

  def packed(self, which):
    """What `EnsembleRollout.run` sets up, restated: (cond, grid_shape, slots, plan, state_src, forcing rows per step)."""
    norm = self.norm(which)
    context = rollout.isel_time(self.inp, slice(-2, None))
    forc0 = rollout.isel_time(self.forcings, slice(0, 1))
    n_in, n_fo = (rollout.normalize(context, norm._scales, norm._locations),
                  rollout.normalize(forc0, norm._scales, norm._locations)) if norm is not None else (context, forc0)
    cond, grid_shape, slots = self.gc.denoiser.init_for(n_in, self.template0, n_fo)
    plan, cols = rollout.build_rollout_plan(context, forc0, self.template0, config.TASK, norm)
    sizes = dict(forc0.sizes)
    sizes.update(context.sizes)
    rows = [rollout.DeviceRollout(self.gc, norm)._forcing_rows(
        rollout.EnsembleRollout.next_forcings(self.forcings, k, HORIZON), cols, sizes, grid_shape) for k in range(HORIZON)]
    return cond, grid_shape, slots, plan, rollout.state_channels(plan, C), rows

  def single_member_contexts(self, which):
    """The parent's path, driven here on ONE handle, member after member: [m][k] = the conditioning after step k's
    context update.  Computed once per normalisation and left unchanged."""
    if which not in self._single:
      cond, _, slots, plan, _, rows = self.packed(which)
      nd = self.gc.denoiser.native
      nd.set_noisy_slots(slots)
      nd.rollout_plan(**plan)
      nd.set_churn(None)
      sig = np.asarray(self.gc._sampler.noise_levels, np.float32)
      out = []
      for m in range(4):
        nd.upload_cond(cond)
        steps = []
        for k in range(HORIZON):
          nd.upload_noise(self.noises[m][k])
          nd.sample_resident(sig, skip_dead_call=True, want_stats=False)
          nd.rollout_advance(rows[k])
          steps.append(nd.download_cond())
        out.append(steps)
      self._single[which] = out
    return self._single[which]

  def stats_per_channel(self, which):
    norm = self.norm(which)
    layout = datasets.channel_layout(self.template0)
    if norm is None:
      return np.ones(C), np.zeros(C)
    s = np.concatenate([rollout._per_channel_stat(norm._scales, n, self.template0[n], 1.0) for n, _, _ in layout])
    l = np.concatenate([rollout._per_channel_stat(norm._locations, n, self.template0[n], 0.0) for n, _, _ in layout])
    return s, l

  def truth(self, targets, k, which):
    """Lead k's truth in the members' units, restated from the definition: (y - l) / s in float64, rounded once."""
    tk = rollout.isel_time(targets, slice(k, k + 1))
    y = np.transpose(datasets.dataset_to_stacked(tk, tk.sizes), (1, 2, 0, 3)).reshape(self.G, B, C)
    if self.norm(which) is None:
      return y.astype(np.float32)
    s, l = self.stats_per_channel(which)
    return ((y.astype(np.float64) - l) / s).astype(np.float32)


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  for lane in getattr(s.gc.denoiser, "_lanes", None) or []:
    lane.close()
  s.gc.denoiser.native.close()


# ---- 1. a member is the single-member rollout, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("M", [3, 4])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_a_member_is_the_single_member_rollout_bit_for_bit(setup, which, lanes, M):
  want = setup.single_member_contexts(which)
  _, _, slots, _, state_src, _ = setup.packed(which)
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which), concurrent_members=lanes)
  res = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, init_noise=setup.noises[:M], keep_members=True)
  nd = setup.gc.denoiser.native
  keep = np.ones(want[0][0].shape[-1], bool)
  keep[slots] = False                                      # the sampler rewrites the noisy-target slots
  assert (state_src >= 0).all() and keep[state_src].all()
  assert res.horizon == HORIZON and res.n_members == M and len(res.members) == HORIZON
  for m in range(M):
    np.testing.assert_array_equal(nd.ctx_download(m)[..., keep], want[m][-1][..., keep], err_msg=f"context of member {m}")
    for k in range(HORIZON):
      np.testing.assert_array_equal(res.members[k][m], want[m][k][..., state_src], err_msg=f"member {m}, lead {k}")
  # the members differ from one another and from lead to lead: a crossed context could not hide
  assert not np.array_equal(res.members[0][0], res.members[0][1])
  assert not np.array_equal(res.members[0][0], res.members[1][0])


# ---- 2. Dataset level, against DeviceRollout with the member's seed ----------------------------------------------------
@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_members_agree_with_device_rollout_of_the_members_seed(setup, which):
  M, base = 4, 11
  norm = setup.norm(which)
  _, grid_shape, *_ = setup.packed(which)
  res = rollout.EnsembleRollout(setup.gc, norm, base_seed=base, concurrent_members=2).run(
      setup.inp, setup.targets, setup.forcings, HORIZON, M, keep_members=True)
  s, l = setup.stats_per_channel(which)
  for m in range(M):
    dev = rollout.DeviceRollout(setup.gc, norm).run(setup.inp, setup.targets, setup.forcings, HORIZON,
                                                    rngs=member_seed(base, m))
    for k in range(HORIZON):
      tmpl = rollout.isel_time(setup.targets, slice(k, k + 1)).map(np.zeros_like)
      phys = (res.members[k][m].astype(np.float64) * s + l).astype(np.float32)
      got = Denoiser.unpack_outputs(phys, grid_shape, tmpl)
      want = rollout.isel_time(dev, slice(k, k + 1))
      for name in tmpl.keys():
        scale = max(1.0, float(np.abs(want[name].data).max()))
        err = float(np.abs(got[name].data - want[name].data).max())
        assert err < 2e-4 * scale, f"member {m}, lead {k}, {name}: {err:.3e} against {2e-4 * scale:.3e}"


# ---- 3. scores per lead time against the float64 definition on the device's own members --------------------------------
@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_scores_per_lead_time_match_the_float64_definition(setup, which):
  M = 4
  targets = datasets.Dataset({k: datasets.Variable(v.dims, v.data.copy()) for k, v in setup.targets.items()},
                             setup.targets.coords)
  # NaNs in the truth of the LAST lead, at known points of one variable (its counter is the one left standing)
  name = sorted(targets.keys())[0]
  v = targets[name]
  idx = [slice(None)] * v.data.ndim
  idx[v.dims.index("time")] = HORIZON - 1
  idx[v.dims.index("lat")] = slice(2, 4)
  idx[v.dims.index("lon")] = slice(5, 9)
  v.data[tuple(idx)] = np.nan
  res = rollout.EnsembleRollout(setup.gc, setup.norm(which), base_seed=3, concurrent_members=2).run(
      setup.inp, targets, setup.forcings, HORIZON, M, keep_members=True, fields=True)
  nd = setup.gc.denoiser.native
  w = verification.node_weights(setup.template0)
  s, _ = setup.stats_per_channel(which)
  for k in range(HORIZON):
    truth = setup.truth(targets, k, which)
    ref = R.reference(np.stack(res.members[k]), truth, w)
    raw = res.scores_normalized[k]
    _check_sums(f"{which} lead {k}", raw.sums, raw.rank_histogram, ref, setup.G, M)
    np.testing.assert_array_equal(raw.sums[..., 0], ref["sums"][..., 0])          # S0: the sums of the weights, exact
    assert int(raw.rank_histogram.sum()) == setup.G * B * C - ref["invalid"]
    assert (ref["invalid"] > 0) == (k == HORIZON - 1)
    want = raw.scaled(s)
    np.testing.assert_array_equal(res.scores[k].sums, want.sums)
    np.testing.assert_array_equal(res.scores[k].rank_histogram, want.rank_histogram)
  per_chan = int(np.isnan(np.transpose(datasets.dataset_to_stacked(rollout.isel_time(targets, slice(HORIZON - 1, HORIZON)),
                                                                   targets.sizes), (1, 2, 0, 3))).sum())
  assert nd.counter("ens_invalid_points") == ref["invalid"] == per_chan and per_chan >= 2 * 4 * B
  assert res.mean[name].data.shape == targets[name].data.shape == res.variance[name].data.shape
  assert np.isfinite(res.mean[name].data).all() and (res.variance[name].data >= 0).all()


# ---- 4. device noise and churn --------------------------------------------------------------------------------------
def test_device_noise_and_churn_do_not_depend_on_the_lanes():
  s = _Setup(churn_rate=2.5)
  try:
    sampler = s.gc._sampler
    assert sampler._stochastic_churn and (sampler._per_step_churn_rates > 0).sum() >= 2
    M, base = 4, 21
    runs = []
    for lanes in (1, 2):
      res = rollout.EnsembleRollout(s.gc, s.wrapper, base_seed=base, concurrent_members=lanes, device_noise=True).run(
          s.inp, s.targets, s.forcings, HORIZON, M)
      runs.append((res, s.gc.denoiser.native.ctx_download(0)))
    for k in range(HORIZON):
      assert runs[0][0].scores_normalized[k].sums.tobytes() == runs[1][0].scores_normalized[k].sums.tobytes(), k
      np.testing.assert_array_equal(runs[0][0].scores_normalized[k].rank_histogram, runs[1][0].scores_normalized[k].rank_histogram)
    assert np.isfinite(runs[0][0].scores_normalized[-1].sums).all()
    # member 0 on one handle, its Philox stream simply running on from step to step
    cond, _, slots, plan, _, rows = s.packed("wrapper")
    nd = s.gc.denoiser.native
    nd.set_noisy_slots(slots)
    nd.rollout_plan(**plan)
    nd.set_churn(sampler._per_step_churn_rates, sampler._noise_level_inflation_factor)
    nd.noise_seed(Sampler.seed_from(np.random.default_rng(member_seed(base, 0))), 0)
    nd.upload_cond(cond)
    sig = np.asarray(sampler.noise_levels, np.float32)
    streams = []
    for k in range(HORIZON):
      nd.noise_draw()
      nd.sample_resident(sig, skip_dead_call=True, want_stats=False)
      streams.append(nd.counter("noise_stream"))
      nd.rollout_advance(rows[k])
    assert streams == [(1 + int((sampler._per_step_churn_rates > 0).sum())) * (k + 1) for k in range(HORIZON)]
    want = nd.download_cond()
    keep = np.ones(want.shape[-1], bool)
    keep[slots] = False
    for _, ctx0 in runs:
      np.testing.assert_array_equal(ctx0[..., keep], want[..., keep])
  finally:
    for lane in getattr(s.gc.denoiser, "_lanes", None) or []:
      lane.close()
    s.gc.denoiser.native.close()


# ---- 5. spectra per lead time ------------------------------------------------------------------------------------------
def test_spectra_per_lead_time_are_those_of_the_kept_members(setup):
  M = 3
  res = rollout.EnsembleRollout(setup.gc, setup.wrapper, base_seed=5, concurrent_members=2).run(
      setup.inp, setup.targets, setup.forcings, HORIZON, M, keep_members=True, spectra=True)
  nd = setup.gc.denoiser.native
  s, _ = setup.stats_per_channel("wrapper")
  for k in range(HORIZON):
    nd.ens_reserve(M)                                      # a fresh store, filled from the host
    for m in range(M):
      nd.ens_push_host(m, res.members[k][m])
    want = nd.ens_spectrum(setup.truth(setup.targets, k, "wrapper"))
    assert res.spectra_normalized[k].sums.tobytes() == want.tobytes(), f"lead {k}"
    np.testing.assert_array_equal(res.spectra[k].sums, res.spectra_normalized[k].scaled(s).sums)
    assert np.isfinite(want).all() and res.spectra[k].lmax == 8


# ---- 6. state and resources --------------------------------------------------------------------------------------------
def test_runs_and_re_reserves_leave_the_allocations_flat(setup):
  den = setup.gc.denoiser
  run = lambda M: rollout.EnsembleRollout(setup.gc, setup.wrapper, concurrent_members=2).run(
      setup.inp, setup.targets, setup.forcings, 2, M, fields=True, spectra=True)
  run(4)
  handles = [den.native] + list(den.member_lanes(1))
  before = [h.counter("device_allocations") for h in handles]
  run(4)
  run(3)
  den.native.ctx_reserve(7)
  den.native.ens_reserve(5)
  assert [h.counter("device_allocations") for h in handles] == before


def test_new_entries_leave_the_sampling_state_alone(setup):
  cond, _, slots, plan, state_src, _ = setup.packed("wrapper")
  nd = setup.gc.denoiser.native
  nd.set_noisy_slots(slots)
  nd.rollout_plan(**plan)
  nd.set_churn(None)
  sig = np.asarray(setup.gc._sampler.noise_levels, np.float32)
  z = setup.noises[0][0]

  def sample():
    nd.upload_noise(z)
    nd.sample_resident(sig, skip_dead_call=True, want_stats=False)
    return nd.download_sample()

  keep = np.ones(cond.shape[-1], bool)
  keep[slots] = False                                      # (what the noisy-target slots of a conditioning hold is not defined)
  nd.upload_cond(cond)
  first = sample()
  np.testing.assert_array_equal(sample(), first)            # (by now the signature is captured)
  nd.ctx_reserve(2)
  nd.ctx_save(0)
  nd.ens_reserve(2)
  nd.ens_set_node_weight(verification.node_weights(setup.template0))
  nd.ens_push_state(0, state_src)
  nd.ens_push_state(1, state_src)
  np.testing.assert_array_equal(nd.ens_download_member(1), cond[..., state_src])   # no advance yet: the input frame itself
  nd.ens_score(setup.truth(setup.targets, 0, "wrapper"))
  np.testing.assert_array_equal(nd.ctx_download(0)[..., keep], cond[..., keep])
  np.testing.assert_array_equal(nd.download_cond()[..., keep], cond[..., keep])
  np.testing.assert_array_equal(nd.download_sample(), first)
  replays = nd.counter("graph_replays")
  np.testing.assert_array_equal(sample(), first)
  assert nd.counter("graph_replays") == replays + 1
  # ... and a load brings back exactly what was saved, onto another handle too
  lane = setup.gc.denoiser.member_lanes(1)[0]
  lane.set_noisy_slots(slots)
  nd.ctx_load(0, dst=lane)
  np.testing.assert_array_equal(lane.download_cond(), nd.ctx_download(0))
  nd.ctx_save(1, src=lane)
  np.testing.assert_array_equal(nd.ctx_download(1), nd.ctx_download(0))


def test_errors_of_the_new_entries(setup):
  cond, _, slots, plan, state_src, _ = setup.packed("wrapper")
  den = setup.gc.denoiser
  nd = den.native
  nd.set_noisy_slots(slots)
  nd.upload_cond(cond)
  nd.upload_noise(setup.noises[0][0])
  nd.sample_resident(np.asarray(setup.gc._sampler.noise_levels, np.float32), skip_dead_call=True, want_stats=False)
  state_err = _lib.GencastHipError
  for n in (0, 65):
    with pytest.raises(ValueError, match="1..64"):
      nd.ctx_reserve(n)
  nd.ctx_reserve(2)
  nd.ens_reserve(2)
  nd.ctx_save(0)
  for call in (lambda: nd.ctx_save(2), lambda: nd.ctx_save(-1), lambda: nd.ctx_load(2), lambda: nd.ctx_download(2)):
    with pytest.raises(ValueError, match="slot outside"):
      call()
  for call in (lambda: nd.ctx_load(1), lambda: nd.ctx_download(1)):
    with pytest.raises(state_err, match="has not been saved"):
      call()
  idle = den.member_lanes(3)[2]                            # finalized; no rollout uses a third lane here
  with pytest.raises(state_err, match="no conditioning"):
    nd.ctx_save(1, src=idle)
  other = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=cond.shape[-1] + 1,
                              c_out=C, batch=B)
  try:
    other.set_graph(den.graph)
    for call in (lambda: nd.ctx_save(1, src=other), lambda: nd.ctx_load(0, dst=other),
                 lambda: nd.ens_push_state(0, state_src, src=other)):
      with pytest.raises(ValueError, match="other dimensions"):
        call()
  finally:
    other.close()
  with pytest.raises(state_err, match="no context store"):
    idle.ctx_save(0)
  with pytest.raises(ValueError, match="slot outside"):
    nd.ens_push_state(2, state_src)
  with pytest.raises(state_err, match="no sample on the source"):
    nd.ens_push_state(0, state_src, src=idle)
  bad = state_src.copy()
  bad[3] = cond.shape[-1]
  with pytest.raises(ValueError, match="out of range"):
    nd.ens_push_state(0, bad)
  bad[3] = slots[0]
  with pytest.raises(ValueError, match="noisy slot"):
    nd.ens_push_state(0, bad)
  with pytest.raises(ValueError, match="state_src must have shape"):
    nd.ens_push_state(0, state_src[:-1])
  nd.ens_push_state(0, state_src)
  with pytest.raises(ValueError, match="slot outside"):
    nd.ens_download_member(2)
  with pytest.raises(state_err, match="has not been pushed"):
    nd.ens_download_member(1)
  bad[3] = -1                                              # a target-only channel: the sample itself
  nd.ens_push_state(1, bad)
  got = nd.ens_download_member(1)
  np.testing.assert_array_equal(got[..., 3], nd.download_sample()[..., 3])
  np.testing.assert_array_equal(np.delete(got, 3, -1), np.delete(nd.ens_download_member(0), 3, -1))
