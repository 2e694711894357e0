"""What keeping an ensemble rollout on the device costs and saves.
Usage: python tests/gpu_ensemble_rollout_timing.py [nano8_1lane] [nano8_3lanes] [one_degree4]   (default: all three).
Each case runs in a child process of its own under a time limit; the first failure ends the run.

Per case it prints
  * wall ms per member-step of `EnsembleRollout.run` (M members x horizon steps, 20 noise levels = 39 denoiser calls per
    member-step, scores at every lead time);
  * what the feature adds to a member-step on the device: REPS x (gc_ctx_load, gc_ctx_save, gc_ens_push_state) enqueued
    back to back on an otherwise idle handle -- the HIP-event time of their gc_pack launches (the state gather and the
    re-pack gc_ctx_load ends with; per-class profiling), and the wall time of the whole batch up to one gc_sync, which also
    holds the two device-to-device copies (an upper bound: it contains the enqueue cost) -- and per lead time the counter
    "ens_score_device_us";
  * the same forecast by the only route there was before: M x `DeviceRollout.run` (every sample downloaded), the states
    composed on the host, `ens_push_host` of every field and one `ens_score` per lead time.
"""
import dataclasses
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"nano8_1lane": ("nano", 8, 4, 1), "nano8_3lanes": ("nano", 8, 4, 3), "one_degree4": ("one_degree", 4, 2, 1)}
LIMIT_S = {"nano8_1lane": 420, "nano8_3lanes": 420, "one_degree4": 900}
REPS = 20


def run(case):
  from gencast_flax_nnx_amd import GenCast, _lib, config, datasets, rollout, synthetic, verification, weights
  from gencast_flax_nnx_amd.denoiser import dims_from_arch
  from gencast_flax_nnx_amd.ensemble import member_seed
  from tests.test_rollout import _stats
  size, M, horizon, lanes = CASES[case]
  if size == "nano":
    lat, lon = synthetic.grid_2p5deg()
    arch = config.nano_architecture(mesh_size=4, d_model=256, num_layers=16, num_heads=4)
  else:
    lat, lon = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0)
    arch = config.nano_architecture(mesh_size=5, d_model=512, num_layers=16, num_heads=4)
  arch = dataclasses.replace(arch, node_output_size=82)
  inp, tgt1, frc1 = synthetic.make_example(lat, lon, batch=1, seed=0)
  rng = np.random.default_rng(1)

  def stretch(ds, nt):
    out = {}
    for k, v in ds.items():
      shape = list(v.data.shape)
      shape[v.dims.index("time")] = nt
      out[k] = datasets.Variable(v.dims, rng.standard_normal(shape).astype(np.float32))
    return datasets.Dataset(out, ds.coords)

  targets, forcings = stretch(tgt1, horizon), stretch(frc1, horizon)
  sc = config.SamplerConfig(max_noise_level=80.0, min_noise_level=0.03, num_noise_levels=20, rho=7.0, stochastic_churn_rate=0.0)
  params = weights.random_params(dims_from_arch(arch, 262, 82), seed=3)
  gc = GenCast(config.TASK, arch, sc, config.NoiseConfig(), None, params=params, rngs=1)
  norm = rollout.InputsAndResiduals(gc, *_stats(config.TASK))
  er = rollout.EnsembleRollout(gc, norm, base_seed=2, concurrent_members=lanes)
  er.run(inp, targets, forcings, 2, max(2, lanes))                 # warm-up: lazy set-up, the sample graph's capture
  nd = gc.denoiser.native
  t0 = time.perf_counter()
  res = er.run(inp, targets, forcings, horizon, M)
  t_ens = time.perf_counter() - t0
  score_us = nd.counter("ens_score_device_us")
  G = len(lat) * len(lon)
  print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
  print(f"{case}: G {G}, M {M}, horizon {horizon}, lanes {lanes}: a context is {G * 262 * 4 / 1e6:.1f} MB, a member {G * 82 * 4 / 1e6:.1f} MB")
  print(f"{case}: EnsembleRollout.run            {1e3 * t_ens:9.1f} ms = {1e3 * t_ens / (M * horizon):8.2f} ms per member-step "
        f"(leads: {', '.join(f'{x:.0f}' for x in er.last_lead_ms)} ms)")

  # ---- what the feature adds per member-step, on an idle handle
  plan, _ = rollout.build_rollout_plan(rollout.isel_time(inp, slice(-2, None)), rollout.isel_time(forcings, slice(0, 1)),
                                       rollout.isel_time(targets, slice(0, 1)).map(np.zeros_like), config.TASK, norm)
  state_src = rollout.state_channels(plan, 82)
  pack = nd.kernel_classes().index("gc_pack")
  nd.sync()
  nd.profile_enable(pack)
  t0 = time.perf_counter()
  for i in range(REPS):
    nd.ctx_load(i % M)
    nd.ctx_save(i % M)
    nd.ens_push_state(i % M, state_src)
  nd.sync()
  t_batch = time.perf_counter() - t0
  launches, ms = nd.profile_read()
  nd.profile_enable(-1)
  assert launches == 2 * REPS, launches
  added = 1e3 * t_batch / REPS
  print(f"{case}: added per member-step: gc_pack launches (gather + re-pack) {1e3 * ms / REPS:7.1f} us on the device; "
        f"with the two context copies, wall of a batch of {REPS} / {REPS}: {added:7.3f} ms")
  print(f"{case}: added per lead time: gc_ens_score {score_us} us on the device")
  step = 1e3 * t_ens / (M * horizon)
  print(f"{case}: added / member-step = {100 * (added + 1e-3 * score_us / M) / step:.2f} % (expected below 1 %)")

  # ---- the route there was: M single-member rollouts, downloads, states on the host, ens_push_host, ens_score
  s = np.concatenate([rollout._per_channel_stat(norm._scales, n, tgt1[n], 1.0) for n, _, _ in datasets.channel_layout(tgt1)])
  l = np.concatenate([rollout._per_channel_stat(norm._locations, n, tgt1[n], 0.0) for n, _, _ in datasets.channel_layout(tgt1)])
  dr = rollout.DeviceRollout(gc, norm)
  dr.run(inp, targets, forcings, 2, rngs=0)                          # warm-up of this route's own signature
  t0 = time.perf_counter()
  preds = [dr.run(inp, targets, forcings, horizon, rngs=member_seed(2, m)) for m in range(M)]
  t_roll = time.perf_counter() - t0
  t0 = time.perf_counter()
  nd.ens_reserve(M)
  nd.ens_set_node_weight(verification.node_weights(tgt1))
  worst = 0.0
  for k in range(horizon):
    tk = rollout.isel_time(targets, slice(k, k + 1))
    to_field = lambda ds: np.transpose(datasets.dataset_to_stacked(ds, ds.sizes), (1, 2, 0, 3)).reshape(G, 1, 82)
    norm_of = lambda y: ((y.astype(np.float64) - l) / s).astype(np.float32)
    for m in range(M):
      nd.ens_push_host(m, norm_of(to_field(rollout.isel_time(preds[m], slice(k, k + 1)))))
    sums, _ = nd.ens_score(norm_of(to_field(tk)))
    old = verification.EnsembleScores(sums, np.zeros(sums.shape[:2] + (M + 1,), np.uint64), M).scaled(s)
    worst = max(worst, float(np.max(np.abs(old.crps - res.scores[k].crps) / np.abs(res.scores[k].crps))))
  t_host = time.perf_counter() - t0
  t_old = t_roll + t_host
  print(f"{case}: M x DeviceRollout.run          {1e3 * t_roll:9.1f} ms; states on the host, ens_push_host, ens_score {1e3 * t_host:8.1f} ms")
  print(f"{case}: the route before, in all       {1e3 * t_old:9.1f} ms = {1e3 * t_old / (M * horizon):8.2f} ms per member-step "
        f"({t_old / t_ens:.2f} x the resident route)")
  print(f"{case}: fair CRPS of the two routes differ by at most {worst:.2e} relative")
  ok = bool(np.isfinite(res.scores[-1].crps).all()) and worst < 1e-2
  for lane in getattr(gc.denoiser, "_lanes", None) or []:
    lane.close()
  nd.close()
  return 0 if ok else 1


if __name__ == "__main__":
  if len(sys.argv) == 3 and sys.argv[1] == "--case":
    sys.exit(run(sys.argv[2]))
  for name in (sys.argv[1:] or list(CASES)):
    if name not in CASES:
      sys.exit(f"unknown case {name!r}: one of {', '.join(CASES)}")
    try:
      rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], timeout=LIMIT_S[name]).returncode
    except subprocess.TimeoutExpired:
      sys.exit(f"{name}: no result within {LIMIT_S[name]} s; stopping here")
    if rc != 0:
      sys.exit(f"{name}: exit status {rc}; stopping here")
