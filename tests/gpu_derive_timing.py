"""Device time of the derived and pooled ensemble fields (gc_ens_derive) next to a plain device-to-device copy of the same
M + 1 fields, next to gc_ens_score on the same store, and next to the route without it: M `ens_download_member` calls plus
the NumPy reference on the host.
Usage: python tests/gpu_derive_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child
process of its own under a time limit; the first failure ends the run.

Per case it prints, best of REPS, the counter "ens_derive_device_us" (HIP events around the call's launches) for the plans
  none + copy        82 channels copied as they are: moves the bytes of the plain copy, the yardstick of this row
  none + wind speed  10 m wind speed, wind speed on 13 levels and 2 m temperature: 15 derived channels from 29 source channels
  max, mean          82 copied channels pooled over the window of `DerivedSpec.window` at 500 km and at 2000 km
the time of `torch.Tensor.copy_` of (M + 1) fields between two device buffers under torch.cuda events in the same process,
"ens_score_device_us" of the source store, and -- for the max plan at 500 km only, where the host takes seconds rather than
minutes -- the host route with the separable restatement of tests/derive_reference.py (the faster of the two), whose result
the device's must equal.  Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_derive_timing.py --case nano50`.
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"nano8": ("nano", 8), "nano50": ("nano", 50), "one_degree8": ("one_degree", 8)}
LIMIT_S = {"nano8": 300, "nano50": 420, "one_degree8": 900}
REPS = 3
WIND = [("norm2", "10m_wind_speed", "10m_u_component_of_wind", "10m_v_component_of_wind"),
        ("norm2", "wind_speed", "u_component_of_wind", "v_component_of_wind"), ("copy", "2m_temperature")]


def run(case):
  import torch
  from gencast_flax_nnx_amd import DerivedSpec, _lib, config, geometry, synthetic, verification
  from tests import derive_reference as R
  size, M = CASES[case]
  if size == "nano":
    lat, lon, mesh = np.linspace(-90, 90, 73), np.arange(144) * 2.5, 4
  else:
    lat, lon, mesh = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0), 5
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh, attention_k_hop=8)
  tgt = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=0)[1]
  G, C = gr.num_grid_nodes, 82
  mk = lambda c: _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=c + 4, c_out=c, batch=1)
  src, views = mk(C), {C: mk(C), 15: mk(15)}                  # the graph only: no weights
  try:
    for h in [src] + list(views.values()):
      h.set_graph(gr)
      h.ens_reserve(M)
    members, truth = R.data(M, G, 1, C, seed=4)
    src.ens_set_node_weight(verification.node_weights(tgt))
    for i in range(M):
      src.ens_push_host(i, members[i])
    src.ens_score(truth)                                        # warm-up; the truth stays on the device
    score = []
    for _ in range(REPS):
      src.ens_score(None)
      score.append(src.counter("ens_score_device_us"))
    a = torch.empty((M + 1) * G * C, dtype=torch.float32, device="cuda")
    b = torch.zeros_like(a)
    a.copy_(b)
    torch.cuda.synchronize()
    plain = []
    for _ in range(REPS):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      a.copy_(b)
      e1.record()
      torch.cuda.synchronize()
      plain.append(int(round(e0.elapsed_time(e1) * 1e3)))
    del a, b
    field_mb = G * C * 4 / 1e6
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_src {C}, M {M}: a field is {field_mb:.2f} MB, the M + 1 fields {(M + 1) * field_mb:.1f} MB")
    print(f"{case}: gc_ens_score, device                      {min(score)} us   (runs: {score})")
    print(f"{case}: plain copy of M + 1 fields, device        {min(plain)} us   (runs: {plain}) = "
          f"{2 * (M + 1) * field_mb / 1e3 / (max(1, min(plain)) * 1e-6):.0f} GB/s read + written")
    every = [("copy", v) for v in config.TASK.target_variables]
    plans = [("none + copy", DerivedSpec(every)), ("none + wind speed", DerivedSpec(WIND))]
    for km in (500.0, 2000.0):
      for pool in ("max", "mean"):
        plans.append((f"{pool} {km:.0f} km", DerivedSpec(every, pool=pool, radius_km=km)))
    ok = True
    for label, spec in plans:
      plan = spec.plan(tgt)
      view = views[len(plan["op"])]
      view.ens_derive_set(**plan)
      view.ens_derive(src)                                      # warm-up: makes the intermediate
      dev, host = [], []
      for _ in range(REPS):
        t0 = time.perf_counter()
        view.ens_derive(src)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(view.counter("ens_derive_device_us"))
      window = "" if spec.pool is None else f" (r_lat {plan['r_lat']}, r_lon {int(plan['r_lon'].min())} .. {int(plan['r_lon'].max())})"
      print(f"{case} {label:18s}: gc_ens_derive, device     {min(dev)} us   (runs: {dev}) = {min(dev) / max(1, min(plain)):.2f} x the plain copy, "
            f"{min(dev) / max(1, min(score)):.2f} x gc_ens_score; host wall {min(host):.3f} ms{window}")
      if label == "max 500 km":
        got = np.stack([view.ens_download_member(i) for i in range(M)])
        t0 = time.perf_counter()
        down = np.stack([src.ens_download_member(i) for i in range(M)])
        t_down = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ref = R.apply(down, plan, separable=True)
        t_ref = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(got, ref))
        ok = ok and same
        print(f"{case} {label:18s}: {M} x ens_download_member      {t_down:.1f} ms")
        print(f"{case} {label:18s}: NumPy reference (separable)   {t_ref:.1f} ms   ({os.cpu_count()} CPUs visible, "
              f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
        print(f"{case} {label:18s}: the derived members equal the reference: {same}")
    return 0 if ok else 1
  finally:
    for h in [src] + list(views.values()):
      h.close()


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
