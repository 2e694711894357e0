"""Device time of the derive ops of gc_ens_derive_set_expr next to a copy plan of the same number of
derived channels through the legacy gc_ens_derive_set plan, and next to the route without them: M `ens_download_member`
calls plus the NumPy reference on the host.
Usage: python tests/gpu_derive_expr_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a
child process of its own under a time limit; the first failure ends the run.

The plan: integrated vapour transport (a norm of two lists of 13 products), the 300 - 500 hPa geopotential thickness and the
850 hPa relative vorticity -- 3 derived channels from 42 source channels of 82.  Per case it prints, best of REPS, the counter
"ens_derive_device_us" (HIP events around the call's launches) for that plan and for the copy plan of 3 channels, their
ratio, and the host route, whose result the device's must lie within the bound of tests/derive_expr_reference.py of.
Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_derive_expr_timing.py --case nano50`."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"nano8": ("nano", 8), "nano50": ("nano", 50), "one_degree8": ("one_degree", 8)}
LIMIT_S = {"nano8": 300, "nano50": 420, "one_degree8": 600}
REPS = 3
LEVELS = (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)
U, V, Q, Z = "u_component_of_wind", "v_component_of_wind", "specific_humidity", "geopotential"


def run(case):
  from gencast_flax_nnx_amd import DerivedSpec, _lib, geometry, synthetic
  from tests import derive_expr_reference as X
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
  src, view = mk(C), mk(3)                                      # the graph only: no weights
  try:
    for h in (src, view):
      h.set_graph(gr)
      h.ens_reserve(M)
    members, truth = R.data(M, G, 1, C, seed=4)
    for i in range(M):
      src.ens_push_host(i, members[i])
    rng = np.random.default_rng(1)
    scale, loc = rng.uniform(0.5, 2.0, C), rng.uniform(-1.0, 1.0, C)
    expr = DerivedSpec([DerivedSpec.ivt("ivt", Q, U, V, LEVELS), DerivedSpec.thickness("thickness", Z, 5, 7), ("vorticity", "vort850", U, V, 10)])
    copy = DerivedSpec([("copy", "2m_temperature"), ("copy", "mean_sea_level_pressure"), ("copy", "10m_u_component_of_wind")])
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_src {C}, M {M}: a source field is {G * C * 4 / 1e6:.2f} MB, a derived field of 3 channels {G * 3 * 4 / 1e6:.2f} MB")
    best, upload = {}, truth
    for label, spec in (("copy x 3 (legacy)", copy), ("ivt, thickness, vort", expr)):
      plan = spec.plan(tgt, scale, loc)
      view.ens_derive_set(**plan)
      view.ens_derive(src, upload)                              # warm-up; the truth stays in the source
      upload = None
      dev, host = [], []
      for _ in range(REPS):
        t0 = time.perf_counter()
        view.ens_derive(src)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(view.counter("ens_derive_device_us"))
      best[label] = min(dev)
      print(f"{case} {label:22s}: gc_ens_derive, device   {min(dev)} us   (runs: {dev}); host wall {min(host):.3f} ms")
    ratio = best["ivt, thickness, vort"] / max(1, best["copy x 3 (legacy)"])
    read_mb = (M + 1) * G * 42 * 4 / 1e6
    print(f"{case}: the new plan takes {ratio:.2f} x the copy plan; it reads 42 source channels per node, {read_mb:.1f} MB = "
          f"{read_mb / 1e3 / (max(1, best['ivt, thickness, vort']) * 1e-6):.0f} GB/s of useful reads")
    got = np.stack([view.ens_download_member(i) for i in range(M)])
    t0 = time.perf_counter()
    down = np.stack([src.ens_download_member(i) for i in range(M)])
    t_down = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref, bound = X.derive(down, plan)
    t_ref = (time.perf_counter() - t0) * 1e3
    print(f"{case}: {M} x ens_download_member      {t_down:.1f} ms")
    print(f"{case}: NumPy reference              {t_ref:.1f} ms   ({os.cpu_count()} CPUs visible, "
          f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
    worst = X.within(got, ref, bound)
    print(f"{case}: the derived members lie within the bound of the reference: largest error / bound {worst:.3g}")
    return 0
  finally:
    src.close()
    view.close()


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
