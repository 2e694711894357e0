"""Device time of ensemble feature detection (gc_ens_feature) for one detector -- a minimum of the mean sea level pressure
over 600 km with a 1000 km ring and a 300 km strike radius -- next to the nearest existing device operation, a one-channel
gc_ens_derive with pool = "min" at 600 km, and next to the route without it: M `ens_download_member` calls plus the NumPy
reference on the host.
Usage: python tests/gpu_feature_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child
process of its own under a time limit; the first failure ends the run.

Per case it prints, best of REPS, the counters "ens_feature_device_us" and "ens_derive_device_us" (HIP events around the
call's launches), the host wall time of the calls, the number of centres found, and the host route with the literal
restatement of tests/feature_reference.py, whose lists and strike fields the device's must equal.  Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_feature_timing.py --case nano50`.
"""
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
MSLP = "mean_sea_level_pressure"


def _pressure(rng, n_lat, n_lon, n):
  """n smooth fields [n, G] float32 around 0 with a few lows each, in units of a standard deviation."""
  x = rng.standard_normal((n, n_lat, n_lon))
  for _ in range(6):
    x = (x + np.roll(x, 1, 1) + np.roll(x, -1, 1) + np.roll(x, 1, 2) + np.roll(x, -1, 2)) / 5.0
  return (x / x.std()).astype(np.float32).reshape(n, -1)


def run(case):
  from gencast_flax_nnx_amd import DerivedSpec, FeatureSpec, _lib, datasets, geometry, synthetic
  from tests import derive_reference as DR
  from tests import feature_reference as R
  size, M = CASES[case]
  if size == "nano":
    lat, lon, mesh = np.linspace(-90, 90, 73), np.arange(144) * 2.5, 4
  else:
    lat, lon, mesh = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0), 5
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh, attention_k_hop=8)
  tgt = synthetic.make_example(lat=lat, lon=lon, batch=1, seed=0)[1]
  G, C = gr.num_grid_nodes, 82
  ch = {n: o for n, o, _ in datasets.channel_layout(tgt)}[MSLP]
  mk = lambda c: _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=c + 4, c_out=c, batch=1)
  src, feat, pooled = mk(C), mk(1), mk(1)                     # the graph only: no weights
  try:
    for h in (src, feat, pooled):
      h.set_graph(gr)
      h.ens_reserve(M)
    members, truth = DR.data(M, G, 1, C, seed=4)
    p = _pressure(np.random.default_rng(9), len(lat), len(lon), M + 1)
    members[..., 0, ch], truth[..., 0, ch] = p[:M], p[M]
    for i in range(M):
      src.ens_push_host(i, members[i])
    spec = FeatureSpec({"low": dict(variable=MSLP, kind="min", radius_km=600.0, threshold=-1.0, ring_km=1000.0, depth=0.25,
                                    strike_km=300.0)}, max_centres=64)
    plan = spec.plan(tgt)
    feat.ens_feature_set(**plan)
    feat.ens_feature(src, truth)                                # warm-up: makes the work buffers; the truth stays on the device
    dev, host = [], []
    for _ in range(REPS):
      t0 = time.perf_counter()
      feat.ens_feature(src)
      host.append((time.perf_counter() - t0) * 1e3)
      dev.append(feat.counter("ens_feature_device_us"))
    count, node, value = feat.ens_feature_centres()
    dplan = DerivedSpec([("copy", MSLP)], pool="min", radius_km=600.0).plan(tgt)
    pooled.ens_derive_set(**dplan)
    pooled.ens_derive(src)
    ddev, dhost = [], []
    for _ in range(REPS):
      t0 = time.perf_counter()
      pooled.ens_derive(src)
      dhost.append((time.perf_counter() - t0) * 1e3)
      ddev.append(pooled.counter("ens_derive_device_us"))
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_src {C}, M {M}; extremum window r_lat {int(plan['r_lat'][0])}, r_lon {int(plan['r_lon'].min())} .. "
          f"{int(plan['r_lon'].max())}; ring r_lat {int(plan['ring_lat'][0])}; strike r_lat {int(plan['strike_lat'][0])}")
    print(f"{case}: gc_ens_feature, device                    {min(dev)} us   (runs: {dev}); host wall {min(host):.3f} ms; "
          f"centres per field {count[:, 0, 0].min()} .. {count[:, 0, 0].max()}")
    print(f"{case}: gc_ens_derive min 600 km, 1 channel, device {min(ddev)} us   (runs: {ddev}); host wall {min(dhost):.3f} ms; "
          f"gc_ens_feature = {min(dev) / max(1, min(ddev)):.2f} x this")
    t0 = time.perf_counter()
    down = np.stack([src.ens_download_member(i) for i in range(M)])
    t_down = (time.perf_counter() - t0) * 1e3
    print(f"{case}: {M} x ens_download_member                  {t_down:.1f} ms")
    got = np.stack([feat.ens_download_member(i) for i in range(M)])
    t0 = time.perf_counter()
    r_count, r_node, r_value, r_strike = R.apply(np.concatenate([down, truth[None]]), plan)
    t_ref = (time.perf_counter() - t0) * 1e3
    ok = bool(np.array_equal(count, r_count) and np.array_equal(node, r_node) and np.array_equal(value, r_value)
              and np.array_equal(got, r_strike[:M], equal_nan=True))
    print(f"{case}: NumPy reference                           {t_ref:.1f} ms   ({os.cpu_count()} CPUs visible)")
    print(f"{case}: the device's lists and strike fields equal the reference: {ok}")
    return 0 if ok else 1
  finally:
    for h in (src, feat, pooled):
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
