"""Device time of the Extreme Forecast Index (gc_ens_efi_score with T = 2 events and E = 20 bins, and the truth-free
gc_ens_efi_fields) next to two things for the same two stores: gc_ens_clim_score -- the yardstick, a pass that reads the same
(M + K + 1) fields -- and the route without it: M + K `ens_download_member` calls plus the NumPy reference on the host.
Usage: python tests/gpu_efi_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child
process of its own under a time limit; the first abnormal exit ends the run.

Per case it prints the counter "ens_efi_device_us" (HIP events around the launches of a call) of REPS calls of each entry,
the rate (M + K + 1) * field bytes / time and the rate of compare-and-adds 2 P M per point that implies (P: K padded to a
power of two), "ens_clim_device_us" in the same process, and the host route.  No time is fixed in advance and none is
asserted.  Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_efi_timing.py --case nano50`.
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"nano8": ("nano", 8, 8), "nano50": ("nano", 50, 30), "one_degree8": ("one_degree", 8, 8)}
LIMIT_S = {"nano8": 240, "nano50": 300, "one_degree8": 420}
REPS = 5


def run(case):
  from gencast_flax_nnx_amd import _lib, geometry
  from gencast_flax_nnx_amd.verification import EfiSpec, efi_table, quantize_node_weights
  from tests import efi_reference as R
  size, M, K = CASES[case]
  if size == "nano":
    lat, lon, mesh, hw = np.linspace(-90, 90, 73), np.arange(144) * 2.5, 4, dict(latent_size=256, d_model=256, num_heads=4)
  else:
    lat, lon, mesh, hw = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0), 5, dict(latent_size=512, d_model=512, num_heads=4)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh, attention_k_hop=8)
  G, C = gr.num_grid_nodes, 82
  make = lambda: _lib.NativeDenoiser(ffw_hidden=2048, num_layers=1, c_in=C + 4, c_out=C, batch=1, **hw)   # the graph only: no weights
  nd, cl = make(), make()
  try:
    nd.set_graph(gr)
    cl.set_graph(gr)
    rng = np.random.default_rng(4)
    scale, offset = np.logspace(-2, 4, C), np.linspace(0.0, 300.0, C)
    clim = (offset + rng.standard_normal((K, G, 1, C)) * scale).astype(np.float32)
    truth = (offset + rng.standard_normal((G, 1, C)) * scale).astype(np.float32)
    members = (truth + 0.5 * rng.standard_normal((M, G, 1, C)) * scale).astype(np.float32)
    w = rng.uniform(0.1, 2.0, G).astype(np.float32)
    wq, _ = quantize_node_weights(w)
    spec = EfiSpec()                                             # T = 2 (the 0.9 and 0.1 quantiles), E = 20
    ranks, a = spec.ranks_for(K), efi_table(K)
    nd.ens_reserve(M)
    nd.ens_set_node_weight(w)
    for i in range(M):
      nd.ens_push_host(i, members[i])
    cl.ens_reserve(K)
    for j in range(K):
      cl.ens_push_host(j, clim[j])
    nd.ens_clim_score(cl, truth)                                 # warm-up; the truth stays on the device
    yard = []
    for _ in range(REPS):
      nd.ens_clim_score(cl, None)
      yard.append(nd.counter("ens_clim_device_us"))
    nd.ens_efi_set(ranks, spec.directions, spec.bins, wq)
    nd.ens_efi_score(cl, a, None)                                # warm-up: makes the buffers
    dev, host, free = [], [], []
    for _ in range(REPS):
      t0 = time.perf_counter()
      got = nd.ens_efi_score(cl, a, None)
      host.append((time.perf_counter() - t0) * 1e3)
      dev.append(nd.counter("ens_efi_device_us"))
    efi, obs = nd.ens_efi_field(0), nd.ens_efi_field(1)
    for _ in range(REPS):
      nd.ens_efi_fields(cl, a)
      free.append(nd.counter("ens_efi_device_us"))
    t0 = time.perf_counter()
    down = np.stack([nd.ens_download_member(i) for i in range(M)])
    down_c = np.stack([cl.ens_download_member(j) for j in range(K)])
    t_down = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = R.reference(down, down_c, truth, w, ranks, spec.directions, spec.bins, wq)
    t_ref = (time.perf_counter() - t0) * 1e3
    tol = R.tolerance(ref, G)
    err = np.abs(got[0] - ref["sums"])
    same = (bool(np.all(err <= tol)) and efi.tobytes() == ref["efi"].tobytes() and obs.tobytes() == ref["observed"].tobytes()
            and np.array_equal(got[1], ref["weighted"]) and np.array_equal(got[2], ref["counts"]) and got[3] == ref["invalid"])
    field_mb = G * C * 4 / 1e6
    read_mb = (M + K + 1) * field_mb
    P = next(p for p in (2, 4, 8, 16, 32, 64) if p >= K)
    gops = 2.0 * P * M * G * C / 1e9
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_out {C}, M {M}, K {K} (P {P}): a field is {field_mb:.2f} MB, the M + K + 1 fields {read_mb:.1f} MB, "
          f"{gops:.2f} G compare-and-adds")
    print(f"{case}: gc_ens_clim_score (the yardstick), device {min(yard)} us   (runs: {yard}) = "
          f"{read_mb / 1e3 / (max(1, min(yard)) * 1e-6):.0f} GB/s of M + K + 1 fields")
    print(f"{case}: gc_ens_efi_score (T 2, E 20), device      {min(dev)} us   (runs: {dev}) = "
          f"{read_mb / 1e3 / (max(1, min(dev)) * 1e-6):.0f} GB/s, {gops / (max(1, min(dev)) * 1e-6) / 1e3:.2f} T compare-and-adds/s; "
          f"{min(dev) / max(1, min(yard)):.2f} x gc_ens_clim_score")
    print(f"{case}: gc_ens_efi_fields (no truth), device      {min(free)} us   (runs: {free}) = "
          f"{(M + K) * field_mb / 1e3 / (max(1, min(free)) * 1e-6):.0f} GB/s of M + K fields; "
          f"{min(free) / max(1, min(yard)):.2f} x gc_ens_clim_score")
    print(f"{case}: gc_ens_efi_score, host wall               {min(host):.3f} ms")
    print(f"{case}: {M} + {K} x ens_download_member              {t_down:.1f} ms")
    print(f"{case}: NumPy reference                           {t_ref:.1f} ms   ({os.cpu_count()} CPUs visible, "
          f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
    print(f"{case}: worst |device - reference| / bound        {float(np.max(err / np.maximum(tol, 1e-300))):.3f}")
    print(f"{case}: fields and tables equal the reference, sums within the bound: {same}")
    return 0 if same else 1
  finally:
    nd.close()
    cl.close()


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
