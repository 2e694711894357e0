"""Device time of the ensemble event tables (gc_ens_event_score) next to gc_ens_score on the same store, and next to the
route without it: M `ens_download_member` calls plus the NumPy reference on the host.
Usage: python tests/gpu_event_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child
process of its own under a time limit; the first failure ends the run.

Per case and T in {1, 4} it prints the counter "ens_event_device_us" (HIP events around the memset, the code pass and the
table pass; best of REPS), the rate (M + T + 1) * field bytes / time that implies (the bytes the code pass must read),
"ens_score_device_us" of the same store in the same process, the host wall time of the call, and the host route.  The one
relation it reports: at T = 1 the event call reads the bytes gc_ens_score reads and does a fraction of its arithmetic, so
it should take no longer.  Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_event_timing.py --case nano50`.
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"nano8": ("nano", 8), "nano50": ("nano", 50), "one_degree8": ("one_degree", 8)}
LIMIT_S = {"nano8": 240, "nano50": 300, "one_degree8": 420}
REPS = 3


def run(case):
  from gencast_flax_nnx_amd import _lib, geometry
  from gencast_flax_nnx_amd.verification import quantize_node_weights
  from tests import event_reference as R
  size, M = CASES[case]
  if size == "nano":
    lat, lon, mesh, hw = np.linspace(-90, 90, 73), np.arange(144) * 2.5, 4, dict(latent_size=256, d_model=256, num_heads=4)
  else:
    lat, lon, mesh, hw = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0), 5, dict(latent_size=512, d_model=512, num_heads=4)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh, attention_k_hop=8)
  G, C = gr.num_grid_nodes, 82
  nd = _lib.NativeDenoiser(ffw_hidden=2048, num_layers=1, c_in=C + 4, c_out=C, batch=1, **hw)   # the graph only: no weights
  try:
    nd.set_graph(gr)
    members, truth, w, thr, d = R.data(M, G, 1, C, seed=4, T=4)
    wq, _ = quantize_node_weights(w)
    nd.ens_reserve(M)
    nd.ens_set_node_weight(w)
    for i in range(M):
      nd.ens_push_host(i, members[i])
    nd.ens_score(truth)                                          # warm-up; the truth stays on the device
    score = []
    for _ in range(REPS):
      nd.ens_score(None)
      score.append(nd.counter("ens_score_device_us"))
    field_mb = G * C * 4 / 1e6
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_out {C}, M {M}: a field is {field_mb:.2f} MB, the members {M * field_mb:.1f} MB")
    print(f"{case}: gc_ens_score, device                    {min(score)} us   (runs: {score})")
    ok = True
    for T in (1, 4):
      nd.ens_event_set(thr[:T], d[:T], wq)
      nd.ens_event_score(None)                                   # warm-up: makes the tables
      dev, host = [], []
      for _ in range(REPS):
        t0 = time.perf_counter()
        got = nd.ens_event_score(None)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(nd.counter("ens_event_device_us"))
      codes = [nd.ens_event_codes(t) for t in range(T)]
      t0 = time.perf_counter()
      down = np.stack([nd.ens_download_member(i) for i in range(M)])
      t_down = (time.perf_counter() - t0) * 1e3
      t0 = time.perf_counter()
      ref = R.tables(down, truth, thr[:T], d[:T], wq)
      t_ref = (time.perf_counter() - t0) * 1e3
      same = all(np.array_equal(a, b) for a, b in zip(got, (ref["weighted"], ref["counts"], ref["invalid"])))
      same = same and all(np.array_equal(codes[t], ref["code"][t]) for t in range(T))
      ok = ok and same
      read_mb = (M + T + 1) * field_mb
      us = max(1, min(dev))
      print(f"{case} T={T}: gc_ens_event_score, device         {min(dev)} us   (runs: {dev}) = {read_mb / 1e3 / (us * 1e-6):.0f} GB/s "
            f"of (M + T + 1) fields; {min(dev) / max(1, min(score)):.2f} x gc_ens_score")
      print(f"{case} T={T}: gc_ens_event_score, host wall      {min(host):.3f} ms")
      print(f"{case} T={T}: {M} x ens_download_member            {t_down:.1f} ms")
      print(f"{case} T={T}: NumPy reference                    {t_ref:.1f} ms   ({os.cpu_count()} CPUs visible, "
            f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
      print(f"{case} T={T}: tables and codes equal the reference: {same}")
      if T == 1:
        print(f"{case} T=1: the event call takes no longer than gc_ens_score: {min(dev) <= min(score)}")
    return 0 if ok else 1
  finally:
    nd.close()


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
