"""Device time of the ensemble order statistics (gc_ens_order_score with Q = 3, gc_ens_order_fields) next to three things
for the same store: gc_ens_score, a plain device copy of M + 1 fields, and the route without it -- M `ens_download_member`
calls plus the NumPy reference on the host.
Usage: python tests/gpu_order_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child
process of its own under a time limit; the first abnormal exit ends the run.

Per case it prints the counter "ens_order_device_us" (HIP events around the pass and the finish; best of REPS), the rate
(M + 1) * field bytes / time that implies (the bytes the pass must read), "ens_score_device_us" of the same store in the
same process, and the host route.  No time is fixed in advance and none is asserted.  The one relation it reports: whether
at this M the sorted pass, O(M log^2 M) compare-exchanges per point, takes no longer than the O(M^2) pair loop of
gc_ens_score.  Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_order_timing.py --case nano50`.
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
PROBS = (0.1, 0.5, 0.9)


def run(case):
  import torch
  from gencast_flax_nnx_amd import _lib, geometry
  from tests import order_reference as R
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
    rng = np.random.default_rng(4)
    scale = np.logspace(-2, 4, C)
    members = (rng.standard_normal((M, G, 1, C)) * scale).astype(np.float32)
    truth = (rng.standard_normal((G, 1, C)) * scale).astype(np.float32)
    w = rng.uniform(0.1, 2.0, G).astype(np.float32)
    nd.ens_reserve(M)
    nd.ens_set_node_weight(w)
    for i in range(M):
      nd.ens_push_host(i, members[i])
    nd.ens_score(truth)                                          # warm-up; the truth stays on the device
    score = []
    for _ in range(REPS):
      nd.ens_score(None)
      score.append(nd.counter("ens_score_device_us"))
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
    nd.ens_order_set(PROBS)
    nd.ens_order_score(None)                                     # warm-up: makes the partial buffers
    dev, host = [], []
    for _ in range(REPS):
      t0 = time.perf_counter()
      got = nd.ens_order_score(None)
      host.append((time.perf_counter() - t0) * 1e3)
      dev.append(nd.counter("ens_order_device_us"))
    fields = [nd.ens_order_quantile(q) for q in range(len(PROBS))]
    nd.ens_order_fields()
    only = []
    for _ in range(REPS):
      nd.ens_order_fields()
      only.append(nd.counter("ens_order_device_us"))
    t0 = time.perf_counter()
    down = np.stack([nd.ens_download_member(i) for i in range(M)])
    t_down = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = R.reference(down, truth, w, PROBS)
    t_ref = (time.perf_counter() - t0) * 1e3
    tol = R.sum_tolerance(ref, G)
    same = all(np.array_equal(fields[q], ref["fields"][q], equal_nan=True) for q in range(len(PROBS)))
    same = same and np.array_equal(got[3], ref["counts"]) and got[4] == ref["invalid"]
    same = same and all(np.all(np.abs(g - ref[n]) <= tol[n]) for n, g in (("bins", got[0]), ("extra", got[1]), ("pinball", got[2])))
    field_mb = G * C * 4 / 1e6
    read_mb = (M + 1) * field_mb
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_out {C}, M {M}: a field is {field_mb:.2f} MB, the M + 1 fields {read_mb:.1f} MB")
    print(f"{case}: gc_ens_score, device                      {min(score)} us   (runs: {score})")
    print(f"{case}: plain copy of M + 1 fields, device        {min(plain)} us   (runs: {plain}) = "
          f"{2 * read_mb / 1e3 / (max(1, min(plain)) * 1e-6):.0f} GB/s read + written")
    print(f"{case}: gc_ens_order_score Q=3, device            {min(dev)} us   (runs: {dev}) = "
          f"{read_mb / 1e3 / (max(1, min(dev)) * 1e-6):.0f} GB/s of M + 1 fields; {min(dev) / max(1, min(score)):.2f} x gc_ens_score")
    print(f"{case}: gc_ens_order_score Q=3, host wall         {min(host):.3f} ms")
    print(f"{case}: gc_ens_order_fields Q=3, device           {min(only)} us   (runs: {only}) = "
          f"{M * field_mb / 1e3 / (max(1, min(only)) * 1e-6):.0f} GB/s of M fields")
    print(f"{case}: {M} x ens_download_member                  {t_down:.1f} ms")
    print(f"{case}: NumPy reference                           {t_ref:.1f} ms   ({os.cpu_count()} CPUs visible, "
          f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
    print(f"{case}: fields and counts equal the reference, sums within the bound: {same}")
    print(f"{case}: the sorted pass takes no longer than gc_ens_score: {min(dev) <= min(score)}")
    return 0 if same else 1
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
