"""Device time of the threshold-weighted CRPS (gc_ens_tail_score at T = 1 and T = 8) next to four things for the same store:
gc_ens_score, gc_ens_order_score, a plain device copy of the M + 1 + T fields, and the route without it -- M
`ens_download_member` calls plus the NumPy reference on the host.
Usage: python tests/gpu_tail_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child
process of its own under a time limit; the first abnormal exit ends the run.

Per case it prints the counter "ens_tail_device_us" (HIP events around the pass and the finish; best of REPS), the rate
(M + 1 + T) * field bytes / time that implies (the bytes the pass must read), "ens_score_device_us" and
"ens_order_device_us" of the same store in the same process, and the host route.  No time is fixed in advance and none is
asserted.  The one relation it reports is what the sort-once design is for: T = 8 thresholds against eight times the O(M^2)
pair loop of gc_ens_score.  Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_tail_timing.py --case
nano50`.
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"nano8": ("nano", 8), "nano50": ("nano", 50), "one_degree8": ("one_degree", 8)}
LIMIT_S = {"nano8": 240, "nano50": 420, "one_degree8": 420}
REPS = 3
T_MAX = 8


def run(case):
  import torch
  from gencast_flax_nnx_amd import _lib, geometry
  from tests import tail_reference as R
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
    offset = np.linspace(-1.5, 1.5, T_MAX)[:, None, None, None]
    thr = ((rng.standard_normal((T_MAX, G, 1, C)) * 0.3 + offset) * scale).astype(np.float32)
    dirs = tuple(+1 if t % 2 == 0 else -1 for t in range(T_MAX))
    nd.ens_reserve(M)
    nd.ens_set_node_weight(w)
    for i in range(M):
      nd.ens_push_host(i, members[i])
    nd.ens_score(truth)                                          # warm-up; the truth stays on the device
    score = []
    for _ in range(REPS):
      nd.ens_score(None)
      score.append(nd.counter("ens_score_device_us"))
    nd.ens_order_set(())
    nd.ens_order_score(None)
    order = []
    for _ in range(REPS):
      nd.ens_order_score(None)
      order.append(nd.counter("ens_order_device_us"))
    field_mb = G * C * 4 / 1e6
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_out {C}, M {M}: a field is {field_mb:.2f} MB")
    print(f"{case}: gc_ens_score, device                      {min(score)} us   (runs: {score})")
    print(f"{case}: gc_ens_order_score Q=0, device            {min(order)} us   (runs: {order})")
    same = True
    best = {}
    down = None
    for T in (1, T_MAX):
      read_mb = (M + 1 + T) * field_mb
      a = torch.empty((M + 1 + T) * G * C, dtype=torch.float32, device="cuda")
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
      nd.ens_tail_set(thr[:T], dirs[:T])
      nd.ens_tail_score(None)                                    # warm-up: makes the partial buffers
      dev, host = [], []
      for _ in range(REPS):
        t0 = time.perf_counter()
        got = nd.ens_tail_score(None)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(nd.counter("ens_tail_device_us"))
      best[T] = min(dev)
      if down is None:
        t0 = time.perf_counter()
        down = np.stack([nd.ens_download_member(i) for i in range(M)])
        t_down = (time.perf_counter() - t0) * 1e3
      t0 = time.perf_counter()
      ref = R.reference(down, truth, w, thr[:T], dirs[:T])
      t_ref = (time.perf_counter() - t0) * 1e3
      ok = bool(np.all(np.abs(got[0] - ref["sums"]) <= R.sum_tolerance(ref, G, M)) and np.array_equal(got[1], ref["counts"])
                and np.array_equal(got[2], ref["invalid"]))
      same = same and ok
      print(f"{case}: plain copy of M + 1 + {T} fields, device        {min(plain)} us   (runs: {plain}) = "
            f"{2 * read_mb / 1e3 / (max(1, min(plain)) * 1e-6):.0f} GB/s read + written")
      print(f"{case}: gc_ens_tail_score T={T}, device            {min(dev)} us   (runs: {dev}) = "
            f"{read_mb / 1e3 / (max(1, min(dev)) * 1e-6):.0f} GB/s of M + 1 + T fields; {min(dev) / max(1, min(score)):.2f} x gc_ens_score, "
            f"{min(dev) / max(1, min(order)):.2f} x gc_ens_order_score")
      print(f"{case}: gc_ens_tail_score T={T}, host wall         {min(host):.3f} ms")
      print(f"{case}: {M} x ens_download_member + NumPy reference T={T}   {t_down:.1f} ms + {t_ref:.1f} ms   "
            f"({os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
      print(f"{case}: T={T}: sums within the bound, counts and invalid equal the reference: {ok}")
    print(f"{case}: T = 8 against eight times gc_ens_score: {best[T_MAX]} us / {8 * min(score)} us = "
          f"{best[T_MAX] / max(1, 8 * min(score)):.3f};   T = 8 against T = 1: {best[T_MAX] / max(1, best[1]):.2f} x")
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
