"""Device time of one time-window emit (gc_ens_window_emit) next to a plain device-to-device copy, and next to the route
without it: L x M `ens_download_member` calls, one set per lead time, plus the NumPy reference on the host.
Usage: python tests/gpu_window_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child
process of its own under a time limit; the first failure ends the run.

Per case, for `sum` with L = 2 and `max` with L = 6 on 82 channels, it prints, best of REPS, the counter
"ens_window_device_us" (HIP events around the emit's launch) and the rate (L + 1) (M + 1) field / time: the emit reads
L (M + 1) fields and writes M + 1.  Next to it the time of `torch.Tensor.copy_` of (L + 1) (M + 1) fields between two device
buffers under torch.cuda events in the same process -- that copy reads AND writes (L + 1) (M + 1) fields, twice the emit's
traffic, and its rate is quoted over both -- then the host route, whose result the device's must equal bit for bit.
Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_window_timing.py --case nano50`.
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
WINDOWS = [("sum", 2), ("max", 6)]


def run(case):
  import torch
  from gencast_flax_nnx_amd import _lib, geometry
  from tests import window_reference as R
  size, M = CASES[case]
  if size == "nano":
    lat, lon, mesh = np.linspace(-90, 90, 73), np.arange(144) * 2.5, 4
  else:
    lat, lon, mesh = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0), 5
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh, attention_k_hop=8)
  G, C = gr.num_grid_nodes, 82
  mk = lambda: _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=1)
  src, win = mk(), mk()                                       # the graph only: no weights
  try:
    for h in (src, win):
      h.set_graph(gr)
      h.ens_reserve(M)
    rng = np.random.default_rng(4)
    scale = np.logspace(-3, 5, C)
    field = lambda: (rng.standard_normal((G, 1, C)) * scale).astype(np.float32)
    for i in range(M):
      src.ens_push_host(i, field())
    field_mb = G * C * 4 / 1e6
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c {C}, M {M}: a field is {field_mb:.2f} MB, a ring slot of M + 1 fields {(M + 1) * field_mb:.1f} MB")
    ok = True
    for name, L in WINDOWS:
      kind, coef = R.coefficients(name, L)
      moved_mb = (L + 1) * (M + 1) * field_mb
      a = torch.empty((L + 1) * (M + 1) * G * C, dtype=torch.float32, device="cuda")
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
      torch.cuda.empty_cache()
      win.ens_window_set(kind, L, coef)
      t_down, kept = 0.0, []
      for t in range(L):                                      # one lead time: a member moves on, the store is pushed -- and,
        src.ens_push_host(t % M, field())                     # on the route without the feature, downloaded
        win.ens_window_push(src, field())
        t0 = time.perf_counter()
        kept.append(np.stack([src.ens_download_member(i) for i in range(M)]))
        t_down += (time.perf_counter() - t0) * 1e3
      win.ens_window_emit()                                   # warm-up
      dev, host = [], []
      for _ in range(REPS):
        t0 = time.perf_counter()
        win.ens_window_emit()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(win.counter("ens_window_device_us"))
      got = np.stack([win.ens_download_member(i) for i in range(M)])
      t0 = time.perf_counter()
      ref = R.window(np.stack(kept), kind, coef)
      t_ref = (time.perf_counter() - t0) * 1e3
      same = R.same_bits(got, ref)
      ok = ok and same
      label = f"{case} {name} L={L}"
      gbs = lambda mb, us: mb / 1e3 / (max(1, us) * 1e-6)
      print(f"{label}: ring {win.counter('ens_window_ring_bytes') / 1e6:.1f} MB; the emit reads and writes {moved_mb:.1f} MB")
      print(f"{label}: gc_ens_window_emit, device               {min(dev)} us   (runs: {dev}) = {gbs(moved_mb, min(dev)):.0f} GB/s; "
            f"host wall {min(host):.3f} ms")
      print(f"{label}: plain copy of (L + 1) (M + 1) fields     {min(plain)} us   (runs: {plain}) = "
            f"{gbs(2 * moved_mb, min(plain)):.0f} GB/s read + written; the emit takes {min(dev) / max(1, min(plain)):.2f} x its time "
            f"for half its traffic")
      print(f"{label}: {L} x {M} x ens_download_member             {t_down:.1f} ms")
      print(f"{label}: NumPy reference                          {t_ref:.1f} ms   ({os.cpu_count()} CPUs visible, "
            f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
      print(f"{label}: the window members equal the reference bit for bit: {same}")
    return 0 if ok else 1
  finally:
    src.close()
    win.close()


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
