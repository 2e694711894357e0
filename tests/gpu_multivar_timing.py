"""Device time of the multivariate ensemble scores (gc_ens_energy_score, gc_ens_variogram_score) next to three things for
the same store: gc_ens_score, a plain device copy of M + 1 fields, and the route without them -- M `ens_download_member`
calls plus the NumPy reference on the host.
Usage: python tests/gpu_multivar_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a
child process of its own under a time limit; the first abnormal exit ends the run.

Per case it prints the counters "ens_energy_device_us" -- for one group over all 82 channels (K = 1), for eight groups
(six blocks of 13 levels, a pair, two single channels) and for 32 single-channel groups (channels 0 .. 31: the staging loads
of such a group are a whole node apart and do not coalesce) -- and "ens_variogram_device_us" (four offsets, p = 0.5), each the
HIP-event time around the pass and its finish, best of REPS; the pair-point rate of the energy pass (points x P pairs per
second); "ens_score_device_us" of the same store in the same process; and the host route.  No time is fixed in advance and
none is asserted.  Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_multivar_timing.py --case nano50`.
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
OFFSETS = [(0, 1), (1, 0), (0, 4), (4, 0)]


def run(case):
  import torch
  from gencast_flax_nnx_amd import _lib, geometry
  from tests import multivar_reference as R
  size, M = CASES[case]
  if size == "nano":
    lat, lon, mesh, hw = np.linspace(-90, 90, 73), np.arange(144) * 2.5, 4, dict(latent_size=256, d_model=256, num_heads=4)
  else:
    lat, lon, mesh, hw = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0), 5, dict(latent_size=512, d_model=512, num_heads=4)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh, attention_k_hop=8)
  G, C, P = gr.num_grid_nodes, 82, M * (M + 1) // 2
  nd = _lib.NativeDenoiser(ffw_hidden=2048, num_layers=1, c_in=C + 4, c_out=C, batch=1, **hw)   # the graph only: no weights
  try:
    nd.set_graph(gr)
    rng = np.random.default_rng(4)
    members = rng.standard_normal((M, G, 1, C)).astype(np.float32)
    truth = rng.standard_normal((G, 1, C)).astype(np.float32)
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
    one = np.zeros(C, np.int32)
    eight = np.concatenate([np.repeat(np.arange(6), 13), [6, 6], [7], [-1]]).astype(np.int32)
    single = np.where(np.arange(C) < 32, np.arange(C), -1).astype(np.int32)
    scale = np.ones(C)
    energy = {}
    for name, K, group in (("K=1", 1, one), ("K=8", 8, eight), ("K=32x1", 32, single)):
      nd.ens_energy_set(K, group, scale)
      got = nd.ens_energy_score(None)                            # warm-up: makes the partial buffers
      dev = []
      for _ in range(REPS):
        got = nd.ens_energy_score(None)
        dev.append(nd.counter("ens_energy_device_us"))
      energy[name] = (dev, got, group)
    nd.ens_variogram_set(len(lat), len(lon), OFFSETS, 0.5)
    vg = nd.ens_variogram_score(None)
    vdev, host = [], []
    for _ in range(REPS):
      t0 = time.perf_counter()
      vg = nd.ens_variogram_score(None)
      host.append((time.perf_counter() - t0) * 1e3)
      vdev.append(nd.counter("ens_variogram_device_us"))
    t0 = time.perf_counter()
    down = np.stack([nd.ens_download_member(i) for i in range(M)])
    t_down = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = R.energy(down, truth, w, eight, scale)
    t_ref_e = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    vref = R.variogram(down, truth, w, len(lat), len(lon), OFFSETS, 0.5)
    t_ref_v = (time.perf_counter() - t0) * 1e3
    same = bool(np.all(np.abs(energy["K=8"][1][0] - ref["d2"]) <= R.energy_tolerance(ref)) and energy["K=8"][1][2] == ref["invalid"])
    same = same and bool(np.all(np.abs(vg[0] - vref["sums"]) <= R.variogram_tolerance(vref, G, M)) and np.array_equal(vg[1], vref["counts"]))
    field_mb = G * C * 4 / 1e6
    read_mb = (M + 1) * field_mb
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_out {C}, M {M}, P {P}: a field is {field_mb:.2f} MB, the M + 1 fields {read_mb:.1f} MB")
    print(f"{case}: gc_ens_score, device                      {min(score)} us   (runs: {score})")
    print(f"{case}: plain copy of M + 1 fields, device        {min(plain)} us   (runs: {plain}) = "
          f"{2 * read_mb / 1e3 / (max(1, min(plain)) * 1e-6):.0f} GB/s read + written")
    for name, (dev, _, group) in energy.items():
      pts = G * int((group >= 0).sum())
      print(f"{case}: gc_ens_energy_score {name}, device          {min(dev)} us   (runs: {dev}) = "
            f"{pts * P / 1e9 / (max(1, min(dev)) * 1e-6):.1f} G pair-points/s; {min(dev) / max(1, min(score)):.2f} x gc_ens_score")
    print(f"{case}: gc_ens_variogram_score O=4, device        {min(vdev)} us   (runs: {vdev}) = "
          f"{len(OFFSETS) * 2 * read_mb / 1e3 / (max(1, min(vdev)) * 1e-6):.0f} GB/s of both ends' M + 1 fields per offset")
    print(f"{case}: gc_ens_variogram_score O=4, host wall     {min(host):.3f} ms")
    print(f"{case}: {M} x ens_download_member                  {t_down:.1f} ms")
    print(f"{case}: NumPy reference, energy K=8               {t_ref_e:.1f} ms   ({os.cpu_count()} CPUs visible, "
          f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
    print(f"{case}: NumPy reference, variogram O=4            {t_ref_v:.1f} ms")
    print(f"{case}: sums within the bounds of the reference, counts equal: {same}")
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
