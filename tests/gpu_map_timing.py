"""Device time of the score maps (gc_ens_map_accumulate, gc_ens_map_accumulate_events) next to two things for the same store:
gc_ens_score, and the route without the unit -- M `ens_download_member` calls plus the NumPy reference on the host, with the
running sums kept there.
Usage: python tests/gpu_map_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child
process of its own under a time limit; the first abnormal exit ends the run.

Per case, for all 82 channels and for a 3-channel subset, it prints the counter "ens_map_device_us" (HIP events around the
pass; best of REPS) and the rate the traffic by arithmetic implies: per selected point 4 M + 4 bytes of members and truth
and 120 bytes of accumulators read and written (six doubles and three uint32, both ways); for the event pass with T = 2, per
selected point and threshold 1 code byte and 40 bytes of planes.  Beside it "ens_score_device_us" of the same store in the same
process, the ratio of the two against the ratio of their bytes, and the host route.  No time is fixed in advance and none is
asserted; the planes are compared with the reference byte for byte.  Kernel-level times: `rocprofv3 --kernel-trace --stats --
python tests/gpu_map_timing.py --case nano50`.
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
SUBSET = [0, 40, 81]


def run(case):
  from gencast_flax_nnx_amd import _lib, geometry
  from gencast_flax_nnx_amd.verification import quantize_node_weights
  from tests import map_reference as R
  size, M = CASES[case]
  if size == "nano":
    lat, lon, mesh, hw = np.linspace(-90, 90, 73), np.arange(144) * 2.5, 4, dict(latent_size=256, d_model=256, num_heads=4)
  else:
    lat, lon, mesh, hw = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0), 5, dict(latent_size=512, d_model=512, num_heads=4)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh, attention_k_hop=8)
  G, C, T = gr.num_grid_nodes, 82, 2
  nd = _lib.NativeDenoiser(ffw_hidden=2048, num_layers=1, c_in=C + 4, c_out=C, batch=1, **hw)   # the graph only: no weights
  try:
    nd.set_graph(gr)
    rng = np.random.default_rng(4)
    scale = np.logspace(-2, 4, C)
    members = (rng.standard_normal((M, G, 1, C)) * scale).astype(np.float32)
    truth = (rng.standard_normal((G, 1, C)) * scale).astype(np.float32)
    w = rng.uniform(0.1, 2.0, G).astype(np.float32)
    thr = (np.array([0.8, -0.8])[:, None, None, None] * np.broadcast_to(scale, (T, G, 1, C))).astype(np.float32)
    nd.ens_reserve(M)
    nd.ens_set_node_weight(w)
    for i in range(M):
      nd.ens_push_host(i, members[i])
    nd.ens_score(truth)                                          # warm-up; the truth stays on the device
    score = []
    for _ in range(REPS):
      nd.ens_score(None)
      score.append(nd.counter("ens_score_device_us"))
    nd.ens_event_set(thr, (+1, -1), quantize_node_weights(w)[0])
    nd.ens_event_score(None)
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_out {C}, M {M}: a field is {G * C * 4 / 1e6:.2f} MB")
    print(f"{case}: gc_ens_score, device                          {min(score)} us   (runs: {score})")
    score_bytes = (4 * M + 4) * G * C
    t0 = time.perf_counter()
    down = np.stack([nd.ens_download_member(i) for i in range(M)])
    t_down = (time.perf_counter() - t0) * 1e3
    same = True
    for name, channels in (("all 82 channels", None), ("3 channels", SUBSET)):
      n_sel = G * (C if channels is None else len(channels))
      nd.ens_map_set(channels, 1, T)
      nd.ens_map_accumulate(0)                                   # warm-up
      dev = []
      for _ in range(REPS):
        nd.ens_map_accumulate(0)
        dev.append(nd.counter("ens_map_device_us"))
      blocks = nd.counter("ens_map_blocks")
      evt = []
      for _ in range(REPS):
        nd.ens_map_accumulate_events(0)
        evt.append(nd.counter("ens_map_device_us"))
      got = nd.ens_map_download(0)
      t0 = time.perf_counter()
      sums, counts = R.empty(G, 1, C if channels is None else len(channels))
      for _ in range(REPS + 1):
        R.accumulate(sums, counts, down, truth, channels)
      t_ref = (time.perf_counter() - t0) * 1e3 / (REPS + 1)
      ok = got[0].tobytes() == sums.tobytes() and got[1].tobytes() == counts.tobytes() and bool((got[2][:, 0] == REPS).all())
      same = same and ok
      map_bytes = (4 * M + 4 + 120) * n_sel
      evt_bytes = T * (1 + 40) * n_sel
      us, ue = max(1, min(dev)), max(1, min(evt))
      print(f"{case}: {name}: gc_ens_map_accumulate, device        {min(dev)} us   (runs: {dev}; {blocks} workgroups) = "
            f"{map_bytes / 1e3 / us:.0f} GB/s of {map_bytes / 1e6:.1f} MB by arithmetic")
      print(f"{case}: {name}: against gc_ens_score                  {us / max(1, min(score)):.2f} x its time, "
            f"{map_bytes / score_bytes:.2f} x its bytes")
      print(f"{case}: {name}: gc_ens_map_accumulate_events T={T}      {min(evt)} us   (runs: {evt}) = "
            f"{evt_bytes / 1e3 / ue:.0f} GB/s of {evt_bytes / 1e6:.1f} MB by arithmetic")
      print(f"{case}: {name}: {M} x ens_download_member + NumPy reference   {t_down:.1f} ms + {t_ref:.1f} ms per date   "
            f"({os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
      print(f"{case}: {name}: planes equal the reference byte for byte after {REPS + 1} dates: {ok}")
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
