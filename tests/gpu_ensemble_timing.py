"""Device time of scoring an ensemble (gc_ens_score) next to the route without it: M `download_sample` calls plus the
NumPy float64 reference on the host.  Usage: python tests/gpu_ensemble_timing.py [nano8] [nano50] [one_degree8]
(default: all three).  Each case runs in a child process of its own under a time limit; the first failure ends the run.

Per case it prints the counter "ens_score_device_us" (HIP events around the score and the finish kernel; best of
REPS, with and without the mean / variance fields), the HBM rate M * field bytes / time that implies, the host wall
time of the call, and the host route: M downloads of a resident sample and tests/verification_reference.py on them.
Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_ensemble_timing.py --case nano50`.
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
  from gencast_flax_nnx_amd import _lib
  from oracle import gencast_oracle as O
  from tests import helpers
  from tests import verification_reference as R
  size, M = CASES[case]
  gr, dims, params, x, _ = helpers.nano_setup() if size == "nano" else helpers.one_degree_setup()
  nd = helpers.make_native(gr, dims, params, 1)
  try:
    G, C = gr.num_grid_nodes, dims.c_out
    rng = np.random.default_rng(4)
    members = rng.standard_normal((M, G, 1, C)).astype(np.float32)
    truth = rng.standard_normal((G, 1, C)).astype(np.float32)
    w = rng.uniform(0.1, 2.0, G).astype(np.float32)
    nd.ens_reserve(M)
    nd.ens_set_node_weight(w)
    for i in range(M):
      nd.ens_push_host(i, members[i])
    nd.ens_score(truth)                                          # warm-up; the truth stays on the device
    dev, dev_f, host = [], [], []
    for _ in range(REPS):
      t0 = time.perf_counter()
      sums, hist = nd.ens_score(None)
      host.append((time.perf_counter() - t0) * 1e3)
      dev.append(nd.counter("ens_score_device_us"))
      nd.ens_score(None, want_fields=True)
      dev_f.append(nd.counter("ens_score_device_us"))
    # the route without the device reduction: a resident sample downloaded M times, then NumPy
    nd.set_noisy_slots(np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32))
    nd.upload_cond(x)
    nd.upload_noise(rng.standard_normal((G, 1, C)).astype(np.float32))
    nd.sample_resident(O.noise_schedule(80.0, 0.03, 2, 7.0).astype(np.float32))
    nd.download_sample()
    t0 = time.perf_counter()
    for _ in range(M):
      nd.download_sample()
    t_down = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ref = R.reference(members, truth, w)
    t_ref = (time.perf_counter() - t0) * 1e3
    ok = bool(np.all(np.abs(sums - ref["sums"]) <= R.sum_tolerance(ref, G, M))) and bool(np.array_equal(hist, ref["hist"]))
    mb = M * G * C * 4 / 1e6
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_out {C}, M {M}: the members are {mb:.1f} MB")
    print(f"{case}: gc_ens_score, device              {min(dev)} us   (runs: {dev}) = {mb / 1e3 / (min(dev) * 1e-6):.0f} GB/s of member reads")
    print(f"{case}: gc_ens_score with fields, device  {min(dev_f)} us   (runs: {dev_f})")
    print(f"{case}: gc_ens_score, host wall           {min(host):.3f} ms")
    print(f"{case}: {M} x download_sample               {t_down:.1f} ms")
    print(f"{case}: NumPy float64 reference           {t_ref:.1f} ms   ({os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
    print(f"{case}: device sums within the tests' bound of the reference, histogram equal: {ok}")
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
