"""Device time of the power spectra of an ensemble (gc_ens_spectrum) next to the route without it: M `download_sample`
calls plus the NumPy float64 reference on the host.  Usage: python tests/gpu_spectrum_timing.py [nano8] [nano50]
[one_degree8] (default: all three).  Each case runs in a child process of its own under a time limit; the first failure
ends the run.

Per case it prints the counter "spec_device_us" (HIP events around all kernels of the call: M + 1 analyses, the mean
and the sums; best of REPS), the same for one field (gc_spec_field), the binary64 rate the arithmetic count implies, the
host wall time of the call, and the host route: M downloads of a resident sample and tests/spectrum_reference.py.  The
reference is timed on REF_COLS of the 82 columns (its loops are vectorised over the columns, so the time is scaled by
82 / REF_COLS and printed as an estimate); the device result of those columns is checked against it.
Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_spectrum_timing.py --case nano50`.
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
GRID = {"nano": (73, 144), "one_degree": (181, 360)}
REF_COLS = {"nano8": 82, "nano50": 10, "one_degree8": 2}
REPS = 3


def run(case):
  from gencast_flax_nnx_amd import SphericalAnalysis, _lib
  from oracle import gencast_oracle as O
  from tests import helpers
  from tests import spectrum_reference as R
  size, M = CASES[case]
  n_lat, n_lon = GRID[size]
  gr, dims, params, x, _ = helpers.nano_setup() if size == "nano" else helpers.one_degree_setup()
  nd = helpers.make_native(gr, dims, params, 1)
  try:
    G, C = gr.num_grid_nodes, dims.c_out
    assert G == n_lat * n_lon
    t0 = time.perf_counter()
    tabs = SphericalAnalysis(np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)).device_tables()
    t_tab = (time.perf_counter() - t0) * 1e3
    L = tabs[0].shape[0]
    rng = np.random.default_rng(4)
    members = rng.standard_normal((M, G, 1, C)).astype(np.float32)
    truth = rng.standard_normal((G, 1, C)).astype(np.float32)
    nd.spec_set_tables(*tabs)
    nd.ens_reserve(M)
    for i in range(M):
      nd.ens_push_host(i, members[i])
    nd.ens_spectrum(truth)                                       # warm-up; the truth stays on the device
    dev, one, host = [], [], []
    for _ in range(REPS):
      t0 = time.perf_counter()
      sums = nd.ens_spectrum(None)
      host.append((time.perf_counter() - t0) * 1e3)
      dev.append(nd.counter("spec_device_us"))
      nd.spec_field(truth)
      one.append(nd.counter("spec_device_us"))
    # the route without the device transform: a resident sample downloaded M times, then NumPy
    nd.set_noisy_slots(np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32))
    nd.upload_cond(x)
    nd.upload_noise(rng.standard_normal((G, 1, C)).astype(np.float32))
    nd.sample_resident(O.noise_schedule(80.0, 0.03, 2, 7.0).astype(np.float32))
    nd.download_sample()
    t0 = time.perf_counter()
    for _ in range(M):
      nd.download_sample()
    t_down = (time.perf_counter() - t0) * 1e3
    nc = REF_COLS[case]
    cols = list(range(0, C, C // nc))[:nc]
    t0 = time.perf_counter()
    ref = R.ensemble(members, truth, n_lat, n_lon, tabs, cols=cols)
    t_ref = (time.perf_counter() - t0) * 1e3
    got = sums.reshape(C, L, 6)[cols]
    ok = bool(np.all(np.abs(got - ref["sums"]) <= ref["tol"]))
    # multiply-adds of one field: Fourier 2 L n_lon per (lat, column), Legendre n_lat per existing (part, m, l, column)
    flop = 2.0 * C * (2 * L * n_lon * n_lat + 2 * n_lat * L * (L + 1) / 2)
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G} ({n_lat} x {n_lon}), c_out {C}, lmax {L}, M {M}; tables built on the host in {t_tab:.0f} ms")
    print(f"{case}: gc_ens_spectrum, device           {min(dev)} us   (runs: {dev}) = {(M + 1) * flop / (min(dev) * 1e-6) / 1e12:.2f} TFLOP/s binary64 over {M + 1} fields")
    print(f"{case}: gc_spec_field (one field), device {min(one)} us   (runs: {one}) = {flop / 1e9:.2f} GFLOP")
    print(f"{case}: gc_ens_spectrum, host wall        {min(host):.3f} ms")
    print(f"{case}: {M} x download_sample               {t_down:.1f} ms")
    print(f"{case}: NumPy float64 reference           {t_ref:.1f} ms on {len(cols)} of {C} columns = about {t_ref * C / len(cols):.0f} ms for all"
          f"   ({os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
    print(f"{case}: device sums within the tests' bound of the reference on those columns: {ok}")
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
