"""Device time of the spectral band views (gc_ens_band) next to gc_ens_spectrum of the same store -- the
analysis alone, of all channels -- and next to the route without them: M `ens_download_member` calls plus the NumPy reference
on the host.
Usage: python tests/gpu_band_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child
process of its own under a time limit; the first failure ends the run.

The plan: three bands of all 82 channels -- l = 0..6, l = 7..20 and the complement of l = 0..20, a true high-pass -- 246 derived
channels.  Per case it prints, best of REPS, the counter "ens_band_device_us" (HIP events around the call's launches), the
counter "spec_device_us" of gc_ens_spectrum, their ratio, and the host route.  The NumPy reference is timed on ONE field and
on a strided subset of the source channels (every 9th at 2.5 degrees, every 27th at 1 degree: its loops keep three arrays of
[2, lmax, n_lat, columns] doubles), and what the M + 1 fields of all channels would take is that time scaled up -- printed as
such; the device result of those columns must lie within the bound of tests/band_reference.py.
Kernel-level times: `rocprofv3 --kernel-trace --stats -- python tests/gpu_band_timing.py --case nano50`."""
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
BANDS = {"planetary": (0, 6), "synoptic": (7, 20), "small": dict(l=(0, 20), complement=True)}


def run(case):
  from gencast_flax_nnx_amd import BandSpec, SphericalAnalysis, _lib, geometry
  from tests import band_reference as R
  size, M = CASES[case]
  if size == "nano":
    lat, lon, mesh, stride = np.linspace(-90, 90, 73), np.arange(144) * 2.5, 4, 9
  else:
    lat, lon, mesh, stride = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0), 5, 27
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh, attention_k_hop=8)
  G, C, K = gr.num_grid_nodes, 82, len(BANDS)
  n_lat, n_lon = len(lat), len(lon)
  sa = SphericalAnalysis(lat, lon)
  atabs, stabs, L = sa.device_tables(), sa.synthesis_tables(), sa.lmax
  response, complement = BandSpec(BANDS).responses(L)
  plan = dict(c_src=C, response=response, complement=complement, src_channel=np.tile(np.arange(C, dtype=np.int32), K),
              band=np.repeat(np.arange(K, dtype=np.int32), C), legendre_synthesis=stabs[0], cos_s=stabs[1], sin_s=stabs[2])
  mk = lambda c: _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=c + 4, c_out=c, batch=1)
  src, view = mk(C), mk(K * C)                                  # the graph only: no weights
  try:
    for h in (src, view):
      h.set_graph(gr)
      h.ens_reserve(M)
      h.spec_set_tables(*atabs)
    rng = np.random.default_rng(4)
    scale = np.logspace(-2, 4, C)
    members = [((rng.standard_normal((G, 1, C)) + 0.5) * scale).astype(np.float32) for _ in range(M)]
    truth = ((rng.standard_normal((G, 1, C)) + 0.5) * scale).astype(np.float32)
    for i in range(M):
      src.ens_push_host(i, members[i])
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, lmax {L}, c_src {C}, c_d {K * C}, M {M}: a source field is {G * C * 4 / 1e6:.2f} MB, a band field {G * K * C * 4 / 1e6:.2f} MB")
    view.ens_band_set(**plan)
    view.ens_band(src, truth)                                   # warm-up; the truth stays in the source
    dev, host = [], []
    for _ in range(REPS):
      t0 = time.perf_counter()
      view.ens_band(src)
      host.append((time.perf_counter() - t0) * 1e3)
      dev.append(view.counter("ens_band_device_us"))
    print(f"{case} three bands of {C} channels: gc_ens_band, device       {min(dev)} us   (runs: {dev}); host wall {min(host):.3f} ms")
    src.ens_spectrum(None)                                      # warm-up
    spec = []
    for _ in range(REPS):
      src.ens_spectrum(None)
      spec.append(src.counter("spec_device_us"))
    print(f"{case} the analysis alone:          gc_ens_spectrum, device   {min(spec)} us   (runs: {spec})")
    print(f"{case}: the band views take {min(dev) / max(1, min(spec)):.2f} x the spectra of the same store "
          f"({min(dev) / (M + 1):.0f} us a field; {3 * M + 3} band fields written)")
    got = view.ens_download_member(0)
    t0 = time.perf_counter()
    down = [src.ens_download_member(i) for i in range(M)]
    t_down = (time.perf_counter() - t0) * 1e3
    chans = np.arange(0, C, stride)
    sel = np.concatenate([k * C + chans for k in range(K)])
    t0 = time.perf_counter()
    ref, tol, _ = R.band_fields(down[0], n_lat, n_lon, response, complement, plan["src_channel"][sel], plan["band"][sel], atabs, stabs)
    t_ref = (time.perf_counter() - t0) * 1e3
    print(f"{case}: {M} x ens_download_member      {t_down:.1f} ms")
    print(f"{case}: NumPy reference              {t_ref:.1f} ms for ONE field and {len(chans)} of {C} channels ({len(sel)} derived columns); "
          f"scaled to {M + 1} fields of all channels: {t_ref * (M + 1) * C / len(chans) / 1e3:.1f} s   ({os.cpu_count()} CPUs visible, "
          f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
    R.check(got[..., sel], ref, tol, f"{case}: member 0, the {len(sel)} columns of the reference")
    return 0
  finally:
    src.close()
    view.close()


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
