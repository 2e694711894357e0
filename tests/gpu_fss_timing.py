"""Device time of the fractions sums (gc_ens_fss_score, S = 4 scales: 0, 200, 500 and 2000 km, at T = 1 and T = 4 thresholds)
next to three things for the same store: gc_ens_event_score, one area-mean pooling derive (gc_ens_derive, pool = mean at
500 km, per field), and the route without it -- T `ens_event_codes` downloads plus the row-and-column restatement in NumPy on
the host.
Usage: python tests/gpu_fss_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child process
of its own under a time limit; the first abnormal exit ends the run.

Per case it prints the counter "ens_fss_device_us" (HIP events around the row, column and finish passes of every threshold;
best of REPS), "ens_event_device_us" of the same store in the same process, "ens_derive_device_us" divided by the M + 1 fields
it pools, and the host route.  No time is fixed in advance and none is asserted.  The relation it reports is the one the
design expects: a four-scale call per threshold against one pooled mean of one field.  Kernel-level times, row pass against
column pass: `rocprofv3 --kernel-trace --stats -- python tests/gpu_fss_timing.py --case nano50`.
"""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"nano8": ("nano", 8), "nano50": ("nano", 50), "one_degree8": ("one_degree", 8)}
LIMIT_S = {"nano8": 240, "nano50": 420, "one_degree8": 540}
REPS = 3
T_MAX = 4
SCALES_KM = (0.0, 200.0, 500.0, 2000.0)


def numpy_sums(code, M, n_lat, n_lon, r_lats, r_lons, row_wq, wq):
  """The definition by prefix sums along the longitude and along the latitude, whole arrays at a time: code [G, W] uint8 ->
  sums [S, W, 4].  The integers are exact (int64); the four sums are NumPy's pairwise ones."""
  grid = code.reshape(n_lat, n_lon, -1)
  valid = grid != 255
  f = np.stack([np.where(valid, grid & 127, 0), np.where(valid, grid >> 7, 0), valid]).astype(np.int64)
  cs = np.concatenate([np.zeros_like(f[:, :, :1]), np.cumsum(np.concatenate([f, f, f], axis=2), axis=2)], axis=2)
  rows_i = np.arange(n_lat)[:, None]
  j = np.arange(n_lon)[None, :]
  w = np.asarray(wq, np.float64).reshape(n_lat, n_lon, 1)
  out = np.zeros((len(r_lats), grid.shape[2], 4))
  for s, r_lat in enumerate(r_lats):
    r = np.asarray(r_lons[s], np.int64)[:, None]
    rows = cs[:, rows_i, n_lon + j + r + 1] - cs[:, rows_i, n_lon + j - r]          # [3, n_lat, n_lon, W]
    cw = np.cumsum(rows * np.asarray(row_wq, np.int64)[None, :, None, None], axis=1)
    cw = np.concatenate([np.zeros_like(cw[:, :1]), cw], axis=1)
    i1 = np.minimum(n_lat - 1, np.arange(n_lat) + int(r_lat)) + 1
    i0 = np.maximum(0, np.arange(n_lat) - int(r_lat))
    A, B, N = cw[:, i1] - cw[:, i0]
    with np.errstate(invalid="ignore", divide="ignore"):
      P = np.where(valid, A.astype(np.float64) / (np.float64(M) * N.astype(np.float64)), 0.0)
      O = np.where(valid, B.astype(np.float64) / N.astype(np.float64), 0.0)
    wv = np.where(valid, w, 0.0)
    out[s] = np.stack([(wv * ((P - O) * (P - O))).sum(axis=(0, 1)), (wv * (P * P + O * O)).sum(axis=(0, 1)),
                       (wv * P).sum(axis=(0, 1)), (wv * O).sum(axis=(0, 1))], axis=-1)
  return out


def run(case):
  from gencast_flax_nnx_amd import _lib, geometry, losses
  from gencast_flax_nnx_amd.verification import DerivedSpec, quantize_node_weights, quantize_row_weights
  size, M = CASES[case]
  if size == "nano":
    lat, lon, mesh, hw = np.linspace(-90, 90, 73), np.arange(144) * 2.5, 4, dict(latent_size=256, d_model=256, num_heads=4)
  else:
    lat, lon, mesh, hw = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0), 5, dict(latent_size=512, d_model=512, num_heads=4)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh, attention_k_hop=8)
  G, C, n_lat, n_lon = gr.num_grid_nodes, 82, len(lat), len(lon)
  mk = lambda: _lib.NativeDenoiser(ffw_hidden=2048, num_layers=1, c_in=C + 4, c_out=C, batch=1, **hw)   # the graph only: no weights
  nd, view = mk(), mk()
  try:
    nd.set_graph(gr)
    view.set_graph(gr)
    rng = np.random.default_rng(4)
    scale = np.logspace(-2, 4, C)
    members = (rng.standard_normal((M, G, 1, C)) * scale).astype(np.float32)
    truth = (rng.standard_normal((G, 1, C)) * scale).astype(np.float32)
    offset = np.linspace(0.5, 2.0, T_MAX)[:, None, None, None]
    thr = (np.broadcast_to(offset, (T_MAX, G, 1, C)) * scale).astype(np.float32)
    dirs = np.ones(T_MAX, np.int32)
    area = np.asarray(losses.normalized_latitude_weights(lat), np.float64)
    wq, _ = quantize_node_weights(np.repeat(area, n_lon))
    row_wq = quantize_row_weights(area)
    windows = [DerivedSpec.window(lat, lon, r) for r in SCALES_KM]
    r_lats, r_lons = np.array([w[0] for w in windows], np.int32), np.stack([w[1] for w in windows]).astype(np.int32)
    nd.ens_reserve(M)
    for i in range(M):
      nd.ens_push_host(i, members[i])
    nd.ens_fss_set(r_lats, r_lons, row_wq)
    field_mb = G * C * 4 / 1e6
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G} = {n_lat} x {n_lon}, c_out {C}, M {M}: a field is {field_mb:.2f} MB, its codes {field_mb / 4:.2f} MB; "
          f"r_lat {r_lats.tolist()}, r_lon at the equator {r_lons[:, n_lat // 2].tolist()}")
    # one pooled mean of the same store, per field
    view.ens_reserve(M)
    view.ens_derive_set(c_src=C, op=np.zeros(C, np.int32), src_a=np.arange(C, dtype=np.int32), src_b=np.zeros(C, np.int32),
                        affine=np.tile([1.0, 0.0, 1.0, 0.0], (C, 1)), pool=3, n_lat=n_lat, n_lon=n_lon, r_lat=int(r_lats[2]),
                        r_lon=r_lons[2], row_weight=area)
    view.ens_derive(nd, truth)
    derive = []
    for _ in range(REPS):
      view.ens_derive(nd, None)
      derive.append(view.counter("ens_derive_device_us"))
    per_field = min(derive) / (M + 1)
    print(f"{case}: gc_ens_derive pool = mean at 500 km, device     {min(derive)} us for M + 1 = {M + 1} fields = {per_field:.1f} us per field "
          f"(runs: {derive})")
    same = True
    for T in (1, T_MAX):
      nd.ens_event_set(thr[:T], dirs[:T], wq)
      nd.ens_event_score(truth)
      nd.ens_fss_score()                                           # warm-up: makes the work buffers
      evt, dev, host = [], [], []
      for _ in range(REPS):
        nd.ens_event_score(None)
        evt.append(nd.counter("ens_event_device_us"))
        t0 = time.perf_counter()
        got = nd.ens_fss_score()
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(nd.counter("ens_fss_device_us"))
      t0 = time.perf_counter()
      codes = [nd.ens_event_codes(t) for t in range(T)]
      t_down = (time.perf_counter() - t0) * 1e3
      t0 = time.perf_counter()
      ref = np.stack([numpy_sums(c.reshape(G, C), M, n_lat, n_lon, r_lats, r_lons, row_wq, wq) for c in codes])
      t_ref = (time.perf_counter() - t0) * 1e3
      ref = ref.reshape(got.shape)
      ok = bool(np.all(np.abs(got - ref) <= 2.0 * (G * 2.0 ** -53 * ref + np.spacing(ref))))       # two orders of addition
      same = same and ok
      print(f"{case}: gc_ens_event_score T={T}, device                 {min(evt)} us   (runs: {evt})")
      print(f"{case}: gc_ens_fss_score T={T} S=4, device               {min(dev)} us   (runs: {dev}) = {min(dev) / T:.1f} us per threshold; "
            f"{min(dev) / max(1, min(evt)):.2f} x gc_ens_event_score, {min(dev) / T / per_field:.2f} x one pooled mean of one field")
      print(f"{case}: gc_ens_fss_score T={T} S=4, host wall            {min(host):.3f} ms")
      print(f"{case}: {T} x ens_event_codes + NumPy prefix sums S=4       {t_down:.1f} ms + {t_ref:.1f} ms   "
            f"({os.cpu_count()} CPUs visible, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
      print(f"{case}: T={T}: sums within twice the bound of the NumPy route: {ok}")
    return 0 if same else 1
  finally:
    nd.close()
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
