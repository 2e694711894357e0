"""Device time of the regional ensemble scores (gc_ens_region_score) for three plans -- R = 1 with all nodes, R = 8 (four
latitude bands, each split into land and sea, overlapping on the rows the inclusive bounds share) and a single box of about
10 % of the nodes -- next to one gc_ens_score pass over the same store and next to the route that exists without it: R times
(`ens_set_node_weight` with masked weights + `ens_score`).
Usage: python tests/gpu_region_timing.py [nano8] [nano50] [one_degree8]   (default: all three).  Each case runs in a child
process of its own under a time limit; the first abnormal exit ends the run.

Per case and plan it prints the counter "ens_region_device_us" (HIP events around the pass and the finish; best of REPS), its
ratio to "ens_score_device_us" of the same store in the same process, the share of the nodes the plan lists, and for the
masked route the sum of the R "ens_score_device_us" and the host wall time of the R pairs of calls.  No time is fixed in
advance and none is asserted.  The expectation it lets one check: R = 8 costs about one gc_ens_score pass, the box about its
share of the nodes.  The sums with non-negative terms (S0, S2..S5) of both routes are compared within the two bounds of
section 8c added; S1 is left out because the masked route has no absolute sum to scale its bound with.
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


def plans(lat, lon, rng):
  """{name: (node_bits [G] uint32, R)} on the grid of `lat` x `lon`."""
  from gencast_flax_nnx_amd import datasets
  from gencast_flax_nnx_amd.verification import RegionSpec
  dims = ("batch", "time", "lat", "lon")
  t = datasets.Dataset({"x": datasets.Variable(dims, np.zeros((1, 1, len(lat), len(lon)), np.float32))}, {"lat": lat, "lon": lon})
  land = rng.random((len(lat), len(lon))) < 0.3                  # a synthetic land-sea mask: 30 % land, scattered
  bands = RegionSpec.from_bounds(t, {"s_extra": dict(lat=(-90, -20)), "s_tropics": dict(lat=(-20, 0)),
                                     "n_tropics": dict(lat=(0, 20)), "n_extra": dict(lat=(20, 90))})
  eight = {}
  for name, m in bands.masks.items():
    eight[name + "_land"], eight[name + "_sea"] = m & land, m & ~land
  box = RegionSpec.from_bounds(t, {"box": dict(lat=(20, 65), lon=(-40, 100))})
  return {"R=1 all nodes": (RegionSpec({"all": np.ones(land.shape, bool)}).node_bits(t), 1),
          "R=8 bands x land/sea": (RegionSpec(eight).node_bits(t), 8), "R=1 box": (box.node_bits(t), 1)}


def run(case):
  from gencast_flax_nnx_amd import _lib, geometry
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
    print(f"{case}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{case}: G {G}, c_out {C}, M {M}: a field is {G * C * 4 / 1e6:.2f} MB")
    print(f"{case}: gc_ens_score, device                      {min(score)} us   (runs: {score})")
    same = True
    factor = 2 * (G + M * M + 8) * 2.0 ** -53
    for name, (bits, R) in plans(lat, lon, rng).items():
      share = float((bits != 0).mean())
      atoms = len(np.unique(bits[bits != 0]))
      nd.ens_region_set(bits, R)
      nd.ens_region_score(None)                                  # warm-up
      dev, host = [], []
      for _ in range(REPS):
        t0 = time.perf_counter()
        got = nd.ens_region_score(None)
        host.append((time.perf_counter() - t0) * 1e3)
        dev.append(nd.counter("ens_region_device_us"))
      # the route without it: one masked weight vector and one full pass per region
      masked_dev, masked_host, ok = [], [], True
      for rep in range(REPS):
        total, t0 = 0, time.perf_counter()
        for r in range(R):
          nd.ens_set_node_weight(np.where((bits >> np.uint32(r)) & np.uint32(1), w, np.float32(0.0)).astype(np.float32))
          sums, _ = nd.ens_score(None)
          total += nd.counter("ens_score_device_us")
          if rep == 0:
            for k in (0, 2, 3, 4, 5):
              ok = ok and bool(np.all(np.abs(sums[..., k] - got[0][r, ..., k]) <= factor * np.abs(sums[..., k])))
        masked_host.append((time.perf_counter() - t0) * 1e3)
        masked_dev.append(total)
      nd.ens_set_node_weight(w)
      same = same and ok
      print(f"{case}: {name}: {share:.3f} of the nodes listed, {atoms} atoms")
      print(f"{case}: {name}: gc_ens_region_score, device     {min(dev)} us   (runs: {dev}) = {min(dev) / max(1, min(score)):.2f} x "
            f"gc_ens_score; host wall {min(host):.3f} ms")
      print(f"{case}: {name}: {R} x (set_node_weight + gc_ens_score), device {min(masked_dev)} us   (runs: {masked_dev}); "
            f"host wall {min(masked_host):.3f} ms; region / masked route, device: {min(dev) / max(1, min(masked_dev)):.3f}")
      print(f"{case}: {name}: S0, S2..S5 of both routes within the added bounds: {ok}")
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
