"""Device time of one denoising-loss evaluation (gc_loss_resident) next to one denoiser call inside a sample, on the
same handle.  Usage: python tests/gpu_loss_timing.py [nano] [one_degree]   (default: both)

Per size it prints the HIP-event time of a 20-level sample divided by its 39 denoiser calls (a graph replay, the
form bench.py times), the HIP-event time of N_EVAL back-to-back loss evaluations divided by N_EVAL (counter
"loss_device_us": eager launches, so it contains whatever the host could not hide), the host time of that call
(uploads of the noise levels and the one download included), and what the launches filed under gc_pack cost inside
an evaluation: the three added passes + the domain guard's finite check + the forward's own affine-rows launch.
Kernel-level times of the added passes: run it under `rocprofv3 --kernel-trace --stats -- python tests/gpu_loss_timing.py nano`.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gencast_flax_nnx_amd import _lib, losses, synthetic  # noqa: E402
from oracle import gencast_oracle as O  # noqa: E402
from tests import helpers  # noqa: E402

N_EVAL = int(os.environ.get("N_EVAL", "20"))
REPS = 3


def run(size):
  if size == "nano":
    gr, dims, params, x, _ = helpers.nano_setup()
    lat, lon = synthetic.grid_2p5deg()
  else:
    gr, dims, params, x, _ = helpers.one_degree_setup()
    lat, lon = synthetic.grid_1deg()
  plan = losses.loss_plan(synthetic.make_example(lat, lon)[1])
  nd = helpers.make_native(gr, dims, params, 1)
  try:
    if os.environ.get("GC_FEATURES"):
      nd.set_option("features", os.environ["GC_FEATURES"])
    rng = np.random.default_rng(2)
    shape = (gr.num_grid_nodes, 1, dims.c_out)
    nd.set_noisy_slots(np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32))
    nd.loss_set_weights(plan.node_weight, plan.channel_weight, plan.channel_group, plan.group_weight)
    nd.upload_cond(x)
    nd.upload_noise(rng.standard_normal(shape).astype(np.float32))
    nd.upload_targets(rng.standard_normal(shape).astype(np.float32))
    sched = O.noise_schedule(80.0, 0.03, 20, 7.0).astype(np.float32)
    per_call = []
    for i in range(2 + REPS):                    # eager, capture, then replays
      st = nd.sample_resident(sched)
      if i >= 2:
        per_call.append(st["device_ms"] / st["denoiser_calls"])
    nd.sync()
    sig = np.exp(np.random.default_rng(3).uniform(np.log(0.02), np.log(88.0), (N_EVAL, 1))).astype(np.float32)
    nd.loss_resident(sig[:2])                    # warm-up
    dev, host = [], []
    for _ in range(REPS):
      t0 = time.perf_counter()
      loss, _ = nd.loss_resident(sig)
      host.append((time.perf_counter() - t0) * 1e3 / N_EVAL)
      dev.append(nd.counter("loss_device_us") / 1e3 / N_EVAL)
    pack = nd.kernel_classes().index("gc_pack")
    nd.profile_enable(pack)
    nd.loss_resident(sig)
    launches, ms = nd.profile_read()
    nd.profile_enable(-1)
    moved = 6 * np.prod(shape) * 4 / 1e6         # noisy: t, n -> x (+ the slots of xp); reduce: F, t, n
    print(f"{size}: build {_lib.load_library().gc_build_info().decode()}")
    print(f"{size}: denoiser call inside a sample (graph replay)  {min(per_call):.3f} ms   (runs: {', '.join(f'{v:.3f}' for v in per_call)})")
    print(f"{size}: loss evaluation, device                        {min(dev):.3f} ms   (runs: {', '.join(f'{v:.3f}' for v in dev)}; {N_EVAL} evaluations per call)")
    print(f"{size}: loss evaluation, host wall                     {min(host):.3f} ms   (runs: {', '.join(f'{v:.3f}' for v in host)})")
    print(f"{size}: gc_pack launches inside an evaluation          {launches / N_EVAL:.1f} launches, {ms / N_EVAL * 1e3:.1f} us per evaluation "
          f"(the added passes move {moved:.1f} MB)")
    print(f"{size}: loss range {float(loss.min()):.4g} .. {float(loss.max()):.4g}, range_fallbacks {nd.counter('range_fallbacks')}")
  finally:
    nd.close()


if __name__ == "__main__":
  for name in (sys.argv[1:] or ["nano", "one_degree"]):
    run(name)
