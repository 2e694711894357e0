"""The f16x3 domain guard at every intermediate operand (table and terms: tests/domain_cases.py; the table itself is
checked on the CPU by tests/test_domain_cases.py).

The kernels never clamp: an operand beyond +-65504 must poison the output of the call, and the poisoned call must be
re-run on the exact-f32 kernels ("never silently altered", csrc/gc_dev_common.inc).  Every row of
the table puts one operand of one kernel form out of range (out: the call is re-run, exactly once, and gives the
oracle's finite answer) and next to it just inside (in: no re-run, same bound); two rows put a value out of range that
is never split (no re-run).  A kernel form that lost or laundered the poison would return a finite, wrong result without
a re-run: `range_fallbacks` and the bound against the float64 oracle both see that.

The static embedders (site k) are computed once, in gc_finalize and when the precision or feature mode changes, not in
the call: out of range there, the embeddings are recomputed on the exact-f32 kernels at once
(`static_embedding_fallbacks`), and calls on that handle behave like calls on any other.

Out of scope: the fp16-feature mode -- there an overflow is the reference's own behaviour (oracle: feature_dtype).

No test sets a tuning variable; every handle comes from helpers.make_native and is closed in `finally`.
"""
import numpy as np
import pytest

from oracle import gencast_oracle as O
from tests import domain_cases as DC
from tests import helpers

pytestmark = pytest.mark.gpu
TOL = DC.TOL


def _handle(case, res):
  gr, dims, _, x, sigma, _, _ = DC.setup(case.shape)
  nd = helpers.make_native(gr, dims, res["params"], x.shape[1])
  return nd, x, sigma


def _within_bound(tag, y, y_ref):
  assert np.isfinite(y).all(), tag
  err, scale = float(np.abs(y - y_ref).max()), max(1.0, float(np.abs(y_ref).max()))
  print(f"{tag}: max |y - y_oracle| {err:.3g}, bound {TOL * scale:.3g}")
  assert err < TOL * scale, (tag, err, TOL * scale)


@pytest.mark.parametrize("case_id", [c.id for c in DC.PAIRS if not c.static])
def test_out_of_range_operand_is_rerun_and_in_range_one_is_not(case_id):
  case = DC.BY_ID[case_id]
  for which, reruns in (("out", 1), ("in", 0)):
    res = DC.evaluate(case_id, which)
    nd, x, sigma = _handle(case, res)
    try:
      assert nd.counter("weights_f16_unsafe") == 0
      before = nd.counter("range_fallbacks")
      y = nd.denoise(x, sigma)
      assert nd.counter("range_fallbacks") - before == reruns, (case_id, which)
      _within_bound(f"{case_id} {which}", y, res["y"])
    finally:
      nd.close()


@pytest.mark.parametrize("case_id", [c.id for c in DC.NOFALLBACK])
def test_out_of_range_values_that_are_never_split_are_not_rerun(case_id):
  case, res = DC.BY_ID[case_id], DC.evaluate(case_id, "nofallback")
  nd, x, sigma = _handle(case, res)
  try:
    assert nd.counter("weights_f16_unsafe") == 0
    y = nd.denoise(x, sigma)
    assert nd.counter("range_fallbacks") == 0
    _within_bound(case_id, y, res["y"])
  finally:
    nd.close()


@pytest.mark.parametrize("shape", ["A", "B", "C", "D", "E"])
def test_a_rerun_leaves_nothing_behind(shape):
  """In range, out of range (one un-normalised input channel), in range again: the third result is the first, bit for
  bit -- the exact-f32 re-run shares every buffer with the f16x3 forward and must leave no state behind."""
  gr, dims, params, x, sigma, _, _ = DC.setup(shape)
  nd = helpers.make_native(gr, dims, params, x.shape[1])
  try:
    y1 = nd.denoise(x, sigma)
    assert nd.counter("range_fallbacks") == 0
    big = x.copy()
    big[:, :, 3] *= 2.0e5
    y2 = nd.denoise(big, sigma)
    assert nd.counter("range_fallbacks") == 1 and np.isfinite(y2).all()
    y3 = nd.denoise(x, sigma)
    assert nd.counter("range_fallbacks") == 1
    np.testing.assert_array_equal(y3, y1)
  finally:
    nd.close()


@pytest.mark.parametrize("case_id", [c.id for c in DC.PAIRS if c.static])
def test_static_embedder_out_of_range(case_id):
  """A static embedder's hidden activation beyond 65504 with every weight inside: the embeddings are made at gc_finalize
  (and again when the precision changes) and every call reads them, the exact-f32 re-run of a call included -- poisoned
  embeddings would make every call of the handle return NaN whatever kernels it runs on."""
  case = DC.BY_ID[case_id]
  res = DC.evaluate(case_id, "out")
  nd, x, sigma = _handle(case, res)
  try:
    assert nd.counter("weights_f16_unsafe") == 0
    assert nd.counter("static_embedding_fallbacks") == 1
    for name in ("m0_hat", "e0_hat", "f0_hat"):
      assert np.isfinite(nd.debug_fetch(name)).all(), name
    y = nd.denoise(x, sigma)
    _within_bound(f"{case_id} out", y, res["y"])
    assert nd.counter("range_fallbacks") == 0                  # the call itself has nothing out of range: like any other handle
    np.testing.assert_array_equal(nd.denoise(x, sigma), y)
    nd.set_option("precision", "f32")
    _within_bound(f"{case_id} out, precision f32", nd.denoise(x, sigma), res["y"])
    assert nd.counter("static_embedding_fallbacks") == 1       # (made on the exact-f32 kernels in the first place)
    nd.set_option("precision", "f16x3")
    assert nd.counter("static_embedding_fallbacks") == 2
    np.testing.assert_array_equal(nd.denoise(x, sigma), y)
    assert nd.counter("range_fallbacks") == 0
  finally:
    nd.close()
  res = DC.evaluate(case_id, "in")
  nd, x, sigma = _handle(case, res)
  try:
    assert nd.counter("weights_f16_unsafe") == 0 and nd.counter("static_embedding_fallbacks") == 0
    _within_bound(f"{case_id} in", nd.denoise(x, sigma), res["y"])
    assert nd.counter("range_fallbacks") == 0
  finally:
    nd.close()


@pytest.mark.parametrize("case_id", ["A-g-ffw_hidden", "A-e-k", "C-g-ffw_hidden", "Cq-e-k"])
def test_sampler_reruns_a_poisoned_sample_also_as_a_graph_replay(case_id):
  """Every denoiser call of the sample has the operand out of range.  The first sample of a signature runs eagerly, the
  second is captured and replayed (the poisoned f16x3 sample and its exact-f32 re-run alike): one re-run per sample, the
  same bits, the oracle's sampler within the bound."""
  case, res = DC.BY_ID[case_id], DC.evaluate(case_id, "out")
  gr, dims, _, x, _, _, _ = DC.setup(case.shape)
  slots = np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32)
  noise = np.random.default_rng(5).standard_normal((gr.num_grid_nodes, x.shape[1], dims.c_out))
  sig = O.noise_schedule(80.0, 0.03, 3, 7.0)
  nd, _, _ = _handle(case, res)
  try:
    nd.set_option("graphs", "on")
    nd.set_noisy_slots(slots)
    out1, st = nd.sample(x, noise, sig)
    assert nd.counter("range_fallbacks") == 1 and st["denoiser_calls"] == 5
    out2, _ = nd.sample(x, noise, sig)
    assert nd.counter("range_fallbacks") == 2
    assert nd.counter("graph_replays") >= 1
    np.testing.assert_array_equal(out2, out1)
    net = lambda f, s: DC.forward(case, res["params"], f, s)
    ref, _ = O.dpm_solver_2s_sample(net, x.astype(np.float64), slots, noise, sig, skip_dead_call=True)
    assert np.isfinite(out1).all()
    err, bound = float(np.abs(out1 - ref).max()), TOL * max(1.0, float(np.abs(ref).max()))
    print(f"{case_id} sample: max |x - x_oracle| {err:.3g}, bound {bound:.3g}")
    assert err < bound
  finally:
    nd.close()


def test_loss_reruns_a_poisoned_evaluation():
  """tests/test_gpu_loss.py::test_out_of_range_conditioning_takes_the_exact_f32_kernels with the FFW hidden activation
  out of range instead of an input channel."""
  from tests import test_gpu_loss as TL
  case = DC.BY_ID["A-g-ffw_hidden"]
  res = DC.evaluate(case.id, "out")
  gr, dims, _, x, _, _, _ = DC.setup("A")
  rng = np.random.default_rng(121)
  targets = rng.standard_normal((gr.num_grid_nodes, 2, dims.c_out)).astype(np.float32)
  noise = rng.standard_normal((gr.num_grid_nodes, 2, dims.c_out)).astype(np.float32)
  weights = TL._tiny_weights()
  nd = helpers.make_native(gr, dims, res["params"], 2)
  nd32 = helpers.make_native(gr, dims, res["params"], 2, precision="f32")
  try:
    TL._ready(nd, dims, weights)
    TL._ready(nd32, dims, weights)
    loss, pg = nd.loss(x, targets, noise, TL.SIGMA_ENDS)
    assert nd.counter("range_fallbacks") == 1
    network = lambda f, s: DC.forward(case, res["params"], f, s)
    ref_loss, ref_pg, _ = TL._reference(weights, x, targets, noise, TL.SIGMA_ENDS, TL._slots(dims), network)
    TL._assert_within_bound("guard vs oracle", loss, pg, ref_loss, ref_pg, TL.SIGMA_ENDS, weights[3], TOL)
    loss32, pg32 = nd32.loss(x, targets, noise, TL.SIGMA_ENDS)
    assert nd32.counter("range_fallbacks") == 0
    TL._assert_within_bound("guard vs the f32 handle", loss, pg, loss32.astype(np.float64), pg32.astype(np.float64),
                            TL.SIGMA_ENDS, weights[3], TOL)
    # several evaluations in one call, all poisoned: every one is re-run and counted
    nd.upload_cond(x)
    many = nd.loss_resident(np.stack([TL.SIGMA_ENDS, TL.SIGMA_ENDS[::-1]]))
    assert nd.counter("range_fallbacks") == 3
    np.testing.assert_array_equal(many[0][0], loss)
  finally:
    nd.close()
    nd32.close()
