"""Every branch of the fused sampler loop (csrc/gc_sampler.hip: run_sampler, sampler_body, resolve_guard) against the
float64 oracle, on the rows of tests/sampler_cases.py: launch elision with and without churn in front of a call, the dead
mid-point call, one-step samples, schedules without a trailing zero, a level below the clamp, the per-call conditioning
path and the full SigmaList next to it, capture / replay / LRU eviction of sample graphs, state changes around a captured
graph, the embed cache, and the noise stream under the domain guard's re-run.  The table is checked without a device in
tests/test_sampler_cases.py.  Every test prints the figure it asserts on; DESIGN.md section 2 holds the measured ones.
"""
import numpy as np
import pytest

from gencast_flax_nnx_amd import noise as noise_mod
from gencast_flax_nnx_amd import weights
from oracle import gencast_oracle as O
from tests import helpers
from tests import sampler_cases as SC

pytestmark = pytest.mark.gpu

IDS = [c.id for c in SC.CASES]
ELIGIBLE = [c.id for c in SC.CASES if c.graph_eligible]
INELIGIBLE = [c.id for c in SC.CASES if not c.graph_eligible]
HOST_TOL = 2e-5              # fused loop against the host-driven loop (test_sampler_matches_golden_and_host_loop)
CACHE_TOL = 2e-6             # embed cache on against off (test_sampler_with_the_cached_static_part_of_the_grid_embedding)


def _make(setup, precision=None, params=None):
  """A finalized handle of a setup with its noise tables and noisy slots set."""
  gr, dims, p0, x, lat, lon, slots, _, _ = SC.setup(setup)
  nd = helpers.make_native(gr, dims, p0 if params is None else params, x.shape[1], precision=precision)
  nd.noise_set_tables(len(lat), len(lon), *noise_mod.SphericalNoise(lat, lon).device_tables())
  nd.set_noisy_slots(slots)
  return nd


def _run(nd, case, cond=None, stream=0):
  """One sample of a row -> (result, denoiser calls, fields drawn).  `stream`: the Philox stream the handle is seeded
  with first; None leaves the handle's key and stream as they are.  Churn is switched off again afterwards."""
  _, _, _, x, _, _, _, noise, _ = SC.setup(case.setup)
  nd.set_churn(case.rates, case.inflation)
  try:
    if stream is not None:
      nd.noise_seed(SC.SEED, stream)
    s0 = nd.counter("noise_stream")
    out, st = nd.sample(x if cond is None else cond, noise, np.asarray(case.sigmas), skip_dead_call=case.skip_dead)
    return out, st["denoiser_calls"], nd.counter("noise_stream") - s0
  finally:
    nd.set_churn(None)


def _rel(out, ref):
  return float(np.abs(out - ref).max() / max(1.0, np.abs(ref).max()))


def _graphs(nd):
  return nd.counter("graph_captures"), nd.counter("graph_replays")


class _Handles:
  """Handles made on first use and closed with the module."""

  def __init__(self, make):
    self.make, self.made = make, {}

  def __call__(self, *key):
    if key not in self.made:
      self.made[key] = self.make(*key)
    return self.made[key]

  def close(self):
    for v in self.made.values():
      for nd in (v.values() if isinstance(v, dict) else [v]):
        nd.close()


@pytest.fixture(scope="module")
def handle():
  """(setup, precision) -> the handle the parity rows share."""
  h = _Handles(_make)
  yield h
  h.close()


@pytest.fixture(scope="module")
def graph_handle():
  """setup -> a handle only the eager / capture / replay rows use: every row's signature is new to it."""
  h = _Handles(_make)
  yield h
  h.close()


@pytest.fixture(scope="module")
def cache_pair():
  """setup -> {"1": handle with the embed cache, "0": handle without}; the switch is read when a handle is created."""
  def make(setup):
    pair = {}
    with pytest.MonkeyPatch.context() as mp:
      for cache in ("1", "0"):
        mp.setenv("GC_TUNE_EMBED_CACHE", cache)
        pair[cache] = _make(setup)
    return pair
  h = _Handles(make)
  yield h
  h.close()


# ---- a. parity of every row, both kernel families --------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("case_id", IDS)
def test_row_matches_the_oracle(handle, case_id, precision):
  case = SC.BY_ID[case_id]
  nd = handle(case.setup, precision)
  fallbacks = nd.counter("range_fallbacks")
  out, calls, drawn = _run(nd, case)
  ref, _, _ = SC.reference(case)
  err = _rel(out, ref)
  print(f"{case_id} [{precision}]: calls {calls}, drawn {drawn}, max |ref| {np.abs(ref).max():.4g}, error {err:.3g} of scale")
  assert calls == case.calls
  assert drawn == case.draws
  assert nd.counter("range_fallbacks") == fallbacks                           # in the f16x3 domain: the kernels asked for
  assert np.isfinite(out).all() and err < SC.TOL


# ---- b. the per-call conditioning path against the loop driven from the host ------------------------------------------

@pytest.mark.parametrize("case_id", ["calls_97", "calls_96"])
def test_long_samples_match_the_host_driven_loop(handle, case_id):
  case = SC.BY_ID[case_id]
  nd = handle("S", "f16x3")
  _, _, _, x, _, _, slots, noise, _ = SC.setup("S")
  six = SC.plain("S", SC.SIX)
  before = _run(nd, six)[0]
  out, calls, _ = _run(nd, case)
  assert calls == case.calls
  host, host_calls = O.dpm_solver_2s_sample(lambda f, s: nd.denoise(f, s), x, slots, noise,
                                            np.asarray(case.sigmas, np.float32), skip_dead_call=case.skip_dead)
  err = _rel(out, host)
  print(f"{case_id}: fused loop against the host-driven loop {err:.3g} of scale")
  assert host.dtype == np.float32 and host_calls == case.calls
  assert err < HOST_TOL
  # neither the per-call conditioning buffer nor the sample-wide one leaks into the other path
  np.testing.assert_array_equal(_run(nd, six)[0], before)
  np.testing.assert_array_equal(_run(nd, case)[0], out)


# ---- c. eager = capture = replay ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", ELIGIBLE)
def test_eligible_rows_are_captured_and_replayed_bit_for_bit(graph_handle, case_id):
  case = SC.BY_ID[case_id]
  nd = graph_handle(case.setup)
  nd.set_option("graphs", "off")
  want = _run(nd, case)[0]
  nd.set_option("graphs", "on")
  captures, replays = _graphs(nd)
  for i in range(4):                                                          # eager, capture + launch, replay, replay
    got, calls, drawn = _run(nd, case)
    np.testing.assert_array_equal(got, want)
    assert (calls, drawn) == (case.calls, 0)
  assert _graphs(nd) == (captures + 1, replays + 3)
  if case.rates is not None:                                                  # all-zero rates ARE "off": the same graph
    plain = SC.plain(case.setup, case.sigmas, case.skip_dead)
    np.testing.assert_array_equal(_run(nd, plain)[0], want)
    assert _graphs(nd) == (captures + 1, replays + 4)


@pytest.mark.parametrize("case_id", INELIGIBLE)
def test_ineligible_rows_stay_eager_and_repeat(graph_handle, case_id):
  case = SC.BY_ID[case_id]
  nd = graph_handle(case.setup)
  nd.set_option("graphs", "on")
  before = _graphs(nd)
  outs = [_run(nd, case) for _ in range(3)]                                   # the same key and stream every time
  assert _graphs(nd) == before
  for out, calls, drawn in outs:
    assert (calls, drawn) == (case.calls, case.draws)
    np.testing.assert_array_equal(out, outs[0][0])


# ---- d. embed cache on and off ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", [c.id for c in SC.CASES if c.rates is not None] + ["no_trailing_zero"])
def test_embed_cache_on_and_off_agree(cache_pair, case_id):
  case = SC.BY_ID[case_id]
  pair = cache_pair(case.setup)
  outs = {}
  for cache, nd in pair.items():
    n0 = nd.counter("embed_cache")
    outs[cache], calls, drawn = _run(nd, case)
    assert (calls, drawn) == (case.calls, case.draws)
    assert nd.counter("embed_cache") - n0 == (1 if cache == "1" else 0)       # once per sample
  err = _rel(outs["1"], outs["0"])
  print(f"{case_id}: embed cache on against off {err:.3g} of scale")
  assert np.isfinite(outs["1"]).all() and err < CACHE_TOL
  assert _rel(outs["1"], SC.reference(case)[0]) < SC.TOL


# ---- e. the least recently used signature is forgotten ------------------------------------------------------------------

def test_the_ninth_signature_evicts_the_least_recently_used_graph():
  nd = _make("T")
  try:
    rows = [SC.plain("T", SC.karras(k)) for k in range(1, 10)]
    nd.set_option("graphs", "off")
    want = [_run(nd, r)[0] for r in rows]
    assert _graphs(nd) == (0, 0)
    nd.set_option("graphs", "on")
    for r, w in zip(rows, want):                                              # eager, capture + launch
      for _ in range(2):
        out, calls, _ = _run(nd, r)
        np.testing.assert_array_equal(out, w)
        assert calls == r.calls
    assert _graphs(nd) == (9, 9)
    np.testing.assert_array_equal(_run(nd, rows[0])[0], want[0])              # forgotten: first sight again, eager
    assert _graphs(nd) == (9, 9)
    np.testing.assert_array_equal(_run(nd, rows[0])[0], want[0])              # second sight: captured
    assert _graphs(nd) == (10, 10)
    np.testing.assert_array_equal(_run(nd, rows[8])[0], want[8])              # the most recent of the nine is still there
    assert _graphs(nd) == (10, 11)
    np.testing.assert_array_equal(_run(nd, rows[1])[0], want[1])              # the second was evicted by the first's return
    assert _graphs(nd) == (10, 11)
  finally:
    nd.close()


# ---- f. state changes around a captured graph ---------------------------------------------------------------------------

SIX_T = SC.plain("T", SC.SIX)


@pytest.fixture
def replaying(request, monkeypatch):
  """(handle, its six-step sample): the sample's graph is captured and has been replayed.  With a parameter, every handle
  the test makes has the embed cache switched on ("1") or off ("0")."""
  cache = getattr(request, "param", None)
  if cache is not None:
    monkeypatch.setenv("GC_TUNE_EMBED_CACHE", cache)
  nd = _make("T")
  nd.set_option("graphs", "on")
  outs = [_run(nd, SIX_T)[0] for _ in range(3)]
  assert _graphs(nd) == (1, 2)
  np.testing.assert_array_equal(outs[0], outs[2])
  yield nd, outs[0]
  nd.close()


def _fresh(**kw):
  option = kw.pop("option", None)
  nd = _make("T", **kw)
  try:
    if option:
      nd.set_option(*option)
    return _run(nd, SIX_T)[0]
  finally:
    nd.close()


def test_a_precision_switch_and_back_keeps_the_graph(replaying):
  nd, original = replaying
  nd.set_option("precision", "f32")
  in_f32 = _run(nd, SIX_T)[0]
  np.testing.assert_array_equal(in_f32, _fresh(precision="f32"))
  assert _graphs(nd) == (1, 2) and not np.array_equal(in_f32, original)      # its own signature, first sight: eager
  nd.set_option("precision", "f16x3")
  np.testing.assert_array_equal(_run(nd, SIX_T)[0], original)
  assert _graphs(nd) == (1, 3)


def test_the_aggregate_normalization_drops_the_graph(replaying):
  nd, original = replaying
  nd.set_option("grid2mesh_aggregate_normalization", "2")
  normed = _run(nd, SIX_T)[0]
  np.testing.assert_array_equal(normed, _fresh(option=("grid2mesh_aggregate_normalization", "2")))
  assert _graphs(nd) == (1, 2) and not np.array_equal(normed, original)
  nd.set_option("grid2mesh_aggregate_normalization", "0")
  np.testing.assert_array_equal(_run(nd, SIX_T)[0], original)
  assert _graphs(nd) == (1, 2)                                                # first sight after the drop: eager
  np.testing.assert_array_equal(_run(nd, SIX_T)[0], original)
  assert _graphs(nd) == (2, 3)


@pytest.mark.parametrize("replaying", ["1", "0"], indirect=True, ids=["embed_cache_on", "embed_cache_off"])
def test_other_weights_are_not_served_by_the_stale_graph(replaying, request):
  """gc_finalize re-makes the weight images, so the captured graph must go.  Two lines drop it: build_embed_cache, which
  gc_finalize reaches when the embed cache is in use (its own images move), and gc_finalize itself.  With the cache off
  the second is the only one, so both configurations run."""
  nd, original = replaying
  cached = request.node.callspec.params["replaying"] == "1"
  assert (nd.counter("embed_cache") > 0) == cached                            # the handle is in the configuration meant
  dims = SC.setup("T")[1]
  other = weights.random_params(dims, seed=4)
  nd.load_weights(other)
  nd.finalize()
  got = _run(nd, SIX_T)[0]
  np.testing.assert_array_equal(got, _fresh(params=other))
  assert _graphs(nd) == (1, 2) and np.abs(got - original).max() > 1e-3
  gr, _, _, _, _, _, _, _, _ = SC.setup("T")
  ref = SC.sample_oracle(SIX_T, net=SC.network(gr, dims, other))[0]
  assert _rel(got, ref) < SC.TOL
  np.testing.assert_array_equal(_run(nd, SIX_T)[0], got)                      # and is captured anew
  assert _graphs(nd) == (2, 3)


def test_churn_on_and_off_around_the_graph(replaying):
  nd, original = replaying
  case = SC.BY_ID["churn_alternate"]
  churned, calls, drawn = _run(nd, case)
  assert (calls, drawn) == (case.calls, case.draws) and _graphs(nd) == (1, 2)
  assert _rel(churned, SC.reference(case)[0]) < SC.TOL
  np.testing.assert_array_equal(_run(nd, SIX_T)[0], original)
  assert _graphs(nd) == (1, 3)


# ---- g. churn under the domain guard ------------------------------------------------------------------------------------

def test_the_guards_rerun_draws_the_same_fields_and_leaves_the_stream_where_one_sample_does():
  case = SC.BY_ID["churn_alternate"]
  k = case.draws
  big = helpers.tiny_setup(batch=2, seed=21)[3]
  big[:, :, 3] *= 2.0e5                                                        # one un-normalised channel, not a noisy slot
  nd = _make("T")
  try:
    fallbacks = nd.counter("range_fallbacks")
    out, calls, drawn = _run(nd, case, cond=big, stream=0)
    assert nd.counter("range_fallbacks") == fallbacks + 1
    assert calls == case.calls and drawn == k                                 # not 2 k: the re-run rewinds, then restores
    err = _rel(out, SC.sample_oracle(case, cond=big, stream0=0)[0])
    print(f"churn under the domain guard: re-run {err:.3g} of scale")
    assert np.isfinite(out).all() and err < SC.TOL
    nxt, calls, drawn = _run(nd, case, stream=None)                           # the stream goes on from k
    assert nd.counter("range_fallbacks") == fallbacks + 1
    assert calls == case.calls and drawn == k and nd.counter("noise_stream") == 2 * k
    err = _rel(nxt, SC.sample_oracle(case, stream0=k)[0])
    print(f"churn under the domain guard: next sample {err:.3g} of scale")
    assert err < SC.TOL
    assert _rel(nxt, SC.reference(case)[0]) > 1e-3                            # (streams 0..k-1 would be another sample)
  finally:
    nd.close()
