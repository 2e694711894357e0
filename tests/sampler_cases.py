"""Every branch of the fused sampler loop: the case table shared by tests/test_sampler_cases.py (CPU: the table itself,
with the oracle alone) and tests/test_gpu_sampler_cases.py (the loop of csrc/gc_sampler.hip).

`run_sampler` / `sampler_body` are a hand-written state machine around every forward of a sample.  A row is one sample
that sends the loop through branches no other sampler test reaches; `BRANCHES` names them, `trace` derives from a row's
schedule alone which ones it takes (a restatement of the loop's control flow, no arithmetic), and the CPU test holds the
row's own `reaches` against that.

Setups (both `helpers.tiny_setup`, dense attention in the oracle):
  T  the default tiny setup: 13 x 24 grid, mesh 2, 2 layers, batch 2
  S  the smallest graph the library accepts, for the long schedules: 7 x 12 grid (G = 84), mesh 1 (42 nodes), 1-hop,
     1 layer, batch 1 -- a 97-call float64 oracle sample takes under a second

What a row expects besides the float64 result: the denoiser calls, the noise fields drawn inside the loop (what the
`noise_stream` counter advances by), `multi` (calls <= 96: one `gc_cond_multi` launch for the sample; above, one `gc_cond`
launch per call) and `graph_eligible` (`multi` and no churn rate > 0: the sample is captured and replayed).
"""
import dataclasses
import functools

import numpy as np

from oracle import gencast_oracle as O
from oracle import noise_oracle as NO
from tests import helpers

TOL = 1e-4                   # the project's bound (tests/test_gpu_parity.py): max |out - ref| < TOL * max(1, max |ref|)
MAX_SIGMA_LIST = 96          # gc::kMaxSigmaList
CLAMP = 1e-6                 # the level below which a call's noise level is clamped (dpm_solver_plus_plus_2s.py:84-85)
SEED = 11                    # the Philox key of every churn row
RATE, INFLATION = 0.3, 1.05

SETUPS = {
    "T": dict(batch=2),
    "S": dict(batch=1, n_lat=7, n_lon=12, mesh_size=1, k_hop=1, layers=1),
}

# what the loop can do, by the `if` that decides it (csrc/gc_sampler.hip, sampler_body)
BRANCHES = {
    "init_fused": "the initial gc_scale also writes c_in x for call 0",
    "init_plain": "churn at step 0: the initial gc_scale carries no fused write, call 0 writes its own input",
    "first_fused": "dpm_first writes the mid-point state for the call that follows",
    "first_plain": "sigma_next == 0 and the dead call is skipped: dpm_first writes nothing fused",
    "dead_call": "sigma_next == 0 with skip_dead off: the mid-point call runs at the clamped level and is discarded",
    "second_fused": "dpm_second writes c_in x for the next step's first call",
    "second_plain_end": "the last step has sigma_next > 0: dpm_second has no next call to write for (i + 1 == n)",
    "second_plain_churn": "the next step churns: dpm_second writes nothing fused",
    "churn_consecutive": "two churned steps in a row",
    "churn_last": "churn at the step whose sigma_next == 0",
    "churn_dead": "a churned step followed by the dead call",
    "one_step": "n == 1",
    "clamp_live": "a live call whose level lies below the clamp",
    "multi_full": "96 calls: still one conditioning launch, SigmaList full",
    "per_call": "more than 96 calls: one conditioning launch per call, never captured",
    "churn_per_call": "churn on the per-call path",
    "zero_rates": "a churn schedule of all-zero rates: the same as off",
}


@dataclasses.dataclass(frozen=True)
class Case:
  id: str
  setup: str               # key of SETUPS
  sigmas: tuple            # n + 1 noise levels
  skip_dead: bool
  rates: tuple             # per-step churn rates, or None
  reaches: tuple           # the keys of BRANCHES this row is there for
  calls: int               # expected denoiser calls
  draws: int               # expected noise fields drawn inside the loop
  multi: bool
  graph_eligible: bool
  inflation: float = INFLATION

  @property
  def n(self):
    return len(self.sigmas) - 1


def karras(n):
  """`n` descending levels from 80 to 0.03 and a trailing zero, as every sampler test of the suite uses them."""
  return tuple(float(s) for s in O.noise_schedule(80.0, 0.03, n, 7.0))


def _rates(n, steps):
  return tuple(RATE if i in steps else 0.0 for i in range(n))


def _c(id, setup, sigmas, skip_dead, rates, reaches, calls, draws, multi=True, graph_eligible=True):
  return Case(id, setup, tuple(sigmas), skip_dead, rates, tuple(reaches), calls, draws, multi, graph_eligible)


SIX = karras(6)
CASES = [
    _c("one_step_skip", "T", (3.0, 0.0), True, None, ["one_step", "init_fused", "first_plain"], 1, 0),
    _c("one_step_dead", "T", (3.0, 0.0), False, None, ["one_step", "dead_call", "first_fused"], 2, 0),
    _c("one_step_live", "T", (3.0, 0.5), True, None, ["one_step", "second_plain_end"], 2, 0),
    _c("no_trailing_zero", "T", SIX[:-1], True, None, ["second_plain_end", "second_fused"], 10, 0),
    _c("below_clamp", "T", (0.5, 1e-7, 0.0), True, None, ["clamp_live"], 3, 0),
    _c("calls_96", "S", karras(48), False, None, ["multi_full", "dead_call"], 96, 0),
    _c("calls_97", "S", karras(49), True, None, ["per_call"], 97, 0, multi=False, graph_eligible=False),
    _c("churn_first", "T", SIX, True, _rates(6, {0}), ["init_plain", "second_fused"], 11, 1, graph_eligible=False),
    _c("churn_last", "T", SIX, True, _rates(6, {5}), ["churn_last", "second_plain_churn", "init_fused"], 11, 1,
       graph_eligible=False),
    _c("churn_all", "T", SIX, True, _rates(6, set(range(6))), ["churn_consecutive", "init_plain", "churn_last"], 11, 6,
       graph_eligible=False),
    _c("churn_alternate", "T", SIX, True, _rates(6, {0, 2, 4}), ["second_plain_churn", "second_fused", "init_plain"],
       11, 3, graph_eligible=False),
    _c("churn_dead", "T", SIX, False, _rates(6, set(range(6))), ["churn_dead", "dead_call"], 12, 6, graph_eligible=False),
    _c("churn_zero_rates", "T", SIX, True, _rates(6, set()), ["zero_rates"], 11, 0),
    _c("churn_97", "S", karras(49), True, _rates(49, {3, 4, 48}), ["churn_per_call", "per_call", "churn_consecutive"],
       97, 3, multi=False, graph_eligible=False),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def trace(case):
  """(calls, draws, branches taken) of a row, from its schedule alone: the control flow of sampler_body."""
  sig, n = case.sigmas, case.n
  rate = lambda i: case.rates[i] if case.rates is not None and i < n else 0.0
  taken, calls, draws = set(), 0, 0
  if n == 1:
    taken.add("one_step")
  if case.rates is not None and not any(r > 0 for r in case.rates):
    taken.add("zero_rates")
  taken.add("init_plain" if rate(0) > 0 else "init_fused")
  for i in range(n):
    sg, sn = sig[i], sig[i + 1]
    if rate(i) > 0:
      draws += 1
      sg = sg * (1.0 + rate(i))
      if rate(i + 1) > 0:
        taken.add("churn_consecutive")
      if sn == 0:
        taken.add("churn_last")
        if not case.skip_dead:
          taken.add("churn_dead")
    if sg < CLAMP:
      taken.add("clamp_live")
    calls += 1
    if sn == 0 and case.skip_dead:
      taken.add("first_plain")
      continue
    taken.add("first_fused")
    calls += 1
    if sn == 0:
      taken.add("dead_call")
      continue
    if np.sqrt(sg * sn) < CLAMP:
      taken.add("clamp_live")
    if i + 1 == n:
      taken.add("second_plain_end")
    elif rate(i + 1) > 0:
      taken.add("second_plain_churn")
    else:
      taken.add("second_fused")
  if calls == MAX_SIGMA_LIST:
    taken.add("multi_full")
  if calls > MAX_SIGMA_LIST:
    taken.add("per_call")
    if draws:
      taken.add("churn_per_call")
  return calls, draws, taken


def plain(setup, sigmas, skip_dead=True):
  """A sample without churn that is NOT a row of the table (the tests use such samples next to the rows: a six-step
  sample before and after a long one, the nine schedules of the LRU test).  It claims to reach nothing, and its counts
  are what `trace` gives for the schedule."""
  case = Case(f"plain_{len(sigmas) - 1}", setup, tuple(sigmas), skip_dead, None, (), 0, 0, True, True)
  calls = trace(case)[0]
  fits = calls <= MAX_SIGMA_LIST
  return dataclasses.replace(case, calls=calls, multi=fits, graph_eligible=fits)


@functools.lru_cache(maxsize=None)
def setup(name):
  """(graph, dims, params, cond, lat, lon, noisy slots, initial noise, network function) of a setup; shared, never
  modified."""
  cfg = dict(SETUPS[name])
  gr, dims, params, x, _ = helpers.tiny_setup(**cfg)
  lat = np.linspace(-90, 90, cfg.get("n_lat", 13))
  n_lon = cfg.get("n_lon", 24)
  lon = np.arange(n_lon) * (360.0 / n_lon)
  slots = np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32)
  noise = np.random.default_rng(5).standard_normal((gr.num_grid_nodes, cfg["batch"], dims.c_out)).astype(np.float32)
  for a in (x, slots, noise):
    a.setflags(write=False)
  return gr, dims, params, x, lat, lon, slots, noise, network(gr, dims, params)


def network(gr, dims, params):
  g = helpers.graph_dict(gr)
  attn = O.make_attention_fn(g, "dense")
  return lambda f, s: O.denoiser_forward(params, g, f, s, num_layers=dims.num_layers, num_heads=dims.num_heads,
                                         attention=attn)


@functools.lru_cache(maxsize=None)
def field(setup_name, stream):
  """The unit-variance field the device draws for (SEED, stream): [G, B, c_out], float64."""
  gr, dims, _, x, lat, lon, _, _, _ = setup(setup_name)
  B = x.shape[1]
  f = NO.device_field(SEED, stream, lat, lon, B * dims.c_out).reshape(gr.num_grid_nodes, B, dims.c_out)
  f.setflags(write=False)
  return f


def sample_oracle(case, cond=None, stream0=0, net=None):
  """(float64 sample, calls, draws) of a row; `cond` replaces the setup's conditioning, `stream0` is the Philox stream
  of the first field drawn, `net` replaces the setup's network function (other weights)."""
  _, _, _, x, _, _, slots, noise, net0 = setup(case.setup)
  cond = (x if cond is None else cond).astype(np.float64)
  net = net or net0
  sig = np.asarray(case.sigmas, np.float64)
  if case.rates is None:
    out, calls = O.dpm_solver_2s_sample(net, cond, slots, noise.astype(np.float64), sig, skip_dead_call=case.skip_dead)
    return out, calls, 0
  return NO.dpm_solver_2s_sample_churn(net, cond, slots, noise.astype(np.float64), sig, case.rates, case.inflation,
                                       lambda k: field(case.setup, stream0 + k), skip_dead_call=case.skip_dead)


@functools.lru_cache(maxsize=None)
def _reference(case_id):
  out, calls, draws = sample_oracle(BY_ID[case_id])
  out.setflags(write=False)
  return out, calls, draws


def reference(case):
  """The float64 result of a row, its denoiser calls and the fields it drew; computed once, shared, never modified."""
  return _reference(case.id)
