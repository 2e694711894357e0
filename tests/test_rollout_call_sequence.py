"""The order and the arguments of every device call of an ensemble rollout and of the single-step ensemble methods, and what
they return, against a recorded log (tests/golden/rollout_call_sequence.json): the handles are `helpers.RecordingHandle`, the
inputs small integers with power-of-two statistics, so every value handed to a handle is exact in float32.

The fixture is a record of what the code did when it was written down, not a definition: a change that is MEANT to alter the
calls records it again with GENCAST_RECORD_CALL_SEQUENCE=1 (nothing in the suite sets it) and reviews the diff of the JSON."""
import json
import os
import types

import numpy as np
import pytest

from gencast_flax_nnx_amd import config as cfg
from gencast_flax_nnx_amd import datasets, rollout, verification
from gencast_flax_nnx_amd.datasets import Dataset, Variable
from gencast_flax_nnx_amd.denoiser import Denoiser
from gencast_flax_nnx_amd.ensemble import EnsembleSampler
from gencast_flax_nnx_amd.verification import DerivedSpec, EventSpec, WindowSpec
from tests.helpers import RecordingHandle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rollout_call_sequence.json")
LAT, LON = np.array([-45.0, 45.0]), np.array([0.0, 120.0, 240.0])
G, B, M, HORIZON = 6, 1, 2, 3
TASK = cfg.TaskConfig(input_variables=("u", "v", "z", "f", "s"), target_variables=("u", "v", "z"), forcing_variables=("f",),
                      pressure_levels=(500, 850), input_duration="24h")


# ---- small exact inputs ---------------------------------------------------------------------------------------------------
def _ints(seed, shape, lo=-4, hi=5):
  return np.random.RandomState(seed).randint(lo, hi, shape).astype(np.float32)   # (the legacy stream: frozen for good)


def _fields(seed, n_time, names=("u", "v", "z")):
  dv = {}
  for i, name in enumerate(names):
    if name == "z":
      dv[name] = Variable(("batch", "time", "level", "lat", "lon"), _ints(seed + i, (B, n_time, 2, 2, 3)))
    else:
      dv[name] = Variable(("batch", "time", "lat", "lon"), _ints(seed + i, (B, n_time, 2, 3)))
  return Dataset(dv, {"lat": LAT, "lon": LON, "level": np.array([500, 850])})


def _example():
  inputs = _fields(10, 2, ("u", "v", "z", "f"))
  inputs = inputs.assign(Dataset({"s": Variable(("lat", "lon"), _ints(19, (2, 3)))}))
  return inputs, _fields(20, HORIZON), _fields(30, HORIZON, ("f",))


def _stats():
  """Scales, locations and residual scales: powers of two and small integers, so (x - l) / s is exact."""
  lev = lambda a: Variable(("level",), np.array(a, np.float32))
  one = lambda a: Variable((), np.float32(a))
  scales = Dataset({"u": one(2.0), "v": one(0.5), "z": lev([4.0, 1.0]), "f": one(2.0), "s": one(1.0)})
  locs = Dataset({"u": one(1.0), "v": one(-1.0), "z": lev([2.0, 0.0]), "f": one(0.0), "s": one(1.0)})
  resid = Dataset({"u": one(0.5), "v": one(0.25), "z": lev([1.0, 0.5])})
  return scales, locs, resid


# ---- a model on handles that record -----------------------------------------------------------------------------------------
class _HostOnlyDenoiser(Denoiser):
  """A `Denoiser` without a device: `init_for` packs as ever, every handle it hands out is a `RecordingHandle`, cached as
  the real one caches (a view per width, a climatology handle per (width, view), a window handle per (width, key))."""

  def __init__(self, log, c_out):  # pylint: disable=super-init-not-called
    self._log, self._c_out, self._handles = log, c_out, {}
    self.native = self.dims = None

  def _handle(self, name, c):
    if name not in self._handles:
      self._handles[name] = RecordingHandle(name, self._log, M=M, B=B, C=c, G=G, full=True)
    return self._handles[name]

  def _maybe_init(self, grid_feats_shape, lat, lon):
    self.dims = types.SimpleNamespace(c_in=grid_feats_shape[2], c_out=self._c_out)
    self.native = self._handle("lane0", self._c_out)

  def member_lanes(self, count):
    return [self._handle(f"lane{i + 1}", self._c_out) for i in range(count)]

  def view_handle(self, c_d):
    return self._handle(f"view{c_d}", c_d)

  def climatology_handle(self, c_d, *, view=False):
    return self._handle(f"clim{'view' if view else ''}{c_d}", c_d)

  def window_handle(self, c_d, key):
    return self._handle(f"window{c_d}:{key}", c_d)


class _Sampler:
  """What `EnsembleRollout` and `EnsembleSampler` read of a `Sampler`; the noise is a fixed field, no generator is used."""
  noise_levels = np.array([4.0, 1.0, 0.0])

  def __init__(self, denoiser):
    self._denoiser = denoiser

  def draw_noise(self, gen, shape, template):
    del gen, template
    return _ints(7, shape)


def _model(log):
  den = _HostOnlyDenoiser(log, c_out=4)
  return types.SimpleNamespace(_sampler=_Sampler(den), denoiser=den)


# ---- what goes into the fixture ---------------------------------------------------------------------------------------------
def _plain(x):
  """JSON for one logged value: scalars as they are, arrays as shape + dtype + values, a handle as its name."""
  if isinstance(x, RecordingHandle):
    return {"handle": x.name}
  if isinstance(x, np.ndarray):
    return {"shape": list(x.shape), "dtype": str(x.dtype), "values": x.reshape(-1).tolist()}
  if isinstance(x, np.generic):
    return x.item()
  if isinstance(x, (list, tuple)):
    return [_plain(v) for v in x]
  if isinstance(x, dict):
    return {str(k): _plain(v) for k, v in sorted(x.items())}
  if x is None or isinstance(x, (bool, int, float, str)):
    return x
  raise TypeError(f"a logged value of type {type(x)}")


def _returned(x):
  """JSON for a returned value: None stays None, a score object becomes its arrays, a Dataset its variables."""
  if isinstance(x, Dataset):
    return {k: _plain(np.asarray(v.data)) for k, v in sorted(x.items())}
  if isinstance(x, dict):
    return {k: _returned(v) for k, v in sorted(x.items())}
  if isinstance(x, (list, tuple)):
    return [_returned(v) for v in x]
  if hasattr(x, "__dict__") and not isinstance(x, np.ndarray):
    return {"type": type(x).__name__,
            **{k: _returned(v) for k, v in sorted(vars(x).items()) if not k.startswith("_")}}
  return _plain(x)


def _check(case, got):
  got = json.loads(json.dumps(got))                        # (tuples become lists, as in the file)
  if os.environ.get("GENCAST_RECORD_CALL_SEQUENCE") == "1":
    known = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    known[case] = got
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
      f.write("{\n" + ",\n".join(
          json.dumps(name) + ": {\n" + ",\n".join(
              json.dumps(part) + ": " + (json.dumps(value, separators=(",", ":")) if part != "calls" else
                                         "[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in value) + "\n]")
              for part, value in sorted(known[name].items())) + "\n}" for name in sorted(known)) + "\n}\n")
    pytest.skip("recorded")                                # never reached in the suite: a recording is not a pass
  want = json.load(open(GOLDEN))[case]
  assert sorted(got) == sorted(want)
  assert [c[:2] for c in got["calls"]] == [c[:2] for c in want["calls"]]      # first the order, for a readable failure
  for i, (a, b) in enumerate(zip(got["calls"], want["calls"])):
    assert a == b, f"call {i}: {a[:2]}"
  for part in want:
    assert got[part] == want[part], part


# ---- the rollout ------------------------------------------------------------------------------------------------------------
def _rollout(log, **kw):
  inputs, targets, forcings = _example()
  model = _model(log)
  norm = rollout.InputsAndResiduals(None, *_stats())
  er = rollout.EnsembleRollout(model, norm, TASK, base_seed=3, concurrent_members=2)
  init_noise = [[_ints(100 + 10 * m + k, (G, B, 4)) for k in range(HORIZON)] for m in range(M)]
  return er.run(inputs, targets, forcings, HORIZON, M, init_noise=init_noise, **kw)


def test_a_rollout_with_everything_on_makes_the_recorded_calls():
  log = []
  thr = lambda k: EventSpec({"u": np.array([1.0 + k, -1.0]), "z": np.array([[2.0, 0.0], [1.0, -2.0]]).reshape(2, 2, 1, 1)}, [1, -1])
  speed = DerivedSpec([("norm2", "speed", "u", "v")])
  smooth = DerivedSpec([("copy", "u")], pool="mean", r_lat=1, r_lon=[1, 1])
  climatology = lambda k: [_fields(40 + 10 * k + j, 1) for j in range(2)]
  res = _rollout(log, fields=True, keep_members=True, events=[thr(k) for k in range(HORIZON)], order=[0.1, 0.5],
                 keep_quantiles=True, climatology=climatology,
                 derived={"speed": (speed, EventSpec({"speed": np.array([2.0])}, [1])), "smooth": smooth},
                 windows={"acc": (WindowSpec("sum", 2), EventSpec({"v": np.array([0.5])}, [-1])),
                          "gust": WindowSpec("max", 2, stride=1, source="speed")})
  # the two derived entries share a view handle (and the climatology view that goes with it)
  assert {c[0] for c in log} == {"lane0", "lane1", "view1", "clim4", "climview1", "window4:acc", "window1:gust"}
  _check("rollout_everything", {"calls": _plain(log), "result": _returned(res)})


def test_a_rollout_with_nothing_optional_makes_the_recorded_calls():
  log = []
  res = _rollout(log)
  assert {c[0] for c in log} == {"lane0", "lane1"}
  _check("rollout_plain", {"calls": _plain(log), "result": _returned(res)})


# ---- the single-step methods ------------------------------------------------------------------------------------------------
def test_the_single_step_methods_make_the_recorded_calls():
  inputs, targets, forcings = _example()
  targets, forcings = rollout.isel_time(targets, slice(0, 1)), rollout.isel_time(forcings, slice(0, 1))
  log, out = [], {}
  runner = EnsembleSampler(_model(log)._sampler, base_seed=3, concurrent_members=2)
  marks = {}
  for name, call in (
      ("scores", lambda: runner.scores(inputs, targets, forcings, M, fields=True)),
      ("events", lambda: runner.events(inputs, targets, forcings, M, EventSpec({"u": np.array([1.0])}, [1]))),
      ("order", lambda: runner.order(inputs, targets, forcings, M, (0.1, 0.5), quantile_fields=True)),
      ("climatology", lambda: runner.climatology(inputs, targets, forcings, M, [_fields(40 + j, 1) for j in range(3)])),
      ("derived", lambda: runner.derived(inputs, targets, forcings, M, DerivedSpec([("norm2", "speed", "u", "v")]),
                                         EventSpec({"speed": np.array([2.0])}, [1])))):
    out[name] = _returned(call())
    marks[name] = len(log)                                 # where the method's calls end in the one log
  _check("single_step", {"calls": _plain(log), "ends": marks, "result": out})
