"""What the ctypes binding (`_lib.NativeDenoiser`) hands to the C library, pinned without a library or a device: every public
method runs on an object made with `object.__new__`, whose `_lib` records each C call instead of making it, and the log, what
the method returned (shapes and dtypes, never contents), the private state it set and every rejection that precedes a C call
(exception type and full text) are compared with tests/golden/binding_contract.json.

A record is `[name, arg...]`: None stays None, a Python scalar is its repr, a ctypes scalar passed by value is its type name
and value, a pointer, array or `byref` is its ctypes type name only (output buffers are `np.empty` and some inputs have no
elements, so nothing is read through a pointer; the GPU suite pins the values).

The file pins the BEHAVIOUR of the binding: a change that only moves code inside `_lib.py` leaves it untouched.  A change that
means to alter a call records it again with GENCAST_RECORD_BINDING_CONTRACT=1 (nothing in the suite sets it) and reviews the
diff of the JSON."""
import ctypes
import functools
import json
import os
import types

import numpy as np
import pytest

from gencast_flax_nnx_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "binding_contract.json")
G, MESH, B, C_IN, C = 312, 42, 2, 10, 6                     # the grid is 13 x 24, as in the other CPU tests
N_LAT, N_LON = 13, 24
DEL = object()                                              # a state override that removes the attribute

# the state of an object on which every set-up call has been made; a case overrides what it wants missing
READY = dict(_loss_groups=3, _ens_members=4, _spec_lmax=5, _event_thresholds=2, _fss_scales=3, _derive_c_src=7, _band_c_src=8,
             _feature_c_src=9, _feature_max=16, _feature_members=4, _order_quantiles=2, _energy_groups=2, _variogram_offsets=3,
             _tail_thresholds=2, _regions=3, _efi_plan=(2, 20), _map_plan=(3, 2, 2), _window_length=3, _n_forcing=2)
RETURNS = {"gc_last_error": b"the library's message", "gc_num_kernel_classes": 2, "gc_kernel_class_name": b"class"}


def _arg(a):
  if a is None:
    return None
  if isinstance(a, (bool, int, float, str, bytes)):
    return repr(a)
  if isinstance(a, np.generic):
    return f"{type(a).__name__}:{a.item()!r}"
  if isinstance(a, ctypes._SimpleCData):                   # pylint: disable=protected-access
    return f"{type(a).__name__}:{a.value!r}"
  if type(a).__name__ == "CArgObject":                     # ctypes.byref(x)
    return f"byref:{type(a._obj).__name__}"                # pylint: disable=protected-access
  assert isinstance(a, (ctypes._Pointer, ctypes.Array)), type(a)   # pylint: disable=protected-access
  return type(a).__name__


class Recorder:
  """Stands in for the loaded library: every attribute is a function that logs its arguments and returns a status."""

  def __init__(self, status):
    self.calls, self.status = [], status                   # status: one code, or {entry: code} (0 for the others)

  def __getattr__(self, name):
    def fn(*args):
      self.calls.append([name] + [_arg(a) for a in args])
      if name in RETURNS:
        return RETURNS[name]
      return self.status.get(name, 0) if isinstance(self.status, dict) else self.status
    return fn


def _bare(rec, **state):
  nd = object.__new__(_lib.NativeDenoiser)
  nd._lib, nd._h = rec, None
  nd.cfg = _lib.GcConfig(128, 128, 2, 256, 1, C_IN, C, B, 32, 32, 16.0)
  nd.num_grid_nodes, nd.num_mesh_nodes = G, MESH
  for k, v in {**READY, **state}.items():
    if v is not DEL:
      setattr(nd, k, v)
  return nd


def _ret(x):
  if x is None:
    return None
  if isinstance(x, np.ndarray):
    return [list(x.shape), str(x.dtype)]
  if isinstance(x, (tuple, list)):
    return [_ret(v) for v in x]
  if isinstance(x, dict):
    return {k: _ret(v) for k, v in sorted(x.items())}
  if isinstance(x, _lib.NativeDenoiser):
    return "NativeDenoiser"
  if isinstance(x, np.generic):
    return f"{type(x).__name__}:{x.item()!r}"
  assert isinstance(x, (bool, int, float, str, bytes)), type(x)
  return repr(x)


def _state(nd):
  return {k: repr(v) for k, v in vars(nd).items() if k not in ("_lib", "cfg")}


def _run(name):
  """-> {"c": the C calls, "r": what the method returned | "e": [exception type, text], "s": the attributes it set}."""
  fn, status, state = CASES[name]
  rec = Recorder(status)
  nd = _bare(rec, **state)
  other = _bare(Recorder(0), _ens_members=5)                # another handle, with a store of K = 5; a case may take its
  other._h = ctypes.c_void_p(2)                             # `_h` away: it is read for the C call only, after every check
  before, loader = _state(nd), _lib.load_library
  _lib.load_library = lambda path=None: rec                 # (only `NativeDenoiser(...)` itself asks for the library)
  got = {}
  try:
    got["r"] = _ret(fn(nd, other))
  except Exception as e:  # pylint: disable=broad-except
    got["e"] = [type(e).__name__, str(e)]
  finally:
    _lib.load_library = loader
  after = _state(nd)
  got["c"] = rec.calls
  got["s"] = {k: after.get(k) for k in sorted(set(before) | set(after)) if before.get(k) != after.get(k)}
  assert not other._lib.calls                               # pylint: disable=protected-access
  return json.loads(json.dumps({k: v for k, v in got.items() if v or k != "s"}))


# ---- arguments every accepted call starts from ------------------------------------------------------------------------------
def Z(*shape, dt=np.float32):
  return np.zeros(shape, dt)


def O(*shape, dt=np.float32):
  return np.ones(shape, dt)


X_IN, X_OUT, SIG = Z(G, B, C_IN), Z(G, B, C), O(B)
BAD_IN, BAD_OUT = Z(G, B, C_IN + 1), Z(G, B, C - 1)
WQ = O(G, dt=np.uint32)
THR = Z(2, G, B, C)
I6 = np.arange(C, dtype=np.int32)
F64 = np.float64


def _graph(**over):
  g = dict(num_grid_nodes=G, num_mesh_nodes=MESH, g2m_senders=Z(5, dt=np.int32), g2m_receivers=Z(5, dt=np.int32),
           m2g_senders=Z(6, dt=np.int32), m2g_receivers=Z(6, dt=np.int32), khop_rowptr=np.full(MESH + 1, 4, np.int32),
           khop_cols=Z(4, dt=np.int32), grid_struct=Z(G, 3), mesh_struct=Z(MESH, 3), g2m_edge_struct=Z(5, 4),
           m2g_edge_struct=Z(6, 4), mesh_xyz=Z(MESH, 3))
  g.update(over)
  return types.SimpleNamespace(**{k: v for k, v in g.items() if v is not DEL})


DERIVE = dict(c_src=7, op=[0, 1, 0, 1, 0, 0], src_a=I6, src_b=I6 + 1, affine=Z(C, 4, dt=F64), pool=0, n_lat=N_LAT, n_lon=N_LON)
POOLED = dict(pool=3, r_lat=1, r_lon=Z(N_LAT, dt=np.int32), row_weight=O(N_LAT, dt=F64))
EXPR = dict(scale=O(7, dt=F64), loc=Z(7, dt=F64))
TERMS = dict(op=[2, 3, 0, 1, 0, 0], term_start=[[0, 2, 2], [2, 3, 5]] + [[0, 0, 0]] * 4, term_coef=O(5, dt=F64),
             term_a=[0, 1, 2, 3, 4], term_b=[-1, 0, 1, 2, 3])
ROWS = dict(op=[4, 5, 0, 0, 0, 0], coslat=O(N_LAT, dt=F64), inv_rcos=O(N_LAT, dt=F64), inv_dphi=O(N_LAT, dt=F64), inv_2dlam=0.5,
            pole_row=Z(N_LAT, dt=np.int32))
BAND = dict(c_src=8, response=O(2, 5, dt=F64), complement=[0, 1], src_channel=I6, band=I6 % 2, legendre_synthesis=Z(5, N_LAT, 5),
            cos_s=Z(5, N_LON), sin_s=Z(5, N_LON))
FEATURE = dict(c_src=9, channel=I6, direction=O(C, dt=np.int32), use_threshold=Z(C, dt=np.int32), threshold=Z(C), n_lat=N_LAT,
               n_lon=N_LON, r_lat=Z(C, dt=np.int32), r_lon=Z(C, N_LAT, dt=np.int32), ring_lat=Z(C, dt=np.int32),
               ring_lon=Z(C, N_LAT, dt=np.int32), depth=Z(C, dt=F64), strike_lat=Z(C, dt=np.int32),
               strike_lon=Z(C, N_LAT, dt=np.int32))
PLAN = dict(kind=Z(C_IN, dt=np.int32), src=Z(C_IN, dt=np.int32), sidx=Z(C_IN, dt=np.int32), a=Z(C_IN), b=Z(C_IN), n_forcing=2)
FSS = dict(r_lat=Z(3, dt=np.int32), r_lon=Z(3, N_LAT, dt=np.int32), row_wq=O(N_LAT, dt=np.uint32))
ENERGY = dict(n_groups=2, group=[0, 0, 1, 1, -1, -1], scale=O(C, dt=F64))
VARIO = dict(n_lat=N_LAT, n_lon=N_LON, offsets=[[0, 1], [1, 0], [-1, 2]], p=1.0)
LOSSW = dict(node_weight=O(G), channel_weight=O(C), channel_group=Z(C, dt=np.int32), group_weight=O(3))
INIT = dict(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C_IN, c_out=C, batch=B)
NINE = _lib.GcConfig(128, 128, 2, 256, 1, C_IN, 9, B, 32, 32, 16.0)

CASES = {}


def case(name, fn, status=0, **state):
  assert name not in CASES, name
  CASES[name] = (fn, status, state)


def kw(method, base, **over):
  """A call of `method` with the keyword arguments `base`, some of them replaced."""
  return lambda nd, o: getattr(nd, method)(**{**base, **over})


# ---- construction, plumbing, set-up -------------------------------------------------------------------------------------------
case("init", lambda nd, o: _lib.NativeDenoiser(**INIT))
case("init/hidden_layers", lambda nd, o: _lib.NativeDenoiser(**INIT, hidden_layers=2, device_id=1))
case("init/hidden_layers refused", lambda nd, o: _lib.NativeDenoiser(**INIT, hidden_layers=2), status={"gc_set_option": 1})
for rc in (1, 5, 2):
  case(f"init/status {rc}", lambda nd, o: _lib.NativeDenoiser(**INIT), status={"gc_create": rc})
case("close/no handle", lambda nd, o: nd.close())
case("close", lambda nd, o: nd.close(), _h=ctypes.c_void_p(7))
case("closed", lambda nd, o: [nd.closed, o.closed])
case("set_option", lambda nd, o: nd.set_option("key", "value"))
case("set_graph", lambda nd, o: nd.set_graph(_graph()), num_grid_nodes=None, num_mesh_nodes=None)
case("set_graph/no mesh_xyz", lambda nd, o: nd.set_graph(_graph(mesh_xyz=DEL)))
case("set_graph/grid_struct", lambda nd, o: nd.set_graph(_graph(grid_struct=Z(G, 4))))
case("set_graph/mesh_struct", lambda nd, o: nd.set_graph(_graph(mesh_struct=Z(MESH + 1, 3))))
case("set_graph/g2m_edge_struct", lambda nd, o: nd.set_graph(_graph(g2m_edge_struct=Z(4, 4))))
case("set_graph/m2g_edge_struct", lambda nd, o: nd.set_graph(_graph(m2g_edge_struct=Z(6, 3))))
case("set_graph/g2m_receivers", lambda nd, o: nd.set_graph(_graph(g2m_receivers=Z(4, dt=np.int32))))
case("set_graph/m2g_receivers", lambda nd, o: nd.set_graph(_graph(m2g_receivers=Z(7, dt=np.int32))))
case("set_graph/rowptr shape", lambda nd, o: nd.set_graph(_graph(khop_rowptr=np.full(MESH, 4, np.int32))))
case("set_graph/rowptr end", lambda nd, o: nd.set_graph(_graph(khop_cols=Z(5, dt=np.int32))))
case("load_weights", lambda nd, o: nd.load_weights({"a": Z(2, 3), "b": Z(4, dt=F64)}))
case("load_weights/refused", lambda nd, o: nd.load_weights({"a": Z(2, 3), "b": Z(4)}), status=1)
case("missing_weights", lambda nd, o: nd.missing_weights())
case("finalize", lambda nd, o: nd.finalize())
case("set_noisy_slots", lambda nd, o: nd.set_noisy_slots(I6))
case("set_noisy_slots/shape", lambda nd, o: nd.set_noisy_slots(I6[:5]))

# ---- compute ------------------------------------------------------------------------------------------------------------------
case("denoise", lambda nd, o: nd.denoise(X_IN, SIG))
case("denoise/grid_feats", lambda nd, o: nd.denoise(BAD_IN, SIG))
case("denoise/sigma", lambda nd, o: nd.denoise(X_IN, O(B + 1)))
case("sample", lambda nd, o: nd.sample(X_IN, X_OUT, O(5)))
case("sample/keep dead call", lambda nd, o: nd.sample(X_IN, X_OUT, O(5), skip_dead_call=False))
case("sample/cond_feats", lambda nd, o: nd.sample(BAD_IN, X_OUT, O(5)))
case("sample/init_noise", lambda nd, o: nd.sample(X_IN, BAD_OUT, O(5)))
case("upload_cond", lambda nd, o: nd.upload_cond(X_IN))
case("upload_cond/shape", lambda nd, o: nd.upload_cond(BAD_IN))
case("upload_cond_dev", lambda nd, o: nd.upload_cond_dev(4096))
case("cond_device_ptr", lambda nd, o: nd.cond_device_ptr())
case("commit_cond", lambda nd, o: nd.commit_cond())
case("upload_noise", lambda nd, o: nd.upload_noise(X_OUT))
case("upload_noise/shape", lambda nd, o: nd.upload_noise(BAD_OUT))
case("sample_resident", lambda nd, o: nd.sample_resident(O(5)))
case("sample_resident/no stats", lambda nd, o: nd.sample_resident(O(5), skip_dead_call=False, want_stats=False))
case("download_sample", lambda nd, o: nd.download_sample())
case("stash_sample", lambda nd, o: nd.stash_sample())
case("download_stash", lambda nd, o: nd.download_stash())
case("rollout_plan", kw("rollout_plan", PLAN), _n_forcing=DEL)
for k in ("kind", "src", "sidx", "a", "b"):
  case(f"rollout_plan/{k}", kw("rollout_plan", PLAN, **{k: Z(C_IN + 1)}))
case("rollout_advance/none", lambda nd, o: nd.rollout_advance(None))
case("rollout_advance", lambda nd, o: nd.rollout_advance(Z(G, B, 2)))
case("rollout_advance/shape", lambda nd, o: nd.rollout_advance(Z(G, B, 3)))
case("rollout_advance/no plan", lambda nd, o: nd.rollout_advance(Z(G, B, 2)), _n_forcing=DEL)
case("download_cond", lambda nd, o: nd.download_cond())
case("sync", lambda nd, o: nd.sync())

# ---- measurement, noise, churn --------------------------------------------------------------------------------------------------
case("kernel_classes", lambda nd, o: nd.kernel_classes())
case("profile_enable", lambda nd, o: nd.profile_enable(1))
case("profile_set_stride", lambda nd, o: nd.profile_set_stride(2))
case("profile_read", lambda nd, o: nd.profile_read())
case("algorithmic_work", lambda nd, o: nd.algorithmic_work())
case("noise_set_tables", lambda nd, o: nd.noise_set_tables(N_LAT, N_LON, Z(4, N_LAT, 4), Z(N_LON, 4), Z(N_LON, 4)))
case("noise_set_tables/legendre", lambda nd, o: nd.noise_set_tables(N_LAT, N_LON, Z(4, N_LAT, 5), Z(N_LON, 4), Z(N_LON, 4)))
case("noise_set_tables/cos", lambda nd, o: nd.noise_set_tables(N_LAT, N_LON, Z(4, N_LAT, 4), Z(N_LON, 5), Z(N_LON, 4)))
case("noise_set_tables/sin", lambda nd, o: nd.noise_set_tables(N_LAT, N_LON, Z(4, N_LAT, 4), Z(N_LON, 4), Z(N_LON + 1, 4)))
case("noise_seed", lambda nd, o: nd.noise_seed(-1, 3))
case("noise_seed/default stream", lambda nd, o: nd.noise_seed(2 ** 64 + 5))
case("noise_draw", lambda nd, o: nd.noise_draw())
case("download_noise", lambda nd, o: nd.download_noise())
case("set_churn/none", lambda nd, o: nd.set_churn(None))
case("set_churn", lambda nd, o: nd.set_churn(Z(2, 3), 1.5))

# ---- denoising loss ---------------------------------------------------------------------------------------------------------------
case("loss_set_weights", kw("loss_set_weights", LOSSW), _loss_groups=0)
case("loss_set_weights/node_weight", kw("loss_set_weights", LOSSW, node_weight=O(G + 1)))
case("loss_set_weights/channel_weight", kw("loss_set_weights", LOSSW, channel_weight=O(C + 1)))
case("loss_set_weights/channel_group", kw("loss_set_weights", LOSSW, channel_group=Z(C - 1, dt=np.int32)))
case("loss_set_weights/group_weight", kw("loss_set_weights", LOSSW, group_weight=O(3, 1)))
case("upload_targets", lambda nd, o: nd.upload_targets(X_OUT))
case("upload_targets/shape", lambda nd, o: nd.upload_targets(BAD_OUT))
case("loss_resident", lambda nd, o: nd.loss_resident(O(4, B), draw_noise=True))
case("loss_resident/one evaluation", lambda nd, o: nd.loss_resident(O(B)))
case("loss_resident/sigmas", lambda nd, o: nd.loss_resident(O(4, B + 1)))
case("loss_resident/no evaluation", lambda nd, o: nd.loss_resident(O(0, B)))
case("loss_resident/no weights", lambda nd, o: nd.loss_resident(O(4, B)), _loss_groups=0)
case("loss_resident/everything wrong", lambda nd, o: nd.loss_resident(O(4, B + 1)), _loss_groups=0)
case("download_denoised", lambda nd, o: nd.download_denoised())
case("loss", lambda nd, o: nd.loss(X_IN, X_OUT, X_OUT, SIG))
case("loss/want_denoised", lambda nd, o: nd.loss(X_IN, X_OUT, X_OUT, SIG, want_denoised=True))
case("loss/cond_feats", lambda nd, o: nd.loss(BAD_IN, X_OUT, X_OUT, SIG))
case("loss/targets", lambda nd, o: nd.loss(X_IN, BAD_OUT, X_OUT, SIG))
case("loss/noise", lambda nd, o: nd.loss(X_IN, X_OUT, BAD_OUT, SIG))
case("loss/sigma", lambda nd, o: nd.loss(X_IN, X_OUT, X_OUT, O(B + 1)))
case("loss/no weights", lambda nd, o: nd.loss(X_IN, X_OUT, X_OUT, SIG), _loss_groups=0)
case("loss/everything wrong", lambda nd, o: nd.loss(X_IN, X_OUT, X_OUT, O(B + 1)), _loss_groups=0)

# ---- member store, marginal scores -------------------------------------------------------------------------------------------------
case("ens_reserve", lambda nd, o: nd.ens_reserve(8))
for rc in (1, 5, 4, 3):
  case(f"ens_reserve/status {rc}", lambda nd, o: nd.ens_reserve(8), status=rc)
case("ens_set_node_weight", lambda nd, o: nd.ens_set_node_weight(O(G)))
case("ens_set_node_weight/shape", lambda nd, o: nd.ens_set_node_weight(O(G, 1)))
case("ens_push", lambda nd, o: nd.ens_push(1))
case("ens_push/src", lambda nd, o: nd.ens_push(1, o))
case("ens_push_host", lambda nd, o: nd.ens_push_host(1, X_OUT))
case("ens_push_host/shape", lambda nd, o: nd.ens_push_host(1, BAD_OUT))
case("ens_score", lambda nd, o: nd.ens_score())
case("ens_score/truth, fields", lambda nd, o: nd.ens_score(X_OUT, want_fields=True))
case("ens_score/no store", lambda nd, o: nd.ens_score(), _ens_members=0)
case("ens_score/truth shape", lambda nd, o: nd.ens_score(BAD_OUT))
case("ens_score/everything wrong", lambda nd, o: nd.ens_score(BAD_OUT), _ens_members=0)
case("ens_download_fields", lambda nd, o: nd.ens_download_fields())
case("ens_push_state", lambda nd, o: nd.ens_push_state(1, I6))
case("ens_push_state/src", lambda nd, o: nd.ens_push_state(1, I6, o))
case("ens_push_state/shape", lambda nd, o: nd.ens_push_state(1, I6[:5]))
case("ens_download_member", lambda nd, o: nd.ens_download_member(1))

# ---- events, fractions ----------------------------------------------------------------------------------------------------------------
case("ens_event_set", lambda nd, o: nd.ens_event_set(THR, [1, -1], WQ), _event_thresholds=0)
case("ens_event_set/thresholds ndim", lambda nd, o: nd.ens_event_set(THR[0], [1, -1], WQ))
case("ens_event_set/thresholds shape", lambda nd, o: nd.ens_event_set(THR[:, :G - 1], [1, -1], WQ))
case("ens_event_set/directions", lambda nd, o: nd.ens_event_set(THR, [1], WQ))
case("ens_event_set/weights shape", lambda nd, o: nd.ens_event_set(THR, [1, -1], WQ[:G - 1]))
case("ens_event_set/weights kind", lambda nd, o: nd.ens_event_set(THR, [1, -1], O(G)))
case("ens_event_set/weights negative", lambda nd, o: nd.ens_event_set(THR, [1, -1], -O(G, dt=np.int64)))
case("ens_event_set/weights too large", lambda nd, o: nd.ens_event_set(THR, [1, -1], O(G, dt=np.int64) << 32))
case("ens_event_score", lambda nd, o: nd.ens_event_score())
case("ens_event_score/truth", lambda nd, o: nd.ens_event_score(X_OUT))
case("ens_event_score/no thresholds", lambda nd, o: nd.ens_event_score(), _event_thresholds=0)
case("ens_event_score/no store", lambda nd, o: nd.ens_event_score(), _ens_members=0)
case("ens_event_score/truth shape", lambda nd, o: nd.ens_event_score(BAD_OUT))
case("ens_event_score/everything wrong", lambda nd, o: nd.ens_event_score(BAD_OUT), _event_thresholds=0, _ens_members=0)
case("ens_event_codes", lambda nd, o: nd.ens_event_codes(1))
case("ens_event_codes/no thresholds", lambda nd, o: nd.ens_event_codes(1), _event_thresholds=0)
case("ens_fss_set", kw("ens_fss_set", FSS), _fss_scales=0)
case("ens_fss_set/n_lon", kw("ens_fss_set", FSS, n_lon=N_LON))
case("ens_fss_set/no scale", kw("ens_fss_set", FSS, r_lat=Z(0, dt=np.int32), r_lon=Z(0, N_LAT, dt=np.int32)))
case("ens_fss_set/nine scales", kw("ens_fss_set", FSS, r_lat=Z(9, dt=np.int32), r_lon=Z(9, N_LAT, dt=np.int32)))
case("ens_fss_set/r_lon scales", kw("ens_fss_set", FSS, r_lon=Z(2, N_LAT, dt=np.int32)))
case("ens_fss_set/r_lon ndim", kw("ens_fss_set", FSS, r_lon=Z(3, dt=np.int32)))
case("ens_fss_set/grid", kw("ens_fss_set", FSS, n_lon=N_LON + 1))
case("ens_fss_set/grid from rows", kw("ens_fss_set", FSS, r_lon=Z(3, 7, dt=np.int32), row_wq=O(7, dt=np.uint32)))
case("ens_fss_set/r_lat negative", kw("ens_fss_set", FSS, r_lat=np.array([0, -1, 0], np.int32)))
case("ens_fss_set/r_lon range", kw("ens_fss_set", FSS, r_lon=np.full((3, N_LAT), 12, np.int32)))
case("ens_fss_set/r_lon negative", kw("ens_fss_set", FSS, r_lon=np.full((3, N_LAT), -1, np.int32)))
case("ens_fss_set/row_wq shape", kw("ens_fss_set", FSS, row_wq=O(N_LAT + 1, dt=np.uint32)))
case("ens_fss_set/row_wq kind", kw("ens_fss_set", FSS, row_wq=O(N_LAT)))
case("ens_fss_set/row_wq zero", kw("ens_fss_set", FSS, row_wq=Z(N_LAT, dt=np.uint32)))
case("ens_fss_set/row_wq too large", kw("ens_fss_set", FSS, row_wq=np.full(N_LAT, 2 ** 24, np.uint32)))
case("ens_fss_score", lambda nd, o: nd.ens_fss_score())
case("ens_fss_score/no plan", lambda nd, o: nd.ens_fss_score(), _fss_scales=0)
case("ens_fss_score/no thresholds", lambda nd, o: nd.ens_fss_score(), _event_thresholds=0)
case("ens_fss_score/everything wrong", lambda nd, o: nd.ens_fss_score(), _fss_scales=0, _event_thresholds=0)
case("ens_fss_fields", lambda nd, o: nd.ens_fss_fields(1, 2))
case("ens_fss_fields/no plan", lambda nd, o: nd.ens_fss_fields(1, 2), _fss_scales=0)
case("ens_fss_fields/no thresholds", lambda nd, o: nd.ens_fss_fields(1, 2), _event_thresholds=0)
case("ens_fss_fields/t", lambda nd, o: nd.ens_fss_fields(2, 2))
case("ens_fss_fields/s", lambda nd, o: nd.ens_fss_fields(1, -1))
case("ens_fss_fields/everything wrong", lambda nd, o: nd.ens_fss_fields(2, 3), _fss_scales=0, _event_thresholds=0)

# ---- derived, band and feature views ----------------------------------------------------------------------------------------------------
D = functools.partial(kw, "ens_derive_set", DERIVE)
case("ens_derive_set", D(), _derive_c_src=0)
case("ens_derive_set/pooled", D(**POOLED))
case("ens_derive_set/expr", D(**EXPR), _derive_c_src=0)
case("ens_derive_set/expr, terms", D(**EXPR, **TERMS))
case("ens_derive_set/expr, rows", D(**EXPR, **ROWS))
case("ens_derive_set/expr, terms without term_b", D(**EXPR, **{**TERMS, "term_b": [0, 0, 1, 2, 3]}))
case("ens_derive_set/expr, everything", D(**{**EXPR, **TERMS, **ROWS, **POOLED, "op": [2, 3, 4, 5, 0, 1]}))
case("ens_derive_set/c_src", D(c_src=0))
for k in ("op", "src_a", "src_b"):
  case(f"ens_derive_set/{k} shape", D(**{k: I6[:5]}))
case("ens_derive_set/terms without scale", D(term_coef=O(5, dt=F64), pole_row=Z(N_LAT, dt=np.int32)))
case("ens_derive_set/plain op", D(op=[0, 2, 0, 0, 0, 0]))
case("ens_derive_set/expr op", D(**EXPR, op=[0, 6, 0, 0, 0, 0]))
case("ens_derive_set/expr op negative", D(**EXPR, op=[0, -1, 0, 0, 0, 0]))
case("ens_derive_set/src_a range", D(src_a=I6 + 2))
case("ens_derive_set/src_a negative", D(src_a=I6 - 1))
case("ens_derive_set/src_b range", D(src_b=I6 + 6))
case("ens_derive_set/src_b of a copy", D(op=[0] * C, src_b=I6 + 20), _derive_c_src=0)
case("ens_derive_set/affine", D(affine=Z(C, 3, dt=F64)))
case("ens_derive_set/pool", D(pool=4))
case("ens_derive_set/no n_lat", D(n_lat=None))
case("ens_derive_set/no n_lon", D(n_lon=None))
case("ens_derive_set/grid", D(n_lon=N_LON + 1))
case("ens_derive_set/r_lat", D(r_lat=-1))
case("ens_derive_set/pooled without r_lon", D(**{**POOLED, "r_lon": None}))
case("ens_derive_set/pooled without row_weight", D(**{**POOLED, "row_weight": None}))
case("ens_derive_set/r_lon shape", D(**{**POOLED, "r_lon": Z(N_LAT + 1, dt=np.int32)}))
case("ens_derive_set/row_weight shape", D(**{**POOLED, "row_weight": O(N_LAT - 1, dt=F64)}))
case("ens_derive_set/r_lon range", D(**{**POOLED, "r_lon": np.full(N_LAT, 12, np.int32)}))
case("ens_derive_set/row_weight zero", D(**{**POOLED, "row_weight": Z(N_LAT, dt=F64)}))
case("ens_derive_set/row_weight nan", D(**{**POOLED, "row_weight": np.full(N_LAT, np.nan)}))
case("ens_derive_set/scale alone", D(scale=O(7, dt=F64)))
case("ens_derive_set/loc alone", D(loc=O(7, dt=F64)))
case("ens_derive_set/scale shape", D(**{**EXPR, "scale": O(6, dt=F64)}))
case("ens_derive_set/loc nan", D(**{**EXPR, "loc": np.full(7, np.nan)}))
case("ens_derive_set/term lengths", D(**EXPR, **{**TERMS, "term_a": [0, 1, 2, 3]}))
case("ens_derive_set/term_coef nan", D(**EXPR, **{**TERMS, "term_coef": np.full(5, np.inf)}))
case("ens_derive_set/term_a range", D(**EXPR, **{**TERMS, "term_a": [0, 1, 2, 3, 7]}))
case("ens_derive_set/term_b range", D(**EXPR, **{**TERMS, "term_b": [-2, 0, 1, 2, 3]}))
case("ens_derive_set/no term_start", D(**EXPR, **{**TERMS, "term_start": None}))
case("ens_derive_set/term_start shape", D(**EXPR, **{**TERMS, "term_start": Z(C, 2, dt=np.int32)}))
case("ens_derive_set/term_start empty list", D(**EXPR, **{**TERMS, "term_start": [[0, 0, 0], [2, 3, 5]] + [[0, 0, 0]] * 4}))
case("ens_derive_set/term_start sum with two lists", D(**EXPR, **{**TERMS, "term_start": [[0, 1, 2], [2, 3, 5]] + [[0, 0, 0]] * 4}))
case("ens_derive_set/term_start past the table", D(**EXPR, **{**TERMS, "term_start": [[0, 2, 2], [2, 3, 6]] + [[0, 0, 0]] * 4}))
case("ens_derive_set/rows missing", D(**EXPR, **{**ROWS, "inv_2dlam": None}))
case("ens_derive_set/rows on two longitudes", D(**EXPR, **{**ROWS, "n_lat": 156, "n_lon": 2, "coslat": O(156, dt=F64)}))
case("ens_derive_set/rows shape", D(**EXPR, **{**ROWS, "pole_row": Z(N_LAT + 1, dt=np.int32)}))
OTHER, SELF = object(), object()
for method, c_src, attr in (("ens_derive", 7, "_derive_c_src"), ("ens_band", 8, "_band_c_src"), ("ens_feature", 9, "_feature_c_src")):
  view = lambda method, *a: (lambda nd, o: getattr(nd, method)(*(o if v is OTHER else nd if v is SELF else v for v in a)))
  case(method, view(method, OTHER), _feature_members=-1)
  case(f"{method}/truth", view(method, OTHER, Z(G, B, c_src)))
  case(f"{method}/no plan", view(method, OTHER), **{attr: 0})
  case(f"{method}/src no handle", view(method, "src"))
  case(f"{method}/src is self", view(method, SELF))
  case(f"{method}/truth shape", view(method, OTHER, X_OUT))
  case(f"{method}/everything wrong", view(method, SELF, X_OUT), **{attr: 0})
  case(f"{method}/refused", view(method, OTHER), status=4, _feature_members=-1)
  case(f"{method}/truth shape, src never created", lambda nd, o, method=method: (delattr(o, "_h"), getattr(nd, method)(o, X_OUT)))
Bd = functools.partial(kw, "ens_band_set", BAND)
case("ens_band_set", Bd(), _band_c_src=0)
case("ens_band_set/no tables", Bd(), _spec_lmax=0)
case("ens_band_set/everything wrong", Bd(c_src=0), _spec_lmax=0)
case("ens_band_set/c_src", Bd(c_src=0))
case("ens_band_set/response lmax", Bd(response=O(2, 4, dt=F64)))
case("ens_band_set/response nine bands", Bd(response=O(9, 5, dt=F64)))
case("ens_band_set/response nan", Bd(response=np.full((2, 5), np.nan)))
case("ens_band_set/complement", Bd(complement=[0, 1, 0]))
case("ens_band_set/complement of booleans", Bd(complement=[False, True]))
case("ens_band_set/src_channel shape", Bd(src_channel=I6[:5]))
case("ens_band_set/band shape", Bd(band=Z(C + 1, dt=np.int32)))
case("ens_band_set/src_channel range", Bd(src_channel=I6 + 3))
case("ens_band_set/band range", Bd(band=I6 % 3))
case("ens_band_set/legendre lmax", Bd(legendre_synthesis=Z(4, N_LAT, 5)))
case("ens_band_set/legendre grid", Bd(legendre_synthesis=Z(5, N_LAT + 1, 5)))
case("ens_band_set/cos_s", Bd(cos_s=Z(4, N_LON)))
case("ens_band_set/sin_s", Bd(sin_s=Z(5, N_LON + 1)))
Ft = functools.partial(kw, "ens_feature_set", FEATURE)
case("ens_feature_set", Ft(), _feature_c_src=0, _feature_max=0)
case("ens_feature_set/max_centres", Ft(max_centres=1024))
case("ens_feature_set/nine detectors", Ft(), cfg=NINE)
case("ens_feature_set/c_src", Ft(c_src=0))
case("ens_feature_set/no n_lat", Ft(n_lat=None))
case("ens_feature_set/grid", Ft(n_lon=N_LON - 1))
for k in ("channel", "direction", "use_threshold", "threshold", "r_lat", "ring_lat", "depth", "strike_lat"):
  case(f"ens_feature_set/{k} shape", Ft(**{k: FEATURE[k][:5]}))
case("ens_feature_set/channel range", Ft(channel=I6 + 4))
case("ens_feature_set/direction zero", Ft(direction=I6))
case("ens_feature_set/threshold nan", Ft(use_threshold=O(C, dt=np.int32), threshold=np.full(C, np.nan, np.float32)))
case("ens_feature_set/threshold nan, unused", Ft(threshold=np.full(C, np.nan, np.float32)))
for k in ("r_lat", "ring_lat", "strike_lat"):
  case(f"ens_feature_set/{k} negative", Ft(**{k: -O(C, dt=np.int32)}))
case("ens_feature_set/depth nan", Ft(ring_lat=O(C, dt=np.int32), depth=np.full(C, np.nan)))
for k in ("r_lon", "ring_lon", "strike_lon"):
  case(f"ens_feature_set/{k} shape", Ft(**{k: Z(C, N_LAT + 1, dt=np.int32)}))
  case(f"ens_feature_set/{k} range", Ft(**{k: np.full((C, N_LAT), 12, np.int32)}))
for v in (True, 0, 1025, 2.5):
  case(f"ens_feature_set/max_centres {v!r}", Ft(max_centres=v))
case("ens_feature_centres", lambda nd, o: nd.ens_feature_centres())
case("ens_feature_centres/no lists", lambda nd, o: nd.ens_feature_centres(), _feature_members=-1)

# ---- order statistics, climatology, EFI --------------------------------------------------------------------------------------------------
case("ens_order_set/none", lambda nd, o: nd.ens_order_set(None), _order_quantiles=None)
case("ens_order_set/empty", lambda nd, o: nd.ens_order_set([]))
case("ens_order_set", lambda nd, o: nd.ens_order_set([0.1, 0.5, 0.9]), _order_quantiles=None)
case("ens_order_set/nine", lambda nd, o: nd.ens_order_set(np.linspace(0, 1, 9)))
case("ens_order_set/ndim", lambda nd, o: nd.ens_order_set([[0.5]]))
case("ens_order_set/range", lambda nd, o: nd.ens_order_set([0.5, 1.5]))
case("ens_order_set/nan", lambda nd, o: nd.ens_order_set([np.nan]))
case("ens_order_score", lambda nd, o: nd.ens_order_score())
case("ens_order_score/truth", lambda nd, o: nd.ens_order_score(X_OUT))
case("ens_order_score/no quantiles", lambda nd, o: nd.ens_order_score(), _order_quantiles=0)
case("ens_order_score/not set", lambda nd, o: nd.ens_order_score(), _order_quantiles=None)
case("ens_order_score/no store", lambda nd, o: nd.ens_order_score(), _ens_members=0)
case("ens_order_score/truth shape", lambda nd, o: nd.ens_order_score(BAD_OUT))
case("ens_order_score/everything wrong", lambda nd, o: nd.ens_order_score(BAD_OUT), _order_quantiles=None, _ens_members=0)
case("ens_order_fields", lambda nd, o: nd.ens_order_fields())
case("ens_order_fields/not set", lambda nd, o: nd.ens_order_fields(), _order_quantiles=None)
case("ens_order_fields/no store", lambda nd, o: nd.ens_order_fields(), _ens_members=0)
case("ens_order_quantile", lambda nd, o: nd.ens_order_quantile(1))
case("ens_order_quantile/not set", lambda nd, o: nd.ens_order_quantile(1), _order_quantiles=None)
case("ens_order_quantile/without a store", lambda nd, o: nd.ens_order_quantile(1), _ens_members=0)
case("ens_clim_score", lambda nd, o: nd.ens_clim_score(o))
case("ens_clim_score/truth", lambda nd, o: nd.ens_clim_score(o, X_OUT))
case("ens_clim_score/clim no handle", lambda nd, o: nd.ens_clim_score("clim"))
case("ens_clim_score/clim is self", lambda nd, o: nd.ens_clim_score(nd))
case("ens_clim_score/no store", lambda nd, o: nd.ens_clim_score(o), _ens_members=0)
case("ens_clim_score/truth shape", lambda nd, o: nd.ens_clim_score(o, BAD_OUT))
case("ens_clim_score/everything wrong", lambda nd, o: nd.ens_clim_score("clim", BAD_OUT), _ens_members=0)
case("ens_clim_score/no store, clim never created", lambda nd, o: (delattr(o, "_h"), nd.ens_clim_score(o)), _ens_members=0)
case("ens_clim_score/self, no store", lambda nd, o: nd.ens_clim_score(nd, BAD_OUT), _ens_members=0)
case("ens_efi_set", lambda nd, o: nd.ens_efi_set(), _efi_plan=None)
case("ens_efi_set/events", lambda nd, o: nd.ens_efi_set([1, 3], [1, -1], 10, WQ), _efi_plan=None)
case("ens_efi_set/directions", lambda nd, o: nd.ens_efi_set([1, 3], [1], 10, WQ))
case("ens_efi_set/n_bins True", lambda nd, o: nd.ens_efi_set(n_bins=True))
case("ens_efi_set/n_bins 2.5", lambda nd, o: nd.ens_efi_set(n_bins=2.5))
case("ens_efi_set/no weights", lambda nd, o: nd.ens_efi_set([1, 3], [1, -1]))
case("ens_efi_set/weights kind", lambda nd, o: nd.ens_efi_set([1, 3], [1, -1], 10, O(G)))
case("ens_efi_set/weights negative", lambda nd, o: nd.ens_efi_set([1, 3], [1, -1], 10, -O(G, dt=np.int64)))
case("ens_efi_set/weights unchecked without events", lambda nd, o: nd.ens_efi_set(node_weight_q=O(3)))
TABLE = np.linspace(0.0, 1.0, 6)
case("ens_efi_score", lambda nd, o: nd.ens_efi_score(o, TABLE))
case("ens_efi_score/truth", lambda nd, o: nd.ens_efi_score(o, TABLE, X_OUT))
case("ens_efi_score/no events", lambda nd, o: nd.ens_efi_score(o, TABLE), _efi_plan=(0, 16))
case("ens_efi_score/clim no handle", lambda nd, o: nd.ens_efi_score(None, TABLE))
case("ens_efi_score/clim is self", lambda nd, o: nd.ens_efi_score(nd, TABLE))
case("ens_efi_score/no store", lambda nd, o: nd.ens_efi_score(o, TABLE), _ens_members=0)
case("ens_efi_score/clim no store", lambda nd, o: (setattr(o, "_ens_members", 0), nd.ens_efi_score(o, TABLE)))
case("ens_efi_score/table", lambda nd, o: nd.ens_efi_score(o, TABLE[:5]))
case("ens_efi_score/not set", lambda nd, o: nd.ens_efi_score(o, TABLE), _efi_plan=None)
case("ens_efi_score/truth shape", lambda nd, o: nd.ens_efi_score(o, TABLE, BAD_OUT))
case("ens_efi_score/everything wrong", lambda nd, o: nd.ens_efi_score("clim", TABLE[:5], BAD_OUT), _efi_plan=None, _ens_members=0)
case("ens_efi_score/stores, table, plan", lambda nd, o: (setattr(o, "_ens_members", 0), nd.ens_efi_score(o, TABLE[:5], BAD_OUT)),
     _efi_plan=None, _ens_members=0)
case("ens_efi_score/clim store, table, plan", lambda nd, o: (setattr(o, "_ens_members", 0), nd.ens_efi_score(o, TABLE[:5], BAD_OUT)),
     _efi_plan=None)
case("ens_efi_score/table, plan", lambda nd, o: nd.ens_efi_score(o, TABLE[:5], BAD_OUT), _efi_plan=None)
case("ens_efi_fields", lambda nd, o: nd.ens_efi_fields(o, TABLE), _efi_plan=None)
case("ens_efi_fields/clim is self", lambda nd, o: nd.ens_efi_fields(nd, TABLE))
case("ens_efi_fields/table, clim never created", lambda nd, o: (delattr(o, "_h"), nd.ens_efi_fields(o, [TABLE])))
case("ens_efi_score/truth shape, clim never created", lambda nd, o: (delattr(o, "_h"), nd.ens_efi_score(o, TABLE, BAD_OUT)))
case("ens_efi_fields/table", lambda nd, o: nd.ens_efi_fields(o, [TABLE]))
case("ens_efi_field", lambda nd, o: nd.ens_efi_field())
case("ens_efi_field/observed", lambda nd, o: nd.ens_efi_field(1), _efi_plan=None)

# ---- multivariate scores, score maps, tails, regions ------------------------------------------------------------------------------------
En = functools.partial(kw, "ens_energy_set", ENERGY)
case("ens_energy_set", En(), _energy_groups=None)
case("ens_energy_set/group shape", En(group=[0, 1]))
case("ens_energy_set/scale shape", En(scale=O(C + 1, dt=F64)))
case("ens_energy_set/n_groups 0", En(n_groups=0))
case("ens_energy_set/n_groups 33", En(n_groups=33))
case("ens_energy_set/group below", En(group=[0, 0, 1, 1, -2, -1]))
case("ens_energy_set/group above", En(group=[0, 0, 1, 2, -1, -1]))
case("ens_energy_set/group empty", En(n_groups=3))
case("ens_energy_set/scale zero", En(scale=Z(C, dt=F64)))
case("ens_energy_set/scale nan, ungrouped", En(scale=np.array([1, 1, 1, 1, np.nan, 0.0])))
Va = functools.partial(kw, "ens_variogram_set", VARIO)
case("ens_variogram_set", Va(), _variogram_offsets=None)
case("ens_variogram_set/offsets shape", Va(offsets=[[0, 1, 2]]))
case("ens_variogram_set/no offsets", Va(offsets=Z(0, 2, dt=np.int32)))
case("ens_variogram_set/seventeen offsets", Va(offsets=O(17, 2, dt=np.int32)))
case("ens_variogram_set/p", Va(p=1.5))
case("ens_variogram_set/grid", Va(n_lat=N_LAT + 1))
case("ens_variogram_set/offset zero", Va(offsets=[[0, 1], [0, 0]]))
case("ens_variogram_set/offset rows", Va(offsets=[[N_LAT, 0]]))
case("ens_variogram_set/offset columns", Va(offsets=[[0, -N_LON]]))
for method, attr, unset in (("ens_energy_score", "_energy_groups", None), ("ens_variogram_score", "_variogram_offsets", None),
                            ("ens_tail_score", "_tail_thresholds", 0), ("ens_region_score", "_regions", 0)):
  score = lambda method, *a: (lambda nd, o: getattr(nd, method)(*a))
  case(method, score(method))
  case(f"{method}/truth", score(method, X_OUT))
  case(f"{method}/no plan", score(method), **{attr: unset})
  case(f"{method}/no store", score(method), _ens_members=0)
  case(f"{method}/truth shape", score(method, BAD_OUT))
  case(f"{method}/everything wrong", score(method, BAD_OUT), _ens_members=0, **{attr: unset})
case("ens_map_set", lambda nd, o: nd.ens_map_set(), _map_plan=None)
case("ens_map_set/channels", lambda nd, o: nd.ens_map_set([0, 2, 5], n_slots=4, n_event_thresholds=2), _map_plan=None)
case("ens_map_set/channels empty", lambda nd, o: nd.ens_map_set([]))
case("ens_map_set/channels ndim", lambda nd, o: nd.ens_map_set([[0, 1]]))
case("ens_map_accumulate", lambda nd, o: nd.ens_map_accumulate(1))
case("ens_map_accumulate/truth", lambda nd, o: nd.ens_map_accumulate(1, X_OUT))
case("ens_map_accumulate/truth shape", lambda nd, o: nd.ens_map_accumulate(1, BAD_OUT))
case("ens_map_accumulate/no store, no plan", lambda nd, o: nd.ens_map_accumulate(1), _ens_members=0, _map_plan=None)
case("ens_map_accumulate_events", lambda nd, o: nd.ens_map_accumulate_events(1), _map_plan=None)
case("ens_map_download", lambda nd, o: nd.ens_map_download(1))
case("ens_map_download/events", lambda nd, o: nd.ens_map_download(1, events=True))
case("ens_map_download/no events", lambda nd, o: nd.ens_map_download(1, events=False))
case("ens_map_download/plan without events", lambda nd, o: nd.ens_map_download(1), _map_plan=(6, 2, 0))
case("ens_map_download/events of a plan without", lambda nd, o: nd.ens_map_download(1, events=True), _map_plan=(6, 2, 0))
case("ens_map_download/no plan", lambda nd, o: nd.ens_map_download(1), _map_plan=None)
case("ens_map_download/no plan, refused", lambda nd, o: nd.ens_map_download(1), status=4, _map_plan=None)
case("ens_map_reset", lambda nd, o: nd.ens_map_reset())
case("ens_map_reset/slot", lambda nd, o: nd.ens_map_reset(1))
case("ens_tail_set", lambda nd, o: nd.ens_tail_set(THR, [1, -1]), _tail_thresholds=0)
case("ens_tail_set/thresholds ndim", lambda nd, o: nd.ens_tail_set(THR[0], [1]))
case("ens_tail_set/thresholds shape", lambda nd, o: nd.ens_tail_set(THR[:, :, :1], [1, -1]))
case("ens_tail_set/no thresholds", lambda nd, o: nd.ens_tail_set(THR[:0], []))
case("ens_tail_set/nine thresholds", lambda nd, o: nd.ens_tail_set(Z(9, G, B, C), [1] * 9))
case("ens_tail_set/directions shape", lambda nd, o: nd.ens_tail_set(THR, [1, -1, 1]))
case("ens_tail_set/directions zero", lambda nd, o: nd.ens_tail_set(THR, [1, 0]))
case("ens_region_set", lambda nd, o: nd.ens_region_set(WQ, 4), _regions=0)
case("ens_region_set/n_regions 0", lambda nd, o: nd.ens_region_set(WQ, 0))
case("ens_region_set/n_regions 33", lambda nd, o: nd.ens_region_set(WQ, 33))
case("ens_region_set/shape", lambda nd, o: nd.ens_region_set(WQ[:5], 4))
case("ens_region_set/kind", lambda nd, o: nd.ens_region_set(O(G), 4))
case("ens_region_set/negative", lambda nd, o: nd.ens_region_set(-O(G, dt=np.int32), 4))
case("ens_region_set/bits", lambda nd, o: nd.ens_region_set(WQ * 16, 4))

# ---- time windows, context store, spectra ------------------------------------------------------------------------------------------------
case("ens_window_set/linear", lambda nd, o: nd.ens_window_set(0, 4, [1.0, 1.0, 1.0, 1.0]), _window_length=0)
case("ens_window_set/max", lambda nd, o: nd.ens_window_set(1, 64), _window_length=0)
case("ens_window_set/kind", lambda nd, o: nd.ens_window_set(3, 2))
case("ens_window_set/length 0", lambda nd, o: nd.ens_window_set(0, 0, [1.0]))
case("ens_window_set/length 65", lambda nd, o: nd.ens_window_set(2, 65))
case("ens_window_set/linear without coef", lambda nd, o: nd.ens_window_set(0, 2))
case("ens_window_set/coef shape", lambda nd, o: nd.ens_window_set(0, 2, [1.0]))
case("ens_window_set/coef nan", lambda nd, o: nd.ens_window_set(0, 2, [1.0, np.nan]))
case("ens_window_set/min with coef", lambda nd, o: nd.ens_window_set(2, 2, [1.0, 1.0]))
case("ens_window_push", lambda nd, o: nd.ens_window_push(o))
case("ens_window_push/truth", lambda nd, o: nd.ens_window_push(o, X_OUT))
case("ens_window_push/no plan", lambda nd, o: nd.ens_window_push(o), _window_length=0)
case("ens_window_push/src no handle", lambda nd, o: nd.ens_window_push(None))
case("ens_window_push/src is self", lambda nd, o: nd.ens_window_push(nd))
case("ens_window_push/truth shape", lambda nd, o: nd.ens_window_push(o, BAD_OUT))
case("ens_window_push/truth shape, src never created", lambda nd, o: (delattr(o, "_h"), nd.ens_window_push(o, BAD_OUT)))
case("ens_window_push/everything wrong", lambda nd, o: nd.ens_window_push(nd, BAD_OUT), _window_length=0)
case("ens_window_emit", lambda nd, o: nd.ens_window_emit())
case("ens_window_emit/no plan", lambda nd, o: nd.ens_window_emit(), _window_length=0)
case("ens_window_reset", lambda nd, o: nd.ens_window_reset(), _window_length=0)
case("ctx_reserve", lambda nd, o: nd.ctx_reserve(4))
case("ctx_save", lambda nd, o: nd.ctx_save(1))
case("ctx_save/src", lambda nd, o: nd.ctx_save(1, o))
case("ctx_load", lambda nd, o: nd.ctx_load(1))
case("ctx_load/dst", lambda nd, o: nd.ctx_load(1, o))
case("ctx_download", lambda nd, o: nd.ctx_download(1))
case("spec_set_tables", lambda nd, o: nd.spec_set_tables(Z(7, 7, N_LAT), Z(7, N_LON), Z(7, N_LON)))
case("spec_set_tables/first", lambda nd, o: nd.spec_set_tables(Z(7, 7, N_LAT), Z(7, N_LON), Z(7, N_LON)), _spec_lmax=0, _band_c_src=0)
case("spec_set_tables/legendre ndim", lambda nd, o: nd.spec_set_tables(Z(7, 7), Z(7, N_LON), Z(7, N_LON)))
case("spec_set_tables/legendre square", lambda nd, o: nd.spec_set_tables(Z(7, 6, N_LAT), Z(7, N_LON), Z(7, N_LON)))
case("spec_set_tables/cos ndim", lambda nd, o: nd.spec_set_tables(Z(7, 7, N_LAT), Z(7), Z(7)))
case("spec_set_tables/sin", lambda nd, o: nd.spec_set_tables(Z(7, 7, N_LAT), Z(7, N_LON), Z(7, N_LON + 1)))
case("spec_set_tables/cos lmax", lambda nd, o: nd.spec_set_tables(Z(7, 7, N_LAT), Z(6, N_LON), Z(6, N_LON)))
case("spec_field", lambda nd, o: nd.spec_field())
case("spec_field/field", lambda nd, o: nd.spec_field(X_OUT))
case("spec_field/no tables", lambda nd, o: nd.spec_field(), _spec_lmax=0)
case("spec_field/field shape", lambda nd, o: nd.spec_field(BAD_OUT))
case("spec_field/everything wrong", lambda nd, o: nd.spec_field(BAD_OUT), _spec_lmax=0)
case("ens_spectrum", lambda nd, o: nd.ens_spectrum())
case("ens_spectrum/truth, member power", lambda nd, o: nd.ens_spectrum(X_OUT, want_member_power=True))
case("ens_spectrum/no tables", lambda nd, o: nd.ens_spectrum(), _spec_lmax=0)
case("ens_spectrum/no store", lambda nd, o: nd.ens_spectrum(), _ens_members=0)
case("ens_spectrum/truth shape", lambda nd, o: nd.ens_spectrum(BAD_OUT))
case("ens_spectrum/everything wrong", lambda nd, o: nd.ens_spectrum(BAD_OUT), _spec_lmax=0, _ens_members=0)

# ---- exchange, counters, debug ------------------------------------------------------------------------------------------------------------
case("comm_init", lambda nd, o: nd.comm_init(bytes(128), 1, 2))
case("comm_init/id length", lambda nd, o: nd.comm_init(bytes(127), 1, 2))
case("comm_info", lambda nd, o: nd.comm_info())
case("comm_broadcast_cond", lambda nd, o: nd.comm_broadcast_cond())
case("comm_broadcast_cond/root", lambda nd, o: nd.comm_broadcast_cond(1))
case("comm_allreduce_max", lambda nd, o: nd.comm_allreduce_max(1.5))
case("comm_destroy", lambda nd, o: nd.comm_destroy())
case("counter", lambda nd, o: nd.counter("launches_per_call"))
case("debug_fetch", lambda nd, o: nd.debug_fetch("name"))
case("debug_set_layer_limit", lambda nd, o: nd.debug_set_layer_limit(2))
case("debug_set_stop", lambda nd, o: nd.debug_set_stop(1))
case("debug_set_stop/phase", lambda nd, o: nd.debug_set_stop(-1, 2))
case("debug_mesh_permutation", lambda nd, o: nd.debug_mesh_permutation())
case("debug_attention_stats", lambda nd, o: nd.debug_attention_stats())


@functools.lru_cache(maxsize=None)
def _golden():
  with open(GOLDEN) as f:
    return json.load(f)


def test_every_public_method_has_a_case():
  methods = {n for n, v in vars(_lib.NativeDenoiser).items() if not n.startswith("_") and (callable(v) or isinstance(v, property))}
  assert methods == {name.split("/")[0] for name in CASES} - {"init"}


def test_the_golden_file_holds_exactly_the_cases():
  if os.environ.get("GENCAST_RECORD_BINDING_CONTRACT") == "1":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    with open(GOLDEN, "w") as f:
      f.write("{\n" + ",\n".join(json.dumps(name) + ": " + json.dumps(_run(name), separators=(",", ":"), sort_keys=True)
                                 for name in sorted(CASES)) + "\n}\n")
    pytest.skip("recorded")                                # never reached in the suite: a recording is not a pass
  assert sorted(_golden()) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_binding_makes_the_recorded_calls(name):
  got, want = _run(name), _golden()[name]
  assert got.get("e") == want.get("e")                     # first the rejection and the order, for a readable failure
  assert [c[0] for c in got["c"]] == [c[0] for c in want["c"]]
  assert got == want
