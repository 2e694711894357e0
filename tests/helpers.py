"""Shared builders for the parity tests (tiny and nano configurations)."""
import dataclasses

import numpy as np

from gencast_flax_nnx_amd import geometry, weights


def graph_dict(gr):
  return dataclasses.asdict(gr)


def tiny_setup(batch=2, seed=0, mesh_size=2, k_hop=2, latent=128, heads=2, ffw=256, layers=2,
               c_in=20, c_out=6, n_lat=13, n_lon=24, hidden_layers=1):
  lat = np.linspace(-90, 90, n_lat)
  lon = np.arange(n_lon) * (360.0 / n_lon)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh_size,
                                     attention_k_hop=k_hop)
  dims = weights.ModelDims(c_in=c_in, c_out=c_out, latent=latent, d_model=latent, num_heads=heads,
                           ffw_hidden=ffw, num_layers=layers, hidden_layers=hidden_layers)
  params = weights.random_params(dims, seed=3)
  rng = np.random.default_rng(seed)
  x = rng.standard_normal((gr.num_grid_nodes, batch, c_in)).astype(np.float32)
  sigma = np.exp(rng.uniform(np.log(0.03), np.log(80.0), size=batch)).astype(np.float32)
  return gr, dims, params, x, sigma


def make_native(gr, dims, params, batch, device_id=0, precision=None):
  from gencast_flax_nnx_amd import _lib
  nd = _lib.NativeDenoiser(latent_size=dims.latent, d_model=dims.d_model, num_heads=dims.num_heads,
                           ffw_hidden=dims.ffw_hidden, num_layers=dims.num_layers, c_in=dims.c_in,
                           c_out=dims.c_out, batch=batch, device_id=device_id, hidden_layers=dims.hidden_layers)
  if precision:
    nd.set_option("precision", precision)
  nd.set_graph(gr)
  nd.load_weights(params)
  assert nd.missing_weights() == 0
  nd.finalize()
  return nd


def nano_setup(batch=1):
  """BASELINE.json configs[1]: nano model on the 2.5 deg grid."""
  return tiny_setup(batch=batch, mesh_size=4, k_hop=8, latent=256, heads=4, ffw=2048, layers=16, c_in=262,
                    c_out=82, n_lat=73, n_lon=144)


def one_degree_setup(layers=16, k_hop=8):
  """BASELINE.json configs[3]: 1 deg grid, mesh 5, full GenCast widths (latent 512, 4 heads of 128)."""
  lat = np.arange(-90.0, 90.0 + 1e-9, 1.0)
  lon = np.arange(0.0, 360.0, 1.0)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=5, attention_k_hop=k_hop)
  dims = weights.ModelDims(c_in=262, c_out=82, latent=512, d_model=512, num_heads=4, ffw_hidden=2048,
                           num_layers=layers)
  params = weights.random_params(dims, seed=3)
  x = np.random.default_rng(0).standard_normal((gr.num_grid_nodes, 1, 262)).astype(np.float32)
  return gr, dims, params, x, np.array([3.0], np.float32)


def khop16_setup():
  """SURVEY.md 8d stress case: mesh 5 with k_hop = 16 (up to 799 keys per query), heads of 128."""
  return tiny_setup(batch=1, seed=5, mesh_size=5, k_hop=16, latent=256, heads=2, ffw=256, layers=2, c_in=20,
                    c_out=6, n_lat=73, n_lon=144)


def small_graph(n_lat=13, n_lon=24, mesh_size=2, k_hop=2):
  """The graph of a small equiangular grid, poles included (G = n_lat * n_lon)."""
  lat = np.linspace(-90, 90, n_lat)
  lon = np.arange(n_lon) * (360.0 / n_lon)
  return geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=mesh_size, attention_k_hop=k_hop)


class RecordingHandle:
  """A stand-in for `_lib.NativeDenoiser` that needs no device: every call appends `(name, call, *details)` to the shared
  list `log` and returns arrays of the shapes the library returns -- `G` nodes, batch `B`, `C` channels, `M` members --
  filled with the number of times that call has been made on this handle (1.0 the first time), so two results that were
  appended in another order are not equal.  `details` is what the host-side tests assert on: the scalars, `truth is None`,
  the name of another handle.  With `full=True` the remaining arguments follow them, so that the log pins every value
  handed to the device, and a method the class does not define is logged by its name and arguments (without `full` it is an
  AttributeError: a binding call the test did not expect)."""

  def __init__(self, name, log, M=4, B=2, C=3, G=4, Q=0, full=False):
    self.name, self.calls, self.M, self.B, self.C, self.G, self.full = name, log, M, B, C, G, full
    self.Q, self.T = Q, 0                                   # quantile probabilities (until `ens_order_set`) / events set
    self._made = {}

  def _log(self, call, *details, full=()):
    self.calls.append((self.name, call) + details + (tuple(full) if self.full else ()))
    self._made[call] = self._made.get(call, 0) + 1

  def _filled(self, call, shape, dtype=np.float64):
    return np.full(shape, self._made[call], dtype)

  def __getattr__(self, call):
    if call.startswith("_") or not self.full:               # (without `full`, a call no test expects is an error)
      raise AttributeError(call)
    return lambda *args, **kwargs: self._log(call, full=args + tuple(sorted(kwargs.items())))

  def cond_device_ptr(self):
    self._log("cond_device_ptr")
    return self.name + ".cond", 0

  def ens_reserve(self, n):
    self._log("reserve", n)

  def ens_set_node_weight(self, w):
    self._log("weight", full=(w,))

  def ens_push(self, slot, src=None):
    self._log("push", slot, getattr(src, "name", None))

  def ens_push_host(self, slot, field):
    self._log("push_host", slot, float(np.asarray(field).ravel()[0]), full=(field,))

  def ens_event_set(self, thr, directions, wq):
    self.T = len(directions)
    self._log("event_set", np.asarray(thr).copy(), full=(directions, wq))

  def ens_order_set(self, probs):
    self.Q = len(probs)
    self._log("order_set", tuple(probs))

  def ens_derive_set(self, **plan):
    self._log("derive_set", full=sorted(plan.items()))

  def ens_derive(self, src, truth):
    self._log("derive", getattr(src, "name", None), truth)

  def ens_score(self, truth, want_fields=False):
    self._log("score", truth is None, full=(truth, want_fields))
    return self._filled("score", (self.B, self.C, 6)), self._filled("score", (self.B, self.C, self.M + 1), np.uint64)

  def ens_download_fields(self):
    self._log("download_fields")
    return (self._filled("download_fields", (self.G, self.B, self.C), np.float32),
            2 * self._filled("download_fields", (self.G, self.B, self.C), np.float32))

  def ens_event_score(self, truth):
    self._log("event_score", truth is None, full=(truth,))
    table = self._filled("event_score", (self.T, self.B, self.C, 2, self.M + 1), np.uint64)
    return table, table.copy(), np.zeros(self.T, np.uint64)

  def ens_order_score(self, truth):
    self._log("order_score", truth is None, full=(truth,))
    return (self._filled("order_score", (self.B, self.C, self.M + 1, 2)), self._filled("order_score", (self.B, self.C, 3)),
            self._filled("order_score", (self.B, self.C, self.Q)),
            self._filled("order_score", (self.B, self.C, self.Q + 1), np.uint64), 0)

  def ens_order_quantile(self, q):
    self._log("quantile", q)
    return np.full((self.G, self.B, self.C), float(q), np.float32)

  def ens_clim_score(self, clim, truth):
    self._log("clim_score", clim.name, truth is None, full=(truth,))
    return self._filled("clim_score", (self.B, self.C, 12)), np.full((self.B, self.C), 5, np.uint64), 7

  def ens_download_member(self, m):
    self._log("download", m)
    return np.full((self.G, self.B, self.C), float(m), np.float32)

  def ens_window_set(self, kind, length, coef):
    self._log("window_set", kind, length, None if coef is None else tuple(coef))

  def ens_window_push(self, src, truth):
    self._log("window_push", src.name, truth is None, full=(truth,))

  def ens_window_emit(self):
    self._log("window_emit")

  def ens_window_reset(self):
    self._log("window_reset")


def graph_handle(gr, batch, c_out, latent=128, heads=2, ffw=256):
  """A handle that knows its graph and nothing else: no weights, no gc_finalize."""
  from gencast_flax_nnx_amd import _lib
  nd = _lib.NativeDenoiser(latent_size=latent, d_model=latent, num_heads=heads, ffw_hidden=ffw, num_layers=1,
                           c_in=c_out + 4, c_out=c_out, batch=batch)
  nd.set_graph(gr)
  return nd
