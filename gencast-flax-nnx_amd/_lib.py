"""ctypes binding of libgencast_hip.so (include/gencast_hip.h).

There is no CPU fallback: if the shared library is missing this module raises at
import of the native symbols, and without a HIP device `gc_create` fails.
"""
from __future__ import annotations

import ctypes
import os
import sys
from typing import Dict, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgencast_hip.so")

GC_OK = 0
GC_ERR_INVALID_ARGUMENT = 1
GC_ERR_NO_DEVICE = 2
GC_ERR_HIP = 3
GC_ERR_STATE = 4
GC_ERR_UNSUPPORTED = 5
GC_ERR_INTERNAL = 6
GC_ERR_COMM = 7
COMM_ID_BYTES = 128


class GcConfig(ctypes.Structure):
  _fields_ = [
      ("latent_size", ctypes.c_int32), ("d_model", ctypes.c_int32), ("num_heads", ctypes.c_int32),
      ("ffw_hidden", ctypes.c_int32), ("num_layers", ctypes.c_int32), ("c_in", ctypes.c_int32),
      ("c_out", ctypes.c_int32), ("batch", ctypes.c_int32),
      ("noise_num_frequencies", ctypes.c_int32), ("noise_hidden", ctypes.c_int32),
      ("noise_base_period", ctypes.c_float)]


class GcSampleStats(ctypes.Structure):
  _fields_ = [("denoiser_calls", ctypes.c_int32), ("device_ms", ctypes.c_float)]


class GencastHipError(RuntimeError):
  """A HIP / state failure inside the native library."""


_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
_f64p = ctypes.POINTER(ctypes.c_double)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_hp = ctypes.c_void_p
_hpp = ctypes.POINTER(_hp)

# name -> (restype, argtypes); every symbol include/gencast_hip.h (+ _debug.h) declares.
SIGNATURES = {
    "gc_abi_version": (ctypes.c_int, []),
    "gc_build_info": (ctypes.c_char_p, []),
    "gc_device_count": (ctypes.c_int, []),
    "gc_device_pci_bus_id": (ctypes.c_int, [ctypes.c_int32, ctypes.c_char_p, ctypes.c_int64]),
    "gc_last_error": (ctypes.c_char_p, [_hp]),
    "gc_create": (ctypes.c_int, [ctypes.POINTER(GcConfig), ctypes.c_int, _hpp]),
    "gc_destroy": (None, [_hp]),
    "gc_set_option": (ctypes.c_int, [_hp, ctypes.c_char_p, ctypes.c_char_p]),
    "gc_set_graph": (ctypes.c_int, [_hp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i32p, _i32p, ctypes.c_int32, _i32p,
                                    _i32p, _i32p, _i32p, _f32p, _f32p, _f32p, _f32p, _f32p]),
    "gc_load_weight": (ctypes.c_int, [_hp, ctypes.c_char_p, _f32p, _i64p, ctypes.c_int32]),
    "gc_missing_weights": (ctypes.c_int, [_hp, _i32p]),
    "gc_finalize": (ctypes.c_int, [_hp]),
    "gc_denoise": (ctypes.c_int, [_hp, _f32p, _f32p, _f32p]),
    "gc_set_noisy_slots": (ctypes.c_int, [_hp, _i32p]),
    "gc_sample": (ctypes.c_int, [_hp, _f32p, _f32p, _f32p, ctypes.c_int32, ctypes.c_int32, _f32p, ctypes.POINTER(GcSampleStats)]),
    "gc_upload_cond": (ctypes.c_int, [_hp, _f32p]),
    "gc_upload_cond_dev": (ctypes.c_int, [_hp, ctypes.c_void_p]),
    "gc_upload_noise": (ctypes.c_int, [_hp, _f32p]),
    "gc_sample_resident": (ctypes.c_int, [_hp, _f32p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(GcSampleStats)]),
    "gc_download_sample": (ctypes.c_int, [_hp, _f32p]),
    "gc_stash_sample": (ctypes.c_int, [_hp]),
    "gc_download_stash": (ctypes.c_int, [_hp, _f32p]),
    "gc_rollout_plan": (ctypes.c_int, [_hp, _i32p, _i32p, _i32p, _f32p, _f32p, ctypes.c_int32]),
    "gc_rollout_advance": (ctypes.c_int, [_hp, _f32p]),
    "gc_download_cond": (ctypes.c_int, [_hp, _f32p]),
    "gc_sync": (ctypes.c_int, [_hp]),
    "gc_cond_device_ptr": (ctypes.c_int, [_hp, _hpp, _i64p]),
    "gc_commit_cond": (ctypes.c_int, [_hp]),
    "gc_num_kernel_classes": (ctypes.c_int, []),
    "gc_kernel_class_name": (ctypes.c_char_p, [ctypes.c_int]),
    "gc_profile_enable": (ctypes.c_int, [_hp, ctypes.c_int]),
    "gc_profile_set_stride": (ctypes.c_int, [_hp, ctypes.c_int]),
    "gc_profile_read": (ctypes.c_int, [_hp, _i32p, _f32p]),
    "gc_algorithmic_work": (ctypes.c_int, [_hp, _f64p, _f64p]),
    "gc_get_counter": (ctypes.c_int, [_hp, ctypes.c_char_p, _i64p]),
    "gc_noise_set_tables": (ctypes.c_int, [_hp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _f32p, _f32p, _f32p]),
    "gc_noise_seed": (ctypes.c_int, [_hp, ctypes.c_uint64, ctypes.c_uint64]),
    "gc_noise_draw": (ctypes.c_int, [_hp]),
    "gc_download_noise": (ctypes.c_int, [_hp, _f32p]),
    "gc_set_churn": (ctypes.c_int, [_hp, _f32p, ctypes.c_int32, ctypes.c_float]),
    "gc_loss_set_weights": (ctypes.c_int, [_hp, _f32p, _f32p, _i32p, ctypes.c_int32, _f32p]),
    "gc_upload_targets": (ctypes.c_int, [_hp, _f32p]),
    "gc_loss_resident": (ctypes.c_int, [_hp, _f32p, ctypes.c_int32, ctypes.c_int32, _f32p, _f32p]),
    "gc_download_denoised": (ctypes.c_int, [_hp, _f32p]),
    "gc_loss": (ctypes.c_int, [_hp, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p]),
    "gc_ens_reserve": (ctypes.c_int, [_hp, ctypes.c_int32]),
    "gc_ens_set_node_weight": (ctypes.c_int, [_hp, _f32p]),
    "gc_ens_push": (ctypes.c_int, [_hp, ctypes.c_int32, _hp]),
    "gc_ens_push_host": (ctypes.c_int, [_hp, ctypes.c_int32, _f32p]),
    "gc_ens_score": (ctypes.c_int, [_hp, _f32p, ctypes.c_int32, _f64p, _u64p]),
    "gc_ens_download_fields": (ctypes.c_int, [_hp, _f32p, _f32p]),
    "gc_ctx_reserve": (ctypes.c_int, [_hp, ctypes.c_int32]),
    "gc_ctx_save": (ctypes.c_int, [_hp, ctypes.c_int32, _hp]),
    "gc_ctx_load": (ctypes.c_int, [_hp, ctypes.c_int32, _hp]),
    "gc_ctx_download": (ctypes.c_int, [_hp, ctypes.c_int32, _f32p]),
    "gc_ens_push_state": (ctypes.c_int, [_hp, ctypes.c_int32, _hp, _i32p]),
    "gc_ens_download_member": (ctypes.c_int, [_hp, ctypes.c_int32, _f32p]),
    "gc_spec_set_tables": (ctypes.c_int, [_hp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _f32p, _f32p, _f32p]),
    "gc_spec_field": (ctypes.c_int, [_hp, _f32p, _f64p]),
    "gc_ens_spectrum": (ctypes.c_int, [_hp, _f32p, _f64p, _f64p]),
    "gc_ens_event_set": (ctypes.c_int, [_hp, ctypes.c_int32, _f32p, _i32p, _u32p]),
    "gc_ens_event_score": (ctypes.c_int, [_hp, _f32p, _u64p, _u64p, _u64p]),
    "gc_ens_event_download": (ctypes.c_int, [_hp, ctypes.c_int32, _u8p]),
    "gc_ens_fss_set": (ctypes.c_int, [_hp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i32p, _i32p, _u32p]),
    "gc_ens_fss_score": (ctypes.c_int, [_hp, _f64p]),
    "gc_ens_fss_fields": (ctypes.c_int, [_hp, ctypes.c_int32, ctypes.c_int32, _f32p, _f32p]),
    "gc_ens_derive_set": (ctypes.c_int, [_hp, ctypes.c_int32, _i32p, _i32p, _i32p, _f64p, ctypes.c_int32, ctypes.c_int32,
                                         ctypes.c_int32, ctypes.c_int32, _i32p, _f64p]),
    "gc_ens_derive_set_expr": (ctypes.c_int, [_hp, ctypes.c_int32, _i32p, _i32p, _i32p, _f64p, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_int32, ctypes.c_int32, _i32p, _f64p, _f64p, _f64p, _i32p, ctypes.c_int32,
                                              _f64p, _i32p, _i32p, _f64p, _f64p, _f64p, ctypes.c_double, _i32p]),
    "gc_ens_derive": (ctypes.c_int, [_hp, _hp, _f32p]),
    "gc_ens_band_set": (ctypes.c_int, [_hp, ctypes.c_int32, ctypes.c_int32, _f64p, _i32p, _i32p, _i32p, _f32p, _f32p, _f32p]),
    "gc_ens_band": (ctypes.c_int, [_hp, _hp, _f32p]),
    "gc_ens_order_set": (ctypes.c_int, [_hp, ctypes.c_int32, _f64p]),
    "gc_ens_order_score": (ctypes.c_int, [_hp, _f32p, _f64p, _f64p, _f64p, _u64p, _u64p]),
    "gc_ens_order_fields": (ctypes.c_int, [_hp]),
    "gc_ens_order_download": (ctypes.c_int, [_hp, ctypes.c_int32, _f32p]),
    "gc_ens_clim_score": (ctypes.c_int, [_hp, _hp, _f32p, _f64p, _u64p, _u64p]),
    "gc_ens_efi_set": (ctypes.c_int, [_hp, ctypes.c_int32, _i32p, _i32p, ctypes.c_int32, _u32p]),
    "gc_ens_efi_score": (ctypes.c_int, [_hp, _hp, _f64p, _f32p, _f64p, _u64p, _u64p, _u64p]),
    "gc_ens_efi_fields": (ctypes.c_int, [_hp, _hp, _f64p]),
    "gc_ens_efi_download": (ctypes.c_int, [_hp, ctypes.c_int32, _f32p]),
    "gc_ens_map_set": (ctypes.c_int, [_hp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32]),
    "gc_ens_map_accumulate": (ctypes.c_int, [_hp, ctypes.c_int32, _f32p]),
    "gc_ens_map_accumulate_events": (ctypes.c_int, [_hp, ctypes.c_int32]),
    "gc_ens_map_download": (ctypes.c_int, [_hp, ctypes.c_int32, _f64p, _u32p, _u32p, _i64p]),
    "gc_ens_map_reset": (ctypes.c_int, [_hp, ctypes.c_int32]),
    "gc_ens_window_set": (ctypes.c_int, [_hp, ctypes.c_int32, ctypes.c_int32, _f64p]),
    "gc_ens_window_push": (ctypes.c_int, [_hp, _hp, _f32p]),
    "gc_ens_window_emit": (ctypes.c_int, [_hp]),
    "gc_ens_window_reset": (ctypes.c_int, [_hp]),
    "gc_ens_energy_set": (ctypes.c_int, [_hp, ctypes.c_int32, _i32p, _f64p]),
    "gc_ens_energy_score": (ctypes.c_int, [_hp, _f32p, _f64p, _f64p, _u64p]),
    "gc_ens_variogram_set": (ctypes.c_int, [_hp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _i32p, ctypes.c_double]),
    "gc_ens_variogram_score": (ctypes.c_int, [_hp, _f32p, _f64p, _u64p]),
    "gc_ens_tail_set": (ctypes.c_int, [_hp, ctypes.c_int32, _f32p, _i32p]),
    "gc_ens_tail_score": (ctypes.c_int, [_hp, _f32p, _f64p, _u64p, _u64p]),
    "gc_ens_region_set": (ctypes.c_int, [_hp, ctypes.c_int32, _u32p]),
    "gc_ens_region_score": (ctypes.c_int, [_hp, _f32p, _f64p, _u64p, _u64p]),
    "gc_ens_feature_set": (ctypes.c_int, [_hp, ctypes.c_int32, ctypes.c_int32, _i32p, _i32p, _i32p, _f32p, ctypes.c_int32,
                                          ctypes.c_int32, _i32p, _i32p, _i32p, _i32p, _f64p, _i32p, _i32p, ctypes.c_int32]),
    "gc_ens_feature": (ctypes.c_int, [_hp, _hp, _f32p]),
    "gc_ens_feature_centres": (ctypes.c_int, [_hp, _i32p, _i32p, _f32p]),
    "gc_comm_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "gc_comm_init": (ctypes.c_int, [_hp, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]),
    "gc_comm_info": (ctypes.c_int, [_hp, _i32p, _i32p]),
    "gc_comm_broadcast_cond": (ctypes.c_int, [_hp, ctypes.c_int32]),
    "gc_comm_allreduce_max": (ctypes.c_int, [_hp, _f64p]),
    "gc_comm_destroy": (ctypes.c_int, [_hp]),
    # include/gencast_hip_debug.h (tests only)
    "gc_debug_fetch": (ctypes.c_int, [_hp, ctypes.c_char_p, _f32p, ctypes.c_int64, _i64p, _i64p]),
    "gc_debug_set_layer_limit": (ctypes.c_int, [_hp, ctypes.c_int32]),
    "gc_debug_set_stop": (ctypes.c_int, [_hp, ctypes.c_int32, ctypes.c_int32]),
    "gc_debug_mesh_permutation": (ctypes.c_int, [_hp, _i32p]),
    "gc_debug_attention_stats": (ctypes.c_int, [_hp, _i64p, _i64p, _i64p]),
}

_lib = None


def load_library(path: Optional[str] = None):
  """Loads (once) and returns the ctypes library; raises if it has not been built."""
  global _lib
  if _lib is not None and path is None:
    return _lib
  # GC_LIB_VARIANT=<name>: an EXPERIMENT build of tools/build_variant.sh (csrc/variants/) -- timing-only ablations
  # that may compute WRONG values by construction.  Honoured only together with GC_ALLOW_EXPERIMENT_LIB=1, and loudly:
  # a stray variable in a real run must not swap the product library silently.
  variant = os.environ.get("GC_LIB_VARIANT")
  if variant and path is None:
    if os.environ.get("GC_ALLOW_EXPERIMENT_LIB") != "1":
      raise GencastHipError(
          f"GC_LIB_VARIANT={variant} asks for an experiment build (tools/build_variant.sh), which may compute wrong values; "
          "set GC_ALLOW_EXPERIMENT_LIB=1 as well to load it, or unset GC_LIB_VARIANT")
    print(f"[gencast_hip] WARNING: loading EXPERIMENT library variant {variant!r} (GC_LIB_VARIANT): timing only, "
          "results are not the product's", file=sys.stderr, flush=True)
  p = path or (os.path.join(_HERE, "csrc", "variants", f"libgencast_hip_{variant}.so") if variant else LIB_PATH)
  if not os.path.exists(p):
    raise GencastHipError(
        f"{p} not found: build it with gencast-flax-nnx_amd/csrc/build.sh "
        "(or __graft_entry__.build()); this package has no CPU fallback")
  lib = ctypes.CDLL(p)
  for name, (res, args) in SIGNATURES.items():
    fn = getattr(lib, name)          # AttributeError if the .so lacks a declared symbol
    fn.restype = res
    fn.argtypes = args
  if lib.gc_abi_version() != 1:
    raise GencastHipError("libgencast_hip.so ABI version mismatch")
  if path is None:
    _lib = lib
  return lib


def _f32(a) -> np.ndarray:
  return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a) -> np.ndarray:
  return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a) -> np.ndarray:
  return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a: np.ndarray, ty):
  return a.ctypes.data_as(ty)


def _opt(a: Optional[np.ndarray], ty):
  """The pointer argument of an optional array: NULL for None."""
  return None if a is None else a.ctypes.data_as(ty)


def _handle_of(other):
  """The C handle argument for another object; NULL for None, which the entries that allow it read as this handle itself."""
  return None if other is None else other._h  # pylint: disable=protected-access


def _need(have, missing: str, call: Optional[str] = None, why: Optional[str] = None) -> None:
  """A state guard: what a C entry would answer with GC_ERR_STATE, said before its result buffers are sized from that state.
  `missing` is what the object lacks and `call` the method that supplies it (`why`: the text in brackets, where it is another)."""
  if not have:
    raise GencastHipError(f"libgencast_hip error 4: no {missing} ({why or call + ' has not been called on this object'})")


def _directions(directions, n: int) -> np.ndarray:
  d = _i32(directions)
  if d.shape != (n,):
    raise ValueError(f"directions must have shape ({n},)")
  return d


def _check_r_lon(r: np.ndarray, n_lon: int, name: str = "r_lon") -> None:
  """A window reaches at most half way round a row of `n_lon` longitudes."""
  if np.any((r < 0) | (r > (n_lon - 1) // 2)):
    raise ValueError(f"{name} must lie in 0 .. {(n_lon - 1) // 2}")


class NativeDenoiser:
  """Owns one `gc_handle` (one GPU, one stream).  Array-level API."""

  def __init__(self, *, latent_size, d_model, num_heads, ffw_hidden, num_layers, c_in, c_out,
               batch=1, device_id=0, noise_num_frequencies=32, noise_hidden=32,
               noise_base_period=16.0, hidden_layers=1):
    self._lib = load_library()
    self.cfg = GcConfig(latent_size, d_model, num_heads, ffw_hidden, num_layers, c_in, c_out, batch,
                        noise_num_frequencies, noise_hidden, noise_base_period)
    self._h = _hp()
    rc = self._lib.gc_create(ctypes.byref(self.cfg), device_id, ctypes.byref(self._h))
    if rc != GC_OK:
      msg = self._lib.gc_last_error(None).decode()
      self._h = None
      if rc in (GC_ERR_INVALID_ARGUMENT, GC_ERR_UNSUPPORTED):
        raise ValueError(msg)
      raise GencastHipError(f"gc_create failed ({rc}): {msg}")
    if int(hidden_layers) != 1:      # DenoiserArchitectureConfig.hidden_layers (denoiser.py:135): before any weight is loaded
      try:
        self.set_option("hidden_layers", str(int(hidden_layers)))
      except Exception:
        self.close()
        raise
    self.num_grid_nodes = None
    self.num_mesh_nodes = None
    self._loss_groups = 0                      # groups of the loss weights this object handed to the handle
    self._ens_members = 0                      # slots of the member store this object reserved on the handle
    self._spec_lmax = 0                        # band limit of the analysis tables this object handed to the handle
    self._event_thresholds = 0                 # threshold fields this object handed to the handle
    self._fss_scales = 0                       # scales of the fractions plan this object handed to the handle
    self._derive_c_src = 0                     # source channels of the derive plan this object handed to the handle
    self._band_c_src = 0                       # source channels of the band plan this object handed to the handle
    self._feature_c_src = 0                    # source channels of the feature plan, and the size of its lists
    self._feature_max = 0
    self._feature_members = -1                 # M of the last ens_feature (-1: none since the plan was set)
    self._order_quantiles = None               # probabilities this object handed to the handle (None: ens_order_set not called)
    self._energy_groups = None                 # groups of the energy plan this object set (None: ens_energy_set not called)
    self._variogram_offsets = None             # offsets of the variogram plan this object set (None: ens_variogram_set not called)
    self._tail_thresholds = 0                  # tail threshold fields this object handed to the handle
    self._regions = 0                          # regions of the plan this object handed to the handle (0: ens_region_set not called)
    self._efi_plan = None                      # (T, E) of the events and bins this object set (None: ens_efi_set not called)
    self._map_plan = None                      # (C', L, T) of the map plan this object set (None: ens_map_set not called)
    self._window_length = 0                    # length of the window plan this object handed to the handle

  # -- plumbing ------------------------------------------------------------------------------
  def _check(self, rc):
    if rc == GC_OK:
      return
    msg = self._lib.gc_last_error(self._h).decode()
    if rc in (GC_ERR_INVALID_ARGUMENT, GC_ERR_UNSUPPORTED):
      raise ValueError(msg)
    raise GencastHipError(f"libgencast_hip error {rc}: {msg}")

  def close(self):
    if getattr(self, "_h", None):
      self._lib.gc_destroy(self._h)
      self._h = None

  @property
  def closed(self) -> bool:
    return not getattr(self, "_h", None)

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  # -- set-up ----------------------------------------------------------------------------------
  def set_option(self, key: str, value: str) -> None:
    self._check(self._lib.gc_set_option(self._h, key.encode(), value.encode()))

  def set_graph(self, graph) -> None:
    """`graph`: geometry.DenoiserGraph (or anything with the same attributes)."""
    g = graph
    arrs = dict(
        g2m_s=_i32(g.g2m_senders), g2m_r=_i32(g.g2m_receivers), m2g_s=_i32(g.m2g_senders),
        m2g_r=_i32(g.m2g_receivers), rowptr=_i32(g.khop_rowptr), cols=_i32(g.khop_cols),
        gs=_f32(g.grid_struct), ms=_f32(g.mesh_struct), e1=_f32(g.g2m_edge_struct),
        e2=_f32(g.m2g_edge_struct))
    xyz = getattr(g, "mesh_xyz", None)
    xyz = None if xyz is None else _f32(xyz)
    G, M = int(g.num_grid_nodes), int(g.num_mesh_nodes)
    if arrs["gs"].shape != (G, 3) or arrs["ms"].shape != (M, 3):
      raise ValueError("structural node features must be [N,3]")
    if arrs["e1"].shape != (len(arrs["g2m_s"]), 4) or arrs["e2"].shape != (len(arrs["m2g_s"]), 4):
      raise ValueError("structural edge features must be [E,4]")
    if len(arrs["g2m_s"]) != len(arrs["g2m_r"]) or len(arrs["m2g_s"]) != len(arrs["m2g_r"]):
      raise ValueError("senders / receivers length mismatch")
    if arrs["rowptr"].shape != (M + 1,) or arrs["rowptr"][-1] != len(arrs["cols"]):
      raise ValueError("khop CSR is inconsistent")
    self._check(self._lib.gc_set_graph(
        self._h, G, M, len(arrs["g2m_s"]), _ptr(arrs["g2m_s"], _i32p), _ptr(arrs["g2m_r"], _i32p),
        len(arrs["m2g_s"]), _ptr(arrs["m2g_s"], _i32p), _ptr(arrs["m2g_r"], _i32p),
        _ptr(arrs["rowptr"], _i32p), _ptr(arrs["cols"], _i32p), _ptr(arrs["gs"], _f32p),
        _ptr(arrs["ms"], _f32p), _ptr(arrs["e1"], _f32p), _ptr(arrs["e2"], _f32p),
        _opt(xyz, _f32p)))
    self.num_grid_nodes, self.num_mesh_nodes = G, M

  def load_weights(self, params: Dict[str, np.ndarray]) -> None:
    for name, w in params.items():
      a = _f32(w)
      shape = (ctypes.c_int64 * a.ndim)(*a.shape)
      self._check(self._lib.gc_load_weight(self._h, name.encode(), _ptr(a, _f32p), shape, a.ndim))

  def missing_weights(self) -> int:
    n = ctypes.c_int32(0)
    self._check(self._lib.gc_missing_weights(self._h, ctypes.byref(n)))
    return n.value

  def finalize(self) -> None:
    self._check(self._lib.gc_finalize(self._h))

  def set_noisy_slots(self, slots) -> None:
    s = _i32(slots)
    if s.shape != (self.cfg.c_out,):
      raise ValueError(f"expected {self.cfg.c_out} noisy slots")
    self._check(self._lib.gc_set_noisy_slots(self._h, _ptr(s, _i32p)))

  # -- compute -----------------------------------------------------------------------------------
  def _shape_in(self):
    return (self.num_grid_nodes, self.cfg.batch, self.cfg.c_in)

  def _shape_out(self):
    return (self.num_grid_nodes, self.cfg.batch, self.cfg.c_out)

  def _field(self, dtype=np.float32) -> np.ndarray:
    """An output buffer for one [G, B, c_out] field."""
    return np.empty(self._shape_out(), dtype=dtype)

  def _download(self, entry, *args, shape=None) -> np.ndarray:
    """`entry(handle, *args, out)` into a fresh float32 field ([G, B, c_out] unless `shape` says otherwise), which it returns."""
    out = self._field() if shape is None else np.empty(shape, dtype=np.float32)
    self._check(entry(self._h, *args, _ptr(out, _f32p)))
    return out

  def _need_store(self) -> None:
    _need(self._ens_members, "member store", "ens_reserve")

  def _truth_arg(self, truth, channels: Optional[int] = None) -> Optional[np.ndarray]:
    """The optional truth of a scorer as float32 [G, B, c_out] ([G, B, `channels`] for the source of a view), or None."""
    if truth is None:
      return None
    t = _f32(truth)
    want = self._shape_out() if channels is None else (self.num_grid_nodes, self.cfg.batch, channels)
    if t.shape != want:
      raise ValueError(f"truth must be {want}, got {t.shape}")
    return t

  def _check_src(self, src) -> None:
    """`src` is the object whose store a view of this one reads."""
    if not isinstance(src, NativeDenoiser) or src is self:
      raise ValueError("src must be another NativeDenoiser")

  def _check_clim(self, clim) -> None:
    """`clim` is the object that holds the climatological samples."""
    if not isinstance(clim, NativeDenoiser):
      raise TypeError("clim must be a NativeDenoiser")
    if clim is self:
      raise ValueError("the climatology must be another handle")

  def _weights_q_arg(self, node_weight_q) -> np.ndarray:
    w = np.asarray(node_weight_q)
    if w.shape != (self.num_grid_nodes,) or w.dtype.kind not in "ui" or (w.size and (w.min() < 0 or w.max() > 0xFFFFFFFF)):
      raise ValueError(f"node_weight_q must be unsigned 32-bit integers of shape ({self.num_grid_nodes},)")
    return np.ascontiguousarray(w, dtype=np.uint32)

  def _thresholds_arg(self, thresholds) -> np.ndarray:
    thr = _f32(thresholds)
    if thr.ndim != 4 or thr.shape[1:] != self._shape_out():
      raise ValueError(f"thresholds must be [T, {', '.join(str(n) for n in self._shape_out())}], got {thr.shape}")
    return thr

  def denoise(self, grid_feats, sigma) -> np.ndarray:
    x = _f32(grid_feats)
    s = _f32(sigma).reshape(-1)
    if x.shape != self._shape_in():
      raise ValueError(f"grid_feats must be {self._shape_in()}, got {x.shape}")
    if s.shape != (self.cfg.batch,):
      raise ValueError("noise_levels expected to be shape (batch,).")
    out = self._field()
    self._check(self._lib.gc_denoise(self._h, _ptr(x, _f32p), _ptr(s, _f32p), _ptr(out, _f32p)))
    return out

  def sample(self, cond_feats, init_noise, sigmas, skip_dead_call=True):
    c, z, sg = _f32(cond_feats), _f32(init_noise), _f32(sigmas).reshape(-1)
    if c.shape != self._shape_in():
      raise ValueError(f"cond_feats must be {self._shape_in()}, got {c.shape}")
    if z.shape != self._shape_out():
      raise ValueError(f"init_noise must be {self._shape_out()}, got {z.shape}")
    out = self._field()
    st = GcSampleStats()
    self._check(self._lib.gc_sample(self._h, _ptr(c, _f32p), _ptr(z, _f32p), _ptr(sg, _f32p),
                                    len(sg) - 1, int(bool(skip_dead_call)), _ptr(out, _f32p),
                                    ctypes.byref(st)))
    return out, dict(denoiser_calls=st.denoiser_calls, device_ms=st.device_ms)

  def upload_cond(self, cond_feats):
    c = _f32(cond_feats)
    if c.shape != self._shape_in():
      raise ValueError(f"cond_feats must be {self._shape_in()}, got {c.shape}")
    self._check(self._lib.gc_upload_cond(self._h, _ptr(c, _f32p)))

  def upload_cond_dev(self, dev_ptr: int):
    self._check(self._lib.gc_upload_cond_dev(self._h, ctypes.c_void_p(dev_ptr)))

  def cond_device_ptr(self):
    p, n = ctypes.c_void_p(), ctypes.c_int64()
    self._check(self._lib.gc_cond_device_ptr(self._h, ctypes.byref(p), ctypes.byref(n)))
    return p.value, n.value

  def commit_cond(self):
    self._check(self._lib.gc_commit_cond(self._h))

  def upload_noise(self, init_noise):
    z = _f32(init_noise)
    if z.shape != self._shape_out():
      raise ValueError(f"init_noise must be {self._shape_out()}, got {z.shape}")
    self._check(self._lib.gc_upload_noise(self._h, _ptr(z, _f32p)))

  def sample_resident(self, sigmas, skip_dead_call=True, want_stats=True):
    sg = _f32(sigmas).reshape(-1)
    st = GcSampleStats()
    self._check(self._lib.gc_sample_resident(self._h, _ptr(sg, _f32p), len(sg) - 1,
                                             int(bool(skip_dead_call)),
                                             ctypes.byref(st) if want_stats else None))
    return dict(denoiser_calls=st.denoiser_calls, device_ms=st.device_ms) if want_stats else None

  def download_sample(self) -> np.ndarray:
    return self._download(self._lib.gc_download_sample)

  def stash_sample(self) -> None:
    """Waits for the last sample and snapshots it on the device (gc_stash_sample): the handle is free for the next step."""
    self._check(self._lib.gc_stash_sample(self._h))

  def download_stash(self) -> np.ndarray:
    """Copies the snapshot to the host on a side stream while the main stream keeps running (gc_download_stash)."""
    return self._download(self._lib.gc_download_stash)

  def rollout_plan(self, kind, src, sidx, a, b, n_forcing: int):
    """Per-channel context-update plan (gc_rollout_plan; kinds documented in gencast_hip.h)."""
    kind, src, sidx, a, b = _i32(kind), _i32(src), _i32(sidx), _f32(a), _f32(b)
    for arr in (kind, src, sidx, a, b):
      if arr.shape != (self.cfg.c_in,):
        raise ValueError(f"plan arrays must have shape ({self.cfg.c_in},)")
    self._check(self._lib.gc_rollout_plan(self._h, _ptr(kind, _i32p), _ptr(src, _i32p), _ptr(sidx, _i32p),
                                          _ptr(a, _f32p), _ptr(b, _f32p), int(n_forcing)))
    self._n_forcing = int(n_forcing)

  def rollout_advance(self, forcings=None):
    """Applies the plan to the resident conditioning using the last sample (gc_rollout_advance)."""
    if forcings is None:
      self._check(self._lib.gc_rollout_advance(self._h, None))
      return
    forcings = _f32(forcings)
    want = (self.num_grid_nodes, self.cfg.batch, getattr(self, "_n_forcing", -1))
    if forcings.shape != want:
      raise ValueError(f"forcings must have shape {want}")
    self._check(self._lib.gc_rollout_advance(self._h, _ptr(forcings, _f32p)))

  def download_cond(self) -> np.ndarray:
    return self._download(self._lib.gc_download_cond, shape=self._shape_in())

  def sync(self):
    self._check(self._lib.gc_sync(self._h))

  # -- measurement ---------------------------------------------------------------------------------
  def kernel_classes(self):
    return [self._lib.gc_kernel_class_name(i).decode()
            for i in range(self._lib.gc_num_kernel_classes())]

  def profile_enable(self, cls: int):
    self._check(self._lib.gc_profile_enable(self._h, cls))

  def profile_set_stride(self, stride: int):
    self._check(self._lib.gc_profile_set_stride(self._h, stride))

  def profile_read(self):
    n, ms = ctypes.c_int32(), ctypes.c_float()
    self._check(self._lib.gc_profile_read(self._h, ctypes.byref(n), ctypes.byref(ms)))
    return n.value, ms.value

  def algorithmic_work(self):
    f, b = ctypes.c_double(), ctypes.c_double()
    self._check(self._lib.gc_algorithmic_work(self._h, ctypes.byref(f), ctypes.byref(b)))
    return f.value, b.value

  # -- spherical noise on the device, stochastic churn ----------------------------------------------
  def noise_set_tables(self, n_lat: int, n_lon: int, legendre, cos_table, sin_table) -> None:
    """Tables of `noise.SphericalNoise.device_tables()`: legendre [L, n_lat, L], cos / sin [n_lon, L]."""
    leg, ct, st = _f32(legendre), _f32(cos_table), _f32(sin_table)
    L = leg.shape[0]
    if leg.shape != (L, n_lat, L) or ct.shape != (n_lon, L) or st.shape != (n_lon, L):
      raise ValueError("noise tables must be legendre [L, n_lat, L], cos / sin [n_lon, L]")
    self._check(self._lib.gc_noise_set_tables(self._h, int(n_lat), int(n_lon), int(L), _ptr(leg, _f32p),
                                              _ptr(ct, _f32p), _ptr(st, _f32p)))

  def noise_seed(self, seed: int, stream: int = 0) -> None:
    self._check(self._lib.gc_noise_seed(self._h, ctypes.c_uint64(int(seed) & (2 ** 64 - 1)),
                                        ctypes.c_uint64(int(stream) & (2 ** 64 - 1))))

  def noise_draw(self) -> None:
    self._check(self._lib.gc_noise_draw(self._h))

  def download_noise(self) -> np.ndarray:
    return self._download(self._lib.gc_download_noise)

  def set_churn(self, rates, noise_level_inflation_factor: float = 1.0) -> None:
    """Per-step churn rates for the following sample calls (None / all zero: off)."""
    if rates is None:
      self._check(self._lib.gc_set_churn(self._h, None, 0, float(noise_level_inflation_factor)))
      return
    r = _f32(rates).reshape(-1)
    self._check(self._lib.gc_set_churn(self._h, _ptr(r, _f32p), len(r), float(noise_level_inflation_factor)))

  # -- denoising loss (forward only) ----------------------------------------------------------------
  def loss_set_weights(self, node_weight, channel_weight, channel_group, group_weight) -> None:
    """Flat loss weights (gc_loss_set_weights; `losses.loss_plan` builds them): node_weight [G], channel_weight and
    channel_group [c_out], group_weight [n_groups]."""
    nw, cw, gw = _f32(node_weight), _f32(channel_weight), _f32(group_weight)
    cg = _i32(channel_group)
    if nw.shape != (self.num_grid_nodes,):
      raise ValueError(f"node_weight must have shape ({self.num_grid_nodes},)")
    if cw.shape != (self.cfg.c_out,) or cg.shape != (self.cfg.c_out,):
      raise ValueError(f"channel_weight / channel_group must have shape ({self.cfg.c_out},)")
    if gw.ndim != 1:
      raise ValueError("group_weight must be one-dimensional")
    self._check(self._lib.gc_loss_set_weights(self._h, _ptr(nw, _f32p), _ptr(cw, _f32p), _ptr(cg, _i32p), len(gw),
                                              _ptr(gw, _f32p)))
    self._loss_groups = len(gw)

  def _need_loss_groups(self) -> int:
    """The result buffers are sized by the group count: the weights must have gone through `loss_set_weights`."""
    _need(self._loss_groups, "loss weights", "loss_set_weights")
    return self._loss_groups

  def upload_targets(self, targets) -> None:
    t = _f32(targets)
    if t.shape != self._shape_out():
      raise ValueError(f"targets must be {self._shape_out()}, got {t.shape}")
    self._check(self._lib.gc_upload_targets(self._h, _ptr(t, _f32p)))

  def loss_resident(self, sigmas, draw_noise: bool = False):
    """`sigmas` [n_eval, B] (or [B]: one evaluation) -> (loss [n_eval, B], per_group [n_eval, B, n_groups]) on the
    resident conditioning and targets (gc_loss_resident)."""
    sg = _f32(sigmas)
    sg = sg.reshape(1, -1) if sg.ndim == 1 else sg
    if sg.ndim != 2 or sg.shape[1] != self.cfg.batch or sg.shape[0] < 1:
      raise ValueError("noise_levels expected to be shape (n_eval, batch).")
    ng = self._need_loss_groups()
    loss = np.empty((sg.shape[0], self.cfg.batch), dtype=np.float32)
    per_group = np.empty((sg.shape[0], self.cfg.batch, ng), dtype=np.float32)
    self._check(self._lib.gc_loss_resident(self._h, _ptr(sg, _f32p), sg.shape[0], int(bool(draw_noise)),
                                           _ptr(loss, _f32p), _ptr(per_group, _f32p)))
    return loss, per_group

  def download_denoised(self) -> np.ndarray:
    """The preconditioned prediction D of the last loss evaluation (gc_download_denoised)."""
    return self._download(self._lib.gc_download_denoised)

  def loss(self, cond_feats, targets, noise, sigma, want_denoised: bool = False):
    """One evaluation from host arrays (gc_loss) -> (loss [B], per_group [B, n_groups][, D [G, B, c_out]])."""
    c, t, z, sg = _f32(cond_feats), _f32(targets), _f32(noise), _f32(sigma).reshape(-1)
    if c.shape != self._shape_in():
      raise ValueError(f"cond_feats must be {self._shape_in()}, got {c.shape}")
    if t.shape != self._shape_out() or z.shape != self._shape_out():
      raise ValueError(f"targets and noise must be {self._shape_out()}")
    if sg.shape != (self.cfg.batch,):
      raise ValueError("noise_levels expected to be shape (batch,).")
    ng = self._need_loss_groups()
    loss = np.empty((self.cfg.batch,), dtype=np.float32)
    per_group = np.empty((self.cfg.batch, ng), dtype=np.float32)
    den = self._field() if want_denoised else None
    self._check(self._lib.gc_loss(self._h, _ptr(c, _f32p), _ptr(t, _f32p), _ptr(z, _f32p), _ptr(sg, _f32p),
                                  _ptr(loss, _f32p), _ptr(per_group, _f32p), _opt(den, _f32p)))
    return (loss, per_group, den) if want_denoised else (loss, per_group)

  # -- ensemble verification (scored on the device) -------------------------------------------------
  def ens_reserve(self, n_members: int) -> None:
    """A store of `n_members` (2..64) member fields on the handle; empties an earlier one (gc_ens_reserve)."""
    self._check(self._lib.gc_ens_reserve(self._h, int(n_members)))
    self._ens_members = int(n_members)

  def ens_set_node_weight(self, node_weight) -> None:
    w = _f32(node_weight)
    if w.shape != (self.num_grid_nodes,):
      raise ValueError(f"node_weight must have shape ({self.num_grid_nodes},)")
    self._check(self._lib.gc_ens_set_node_weight(self._h, _ptr(w, _f32p)))

  def ens_push(self, slot: int, src: Optional["NativeDenoiser"] = None) -> None:
    """Slot <- the last sample of `src` (None: of this handle), device to device (gc_ens_push)."""
    self._check(self._lib.gc_ens_push(self._h, int(slot), _handle_of(src)))

  def ens_push_host(self, slot: int, field) -> None:
    x = _f32(field)
    if x.shape != self._shape_out():
      raise ValueError(f"field must be {self._shape_out()}, got {x.shape}")
    self._check(self._lib.gc_ens_push_host(self._h, int(slot), _ptr(x, _f32p)))

  def ens_score(self, truth=None, want_fields: bool = False):
    """-> (sums [B, c_out, 6] float64, rank_hist [B, c_out, M + 1] uint64): the raw, additive sums of gc_ens_score
    (`verification.EnsembleScores` derives the scores).  `truth` [G, B, c_out], or None = the truth uploaded last."""
    self._need_store()
    t = self._truth_arg(truth)
    B, C = self.cfg.batch, self.cfg.c_out
    sums = np.empty((6, B, C), dtype=np.float64)
    hist = np.empty((B, C, self._ens_members + 1), dtype=np.uint64)
    self._check(self._lib.gc_ens_score(self._h, _opt(t, _f32p), int(bool(want_fields)), _ptr(sums, _f64p), _ptr(hist, _u64p)))
    return np.ascontiguousarray(np.moveaxis(sums, 0, -1)), hist

  def ens_download_fields(self):
    """(mean, variance) [G, B, c_out] of the last `ens_score(want_fields=True)` (gc_ens_download_fields)."""
    mean, var = self._field(), self._field()
    self._check(self._lib.gc_ens_download_fields(self._h, _ptr(mean, _f32p), _ptr(var, _f32p)))
    return mean, var

  def ens_push_state(self, slot: int, state_src, src: Optional["NativeDenoiser"] = None) -> None:
    """Slot <- the STATE of `src` (None: of this handle): channel j from conditioning channel `state_src[j]` of the
    advanced context, from the sample where `state_src[j] < 0` (gc_ens_push_state; `rollout.state_channels`)."""
    t = _i32(state_src)
    if t.shape != (self.cfg.c_out,):
      raise ValueError(f"state_src must have shape ({self.cfg.c_out},)")
    self._check(self._lib.gc_ens_push_state(self._h, int(slot), _handle_of(src), _ptr(t, _i32p)))

  def ens_download_member(self, slot: int) -> np.ndarray:
    """One stored member [G, B, c_out] (gc_ens_download_member)."""
    return self._download(self._lib.gc_ens_download_member, int(slot))

  # -- ensemble event verification (exceedance tables formed on the device) ---------------------------
  def ens_event_set(self, thresholds, directions, node_weight_q) -> None:
    """`thresholds` [T, G, B, c_out] float32 (T in 1..8; NaN = not evaluated there), `directions` [T] (> 0: the event is
    `value > threshold`, < 0: `value < threshold`), `node_weight_q` [G] uint32 (`verification.quantize_node_weights`):
    gc_ens_event_set; needs `set_graph` only and survives `ens_reserve`."""
    thr = self._thresholds_arg(thresholds)
    d = _directions(directions, thr.shape[0])
    w = self._weights_q_arg(node_weight_q)
    self._check(self._lib.gc_ens_event_set(self._h, thr.shape[0], _ptr(thr, _f32p), _ptr(d, _i32p), _ptr(w, _u32p)))
    self._event_thresholds = int(thr.shape[0])

  def ens_event_score(self, truth=None):
    """-> (weighted [T, B, c_out, 2, M + 1] uint64, counts (same shape), invalid [T] uint64): the integer tables of
    gc_ens_event_score over the member store (`verification.EventScores` derives the scores).  `truth` [G, B, c_out], or
    None = the truth uploaded last (shared with `ens_score` / `ens_spectrum`)."""
    _need(self._event_thresholds, "thresholds", "ens_event_set")
    self._need_store()
    t = self._truth_arg(truth)
    T, B, C = self._event_thresholds, self.cfg.batch, self.cfg.c_out
    weighted = np.empty((T, B, C, 2, self._ens_members + 1), dtype=np.uint64)
    counts = np.empty_like(weighted)
    invalid = np.empty(T, dtype=np.uint64)
    self._check(self._lib.gc_ens_event_score(self._h, _opt(t, _f32p), _ptr(weighted, _u64p), _ptr(counts, _u64p),
                                             _ptr(invalid, _u64p)))
    return weighted, counts, invalid

  def ens_event_codes(self, t: int) -> np.ndarray:
    """uint8 [G, B, c_out] of threshold `t` from the last `ens_event_score`: k | (o << 7), 255 where the point did not
    count (gc_ens_event_download; `verification.event_probability` decodes)."""
    _need(self._event_thresholds, "thresholds", "ens_event_set")
    code = self._field(np.uint8)
    self._check(self._lib.gc_ens_event_download(self._h, int(t), _ptr(code, _u8p)))
    return code

  # -- fractions skill score (neighbourhood fractions of the event codes, S scales from one pass) -------
  def ens_fss_set(self, r_lat, r_lon, row_wq, n_lon: Optional[int] = None) -> None:
    """The plan of `ens_fss_score` (gc_ens_fss_set; needs `set_graph` only, survives `ens_reserve`): per scale s the window of
    `r_lat[s]` rows either side and `r_lon[s, i']` longitudes either side in row i' (wrapping), as in `ens_derive_set`;
    `r_lat` [S], `r_lon` [S, n_lat], S in 1..8; `row_wq` [n_lat] integer row weights in 1 .. 2^24 - 1
    (`verification.quantize_row_weights`); the grid is n_lat x `n_lon` (None: G / n_lat), node = lat_i n_lon + lon_j.
    `verification.EventSpec.windows` builds these arrays from `scales_km`."""
    rl, ro = _i32(r_lat), _i32(r_lon)
    if rl.ndim != 1 or not 1 <= rl.shape[0] <= 8:
      raise ValueError(f"r_lat must hold 1..8 scales, got shape {rl.shape}")
    if ro.ndim != 2 or ro.shape[0] != rl.shape[0] or ro.shape[1] < 1:
      raise ValueError(f"r_lon must have shape ({rl.shape[0]}, n_lat), got {ro.shape}")
    n_lat = int(ro.shape[1])
    n_lon = self.num_grid_nodes // n_lat if n_lon is None else int(n_lon)
    if n_lon < 1 or n_lat * n_lon != self.num_grid_nodes:
      raise ValueError(f"n_lat * n_lon = {n_lat} * {n_lon} must equal the number of grid nodes {self.num_grid_nodes}")
    if np.any(rl < 0):
      raise ValueError("r_lat must be >= 0")
    _check_r_lon(ro, n_lon)
    w = np.asarray(row_wq)
    if w.shape != (n_lat,) or w.dtype.kind not in "ui" or np.any(w < 1) or np.any(w > 2 ** 24 - 1):
      raise ValueError(f"row_wq must be integers in 1 .. 2^24 - 1 of shape ({n_lat},)")
    w = np.ascontiguousarray(w, dtype=np.uint32)
    self._check(self._lib.gc_ens_fss_set(self._h, rl.shape[0], n_lat, n_lon, _ptr(rl, _i32p), _ptr(ro, _i32p), _ptr(w, _u32p)))
    self._fss_scales = int(rl.shape[0])

  def ens_fss_score(self) -> np.ndarray:
    """-> sums [T, S, B, c_out, 4] float64 of gc_ens_fss_score: sum w (P - O)^2, sum w (P^2 + O^2), sum w P, sum w O over the
    counted centres, from the event codes the last `ens_event_score` left on the device (`verification.FractionsScores`
    derives the scores)."""
    _need(self._fss_scales, "plan", "ens_fss_set")
    _need(self._event_thresholds, "thresholds", "ens_event_set")
    sums = np.empty((self._event_thresholds, self._fss_scales, self.cfg.batch, self.cfg.c_out, 4), dtype=np.float64)
    self._check(self._lib.gc_ens_fss_score(self._h, _ptr(sums, _f64p)))
    return sums

  def ens_fss_fields(self, t: int, s: int):
    """-> (prob, obs), float32 [G, B, c_out] each: the neighbourhood ensemble probability P and the observed fraction O of
    threshold `t` at scale `s`, NaN where the point did not count (gc_ens_fss_fields)."""
    _need(self._fss_scales, "plan", "ens_fss_set")
    _need(self._event_thresholds, "thresholds", "ens_event_set")
    if not 0 <= int(t) < self._event_thresholds:
      raise ValueError(f"t must lie in [0, {self._event_thresholds})")
    if not 0 <= int(s) < self._fss_scales:
      raise ValueError(f"s must lie in [0, {self._fss_scales})")
    prob, obs = self._field(), self._field()
    self._check(self._lib.gc_ens_fss_fields(self._h, int(t), int(s), _ptr(prob, _f32p), _ptr(obs, _f32p)))
    return prob, obs

  # -- derived and pooled ensemble fields (formed on the device, into this handle's member store) -------
  def ens_derive_set(self, c_src: int, op, src_a, src_b, affine, pool: int = 0, n_lat: Optional[int] = None,
                     n_lon: Optional[int] = None, r_lat: int = 0, r_lon=None, row_weight=None, *, scale=None, loc=None,
                     term_start=None, term_coef=None, term_a=None, term_b=None, coslat=None, inv_rcos=None, inv_dphi=None,
                     inv_2dlam=None, pole_row=None) -> None:
    """The plan of `ens_derive` for this handle's c_out = c_d derived channels (gc_ens_derive_set; needs `set_graph` only,
    survives `ens_reserve`).  `op` [c_d]: 0 copy of source channel `src_a[j]`, 1 norm2 = sqrt(u^2 + v^2) in double with
    u = x[src_a[j]] sa + la, v = x[src_b[j]] sb + lb and `affine[j]` = (sa, la, sb, lb).  `pool`: 0 none, 1 max, 2 min,
    3 mean over the window of `r_lat` rows either side and `r_lon[i']` longitudes either side in row i' (wrapping), the mean
    weighted with `row_weight[i']`; `n_lat` x `n_lon` is the grid (node = lat_i n_lon + lon_j).  `verification.DerivedSpec`
    builds these arrays from variable names.

    With `scale` and `loc` [c_src] the plan goes through gc_ens_derive_set_expr and `op` may also be 2 sum, 3 norm (term
    lists: `term_start` [c_d, 3], `term_coef`, `term_a`, `term_b` [n_terms]), 4 vorticity and 5 divergence of u = `src_a[j]`,
    v = `src_b[j]` (row tables `coslat`, `inv_rcos`, `inv_dphi`, `pole_row` [n_lat] and `inv_2dlam`); include/gencast_hip.h
    has the definitions.  Without them the call is gc_ens_derive_set, as before."""
    c_d = self.cfg.c_out
    if int(c_src) < 1:
      raise ValueError("c_src must be positive")
    o, a, b = _i32(op), _i32(src_a), _i32(src_b)
    if o.shape != (c_d,) or a.shape != (c_d,) or b.shape != (c_d,):
      raise ValueError(f"op, src_a and src_b must have shape ({c_d},)")
    expr = scale is not None or loc is not None
    if not expr:
      given = dict(term_start=term_start, term_coef=term_coef, term_a=term_a, term_b=term_b, coslat=coslat, inv_rcos=inv_rcos,
                   inv_dphi=inv_dphi, inv_2dlam=inv_2dlam, pole_row=pole_row)
      if any(v is not None for v in given.values()):
        raise ValueError(f"{sorted(k for k, v in given.items() if v is not None)} need scale and loc")
      if np.any((o != 0) & (o != 1)):
        raise ValueError("op must be 0 (copy) or 1 (norm2)")
    elif np.any((o < 0) | (o > 5)):
      raise ValueError("op must be 0 (copy), 1 (norm2), 2 (sum), 3 (norm), 4 (vorticity) or 5 (divergence)")
    lists = (o == 2) | (o == 3)
    if np.any(~lists & ((a < 0) | (a >= c_src))) or np.any(~lists & (o != 0) & ((b < 0) | (b >= c_src))):
      raise ValueError(f"a source channel lies outside [0, {int(c_src)})")
    aff = _f64(affine)
    if aff.shape != (c_d, 4):
      raise ValueError(f"affine must have shape ({c_d}, 4)")
    if int(pool) not in (0, 1, 2, 3):
      raise ValueError("pool must be 0 (none), 1 (max), 2 (min) or 3 (mean)")
    if n_lat is None or n_lon is None or int(n_lat) * int(n_lon) != self.num_grid_nodes:
      raise ValueError(f"n_lat * n_lon must equal the number of grid nodes ({self.num_grid_nodes})")
    if int(r_lat) < 0:
      raise ValueError("r_lat must be >= 0")
    r = w = None
    if int(pool) != 0:
      if r_lon is None or row_weight is None:
        raise ValueError("a pooled plan needs r_lon and row_weight")
      r = _i32(r_lon)
      w = _f64(row_weight)
      if r.shape != (int(n_lat),) or w.shape != (int(n_lat),):
        raise ValueError(f"r_lon and row_weight must have shape ({int(n_lat)},)")
      _check_r_lon(r, int(n_lon))
      if not np.all(np.isfinite(w) & (w > 0.0)):
        raise ValueError("row_weight must be finite and > 0")
    plain = (self._h, int(c_src), _ptr(o, _i32p), _ptr(a, _i32p), _ptr(b, _i32p), _ptr(aff, _f64p), int(pool), int(n_lat),
             int(n_lon), int(r_lat), _opt(r, _i32p), _opt(w, _f64p))         # (the expression form takes these first)
    if not expr:
      self._check(self._lib.gc_ens_derive_set(*plain))
      self._derive_c_src = int(c_src)
      return
    if scale is None or loc is None:
      raise ValueError("scale and loc go together")
    sc, lo = _f64(scale), _f64(loc)
    if sc.shape != (int(c_src),) or lo.shape != (int(c_src),) or not (np.isfinite(sc).all() and np.isfinite(lo).all()):
      raise ValueError(f"scale and loc must be finite and have shape ({int(c_src)},)")
    tc = _f64(np.zeros(0) if term_coef is None else term_coef).reshape(-1)
    ta, tb = (_i32(np.zeros(0, np.int32) if v is None else v).reshape(-1) for v in (term_a, term_b))
    if not tc.shape == ta.shape == tb.shape:
      raise ValueError("term_coef, term_a and term_b must have one entry per term")
    if not np.isfinite(tc).all():
      raise ValueError("a term coefficient is not finite")
    if np.any((ta < 0) | (ta >= c_src) | (tb < -1) | (tb >= c_src)):
      raise ValueError(f"a term's source channel lies outside [0, {int(c_src)}) (term_b: -1 for none)")
    ts = None
    if lists.any():
      if term_start is None:
        raise ValueError("a sum or norm channel needs term_start")
      ts = _i32(term_start)
      if ts.shape != (c_d, 3):
        raise ValueError(f"term_start must have shape ({c_d}, 3)")
      s0, s1, s2 = ts[lists].T
      if np.any((s0 < 0) | (s1 <= s0) | (s2 < s1) | (s2 > tc.size) | ((s2 > s1) != (o[lists] == 3))):
        raise ValueError("term_start: a sum takes one list of terms inside the table, a norm two, none of them empty")
    rows = [None] * 4
    if np.any(o >= 4):
      if any(v is None for v in (coslat, inv_rcos, inv_dphi, inv_2dlam, pole_row)):
        raise ValueError("vorticity and divergence need coslat, inv_rcos, inv_dphi, inv_2dlam and pole_row")
      if int(n_lon) < 3 or int(n_lat) < 2:
        raise ValueError("vorticity and divergence need n_lon >= 3 and n_lat >= 2")
      rows = [_f64(coslat), _f64(inv_rcos), _f64(inv_dphi), _i32(pole_row)]
      if any(v.shape != (int(n_lat),) for v in rows):
        raise ValueError(f"coslat, inv_rcos, inv_dphi and pole_row must have shape ({int(n_lat)},)")
    self._check(self._lib.gc_ens_derive_set_expr(
        *plain, _ptr(sc, _f64p), _ptr(lo, _f64p), _opt(ts, _i32p), int(tc.size), _ptr(tc, _f64p), _ptr(ta, _i32p), _ptr(tb, _i32p),
        *(_opt(v, _f64p) for v in rows[:3]), 0.0 if inv_2dlam is None else float(inv_2dlam), _opt(rows[3], _i32p)))
    self._derive_c_src = int(c_src)

  def ens_derive(self, src: "NativeDenoiser", truth=None) -> None:
    """Every slot of this handle's member store <- the derived (and pooled) member of `src`'s store, this handle's truth <-
    the derived truth of `src` (gc_ens_derive): afterwards `ens_score(None)`, `ens_event_score(None)`, `ens_spectrum(None)`
    and `ens_download_member` of THIS handle see the derived fields.  `truth` [G, B, c_src] is uploaded into `src`, or
    None = the truth `src` holds."""
    _need(self._derive_c_src, "plan", "ens_derive_set")
    self._check_src(src)
    t = self._truth_arg(truth, self._derive_c_src)
    self._check(self._lib.gc_ens_derive(self._h, _handle_of(src), _opt(t, _f32p)))

  # -- spectral band views (band-limited members and truth, into this handle's member store) -----------------
  def ens_band_set(self, c_src: int, response, complement, src_channel, band, legendre_synthesis, cos_s, sin_s) -> None:
    """The plan of `ens_band` for this handle's c_out = c_d derived channels (gc_ens_band_set; needs `set_graph` and
    `spec_set_tables`, survives `ens_reserve`, dropped by the next `spec_set_tables`).  `response` [K, lmax] float64 (K in
    1..8): the weight of every total wavenumber in band k; `complement` [K]: the band's field is f - synth(w a) instead of
    synth(w a); derived channel j is band `band[j]` of source channel `src_channel[j]`.  `legendre_synthesis` [lmax, n_lat,
    lmax], `cos_s`, `sin_s` [lmax, n_lon]: `spectra.SphericalAnalysis.synthesis_tables()`.  `verification.BandSpec` builds
    these arrays from variable names."""
    _need(self._spec_lmax, "analysis tables", "spec_set_tables")
    c_d, L = self.cfg.c_out, self._spec_lmax
    if int(c_src) < 1:
      raise ValueError("c_src must be positive")
    w = _f64(response)
    if w.ndim != 2 or not 1 <= w.shape[0] <= 8 or w.shape[1] != L:
      raise ValueError(f"response must be [K, {L}] with K in 1..8, got {w.shape}")
    if not np.isfinite(w).all():
      raise ValueError("a response value is not finite")
    comp = _i32(np.asarray(complement).astype(np.int32))
    if comp.shape != (w.shape[0],):
      raise ValueError(f"complement must have shape ({w.shape[0]},)")
    ch, bd = _i32(src_channel), _i32(band)
    if ch.shape != (c_d,) or bd.shape != (c_d,):
      raise ValueError(f"src_channel and band must have shape ({c_d},)")
    if np.any((ch < 0) | (ch >= int(c_src))):
      raise ValueError(f"a source channel lies outside [0, {int(c_src)})")
    if np.any((bd < 0) | (bd >= w.shape[0])):
      raise ValueError(f"a band index lies outside [0, {w.shape[0]})")
    leg, cs, sn = _f32(legendre_synthesis), _f32(cos_s), _f32(sin_s)
    if leg.ndim != 3 or leg.shape[0] != L or leg.shape[2] != L or leg.shape[1] * cs.shape[-1] != self.num_grid_nodes:
      raise ValueError(f"legendre_synthesis must be [{L}, n_lat, {L}] with n_lat * n_lon = {self.num_grid_nodes}, got {leg.shape}")
    if cs.shape != (L, cs.shape[-1]) or sn.shape != cs.shape:
      raise ValueError(f"cos_s and sin_s must be [{L}, n_lon], got {cs.shape} and {sn.shape}")
    self._check(self._lib.gc_ens_band_set(self._h, int(c_src), int(w.shape[0]), _ptr(w, _f64p), _ptr(comp, _i32p), _ptr(ch, _i32p),
                                          _ptr(bd, _i32p), _ptr(leg, _f32p), _ptr(cs, _f32p), _ptr(sn, _f32p)))
    self._band_c_src = int(c_src)

  def ens_band(self, src: "NativeDenoiser", truth=None) -> None:
    """Every slot of this handle's member store <- the band fields of the member of `src`'s store, this handle's truth <- the
    band fields of the truth of `src` (gc_ens_band): afterwards every scorer of THIS handle sees the band-limited fields.
    `truth` [G, B, c_src] is uploaded into `src`, or None = the truth `src` holds.  A band is linear: a view of `x s + l` is
    `s view(x) + l w[0]` (`l (1 - w[0])` with complement); with float32 tables a constant comes back within a few 1e-7
    relative."""
    _need(self._band_c_src, "plan", "ens_band_set")
    self._check_src(src)
    t = self._truth_arg(truth, self._band_c_src)
    self._check(self._lib.gc_ens_band(self._h, _handle_of(src), _opt(t, _f32p)))

  # -- ensemble feature detection (centres and strike fields, into this handle's member store) -------------
  def ens_feature_set(self, c_src: int, channel, direction, use_threshold, threshold, n_lat: int, n_lon: int, r_lat, r_lon,
                      ring_lat, ring_lon, depth, strike_lat, strike_lon, max_centres: int = 64) -> None:
    """The plan of `ens_feature` for this handle's c_out = D detectors (gc_ens_feature_set; needs `set_graph` only, survives
    `ens_reserve`).  Per detector: the source `channel`, `direction` (< 0 a minimum, > 0 a maximum), `use_threshold` and
    `threshold` (the members' units), the extremum window `r_lat`, `r_lon` [D, n_lat], the ring `ring_lat` (0: no ring test),
    `ring_lon` [D, n_lat] and its `depth` (the members' units), the strike window `strike_lat`, `strike_lon` [D, n_lat];
    `max_centres` (1..1024) entries per list.  `verification.FeatureSpec` builds these arrays from variable names."""
    D = self.cfg.c_out
    if not 1 <= D <= 8:
      raise ValueError(f"a feature plan needs a handle with c_out in 1 .. 8, got {D}")
    if int(c_src) < 1:
      raise ValueError("c_src must be positive")
    if n_lat is None or n_lon is None or int(n_lat) * int(n_lon) != self.num_grid_nodes:
      raise ValueError(f"n_lat * n_lon must equal the number of grid nodes ({self.num_grid_nodes})")
    n_lat, n_lon = int(n_lat), int(n_lon)
    ch, di, ut = _i32(channel), _i32(direction), _i32(use_threshold)
    rl, gl, sl = _i32(r_lat), _i32(ring_lat), _i32(strike_lat)
    th, de = _f32(threshold), _f64(depth)
    for name, a in (("channel", ch), ("direction", di), ("use_threshold", ut), ("threshold", th), ("r_lat", rl), ("ring_lat", gl),
                    ("depth", de), ("strike_lat", sl)):
      if a.shape != (D,):
        raise ValueError(f"{name} must have shape ({D},), got {a.shape}")
    if np.any((ch < 0) | (ch >= int(c_src))):
      raise ValueError(f"a source channel lies outside [0, {int(c_src)})")
    if np.any(di == 0):
      raise ValueError("direction must be < 0 (a minimum) or > 0 (a maximum)")
    if not np.all(np.isfinite(th[ut != 0])):
      raise ValueError("a threshold in use must be finite")
    if np.any(rl < 0) or np.any(gl < 0) or np.any(sl < 0):
      raise ValueError("r_lat, ring_lat and strike_lat must be >= 0")
    if not np.all(np.isfinite(de[gl > 0])):
      raise ValueError("the depth of a ring in use must be finite")
    lons = []
    for name, a in (("r_lon", r_lon), ("ring_lon", ring_lon), ("strike_lon", strike_lon)):
      a = _i32(a)
      if a.shape != (D, n_lat):
        raise ValueError(f"{name} must have shape ({D}, {n_lat}), got {a.shape}")
      _check_r_lon(a, n_lon, name)
      lons.append(a)
    if isinstance(max_centres, bool) or int(max_centres) != max_centres or not 1 <= int(max_centres) <= 1024:
      raise ValueError(f"max_centres must be an integer in 1 .. 1024, got {max_centres!r}")
    self._check(self._lib.gc_ens_feature_set(self._h, int(c_src), D, _ptr(ch, _i32p), _ptr(di, _i32p), _ptr(ut, _i32p), _ptr(th, _f32p),
                                             n_lat, n_lon, _ptr(rl, _i32p), _ptr(lons[0], _i32p), _ptr(gl, _i32p), _ptr(lons[1], _i32p),
                                             _ptr(de, _f64p), _ptr(sl, _i32p), _ptr(lons[2], _i32p), int(max_centres)))
    self._feature_c_src, self._feature_max, self._feature_members = int(c_src), int(max_centres), -1

  def ens_feature(self, src: "NativeDenoiser", truth=None) -> None:
    """Every slot of this handle's member store <- the strike fields of the centres found in the member of `src`'s store,
    this handle's truth <- those of the truth of `src` (gc_ens_feature): afterwards every scorer of THIS handle sees the
    0 / 1 fields (truth None) and `ens_feature_centres` returns the lists.  `truth` [G, B, c_src] is uploaded into `src`, or
    None = the truth `src` holds."""
    _need(self._feature_c_src, "plan", "ens_feature_set")
    self._check_src(src)
    t = self._truth_arg(truth, self._feature_c_src)
    self._check(self._lib.gc_ens_feature(self._h, _handle_of(src), _opt(t, _f32p)))
    self._feature_members = self._ens_members

  def ens_feature_centres(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (count [M + 1, B, D] int32, node [M + 1, B, D, max_centres] int32, value [M + 1, B, D, max_centres] float32) of the
    last `ens_feature` (gc_ens_feature_centres): field M is the truth; `count` is the true number of centres, of which the
    first min(count, max_centres) in ascending node index are listed (`value`: the source value, the same bits); the entries
    behind them read node -1, value 0."""
    _need(self._feature_members >= 0, "centre lists", why="ens_feature has not run since ens_feature_set")
    shape = (self._feature_members + 1, self.cfg.batch, self.cfg.c_out)
    count = np.empty(shape, np.int32)
    node = np.empty(shape + (self._feature_max,), np.int32)
    value = np.empty(shape + (self._feature_max,), np.float32)
    self._check(self._lib.gc_ens_feature_centres(self._h, _ptr(count, _i32p), _ptr(node, _i32p), _ptr(value, _f32p)))
    return count, node, value

  # -- ensemble order statistics (members sorted on the device) ----------------------------------------
  def ens_order_set(self, probs) -> None:
    """`probs` [Q] in [0, 1], Q in 0..8: the quantile fields `ens_order_score` / `ens_order_fields` leave on the device
    (gc_ens_order_set; needs `set_graph` only and survives `ens_reserve`).  Q = 0: the bin sums only."""
    p = _f64([] if probs is None else probs)
    if p.ndim != 1 or p.shape[0] > 8:
      raise ValueError(f"probs must be a sequence of at most 8 probabilities, got shape {p.shape}")
    if not np.all((p >= 0.0) & (p <= 1.0)):                # (NaN fails both comparisons)
      raise ValueError("probs must lie in [0, 1]")
    self._check(self._lib.gc_ens_order_set(self._h, p.shape[0], _ptr(p, _f64p) if p.shape[0] else None))
    self._order_quantiles = int(p.shape[0])

  def _order_need_set(self) -> int:
    _need(self._order_quantiles is not None, "probabilities", "ens_order_set")
    self._need_store()
    return self._order_quantiles

  def ens_order_score(self, truth=None):
    """-> (bins [B, c_out, M + 1, 2], extra [B, c_out, 3], pinball [B, c_out, Q] float64, counts [B, c_out, Q + 1] uint64,
    invalid int): the raw, additive sums of gc_ens_order_score over the member store (`verification.OrderScores` derives
    the scores); the Q quantile fields stay on the device (`ens_order_quantile`).  `truth` [G, B, c_out], or None = the
    truth uploaded last (shared with `ens_score`)."""
    Q = self._order_need_set()
    t = self._truth_arg(truth)
    B, C, M = self.cfg.batch, self.cfg.c_out, self._ens_members
    bins = np.empty((B, C, M + 1, 2), dtype=np.float64)
    extra = np.empty((B, C, 3), dtype=np.float64)
    pinball = np.empty((B, C, Q), dtype=np.float64)
    counts = np.empty((B, C, Q + 1), dtype=np.uint64)
    invalid = np.zeros(1, dtype=np.uint64)
    self._check(self._lib.gc_ens_order_score(self._h, _opt(t, _f32p), _ptr(bins, _f64p), _ptr(extra, _f64p),
                                             _ptr(pinball, _f64p) if Q else None, _ptr(counts, _u64p), _ptr(invalid, _u64p)))
    return bins, extra, pinball, counts, int(invalid[0])

  def ens_order_fields(self) -> None:
    """The quantile fields of the member store, without truth and without weights (gc_ens_order_fields)."""
    self._order_need_set()
    self._check(self._lib.gc_ens_order_fields(self._h))

  def ens_order_quantile(self, q: int) -> np.ndarray:
    """Quantile field `q` [G, B, c_out] of the last `ens_order_score` / `ens_order_fields` (gc_ens_order_download)."""
    _need(self._order_quantiles is not None, "probabilities", "ens_order_set")
    return self._download(self._lib.gc_ens_order_download, int(q))

  # -- an ensemble against a climatology (two member stores, one pass) -----------------------------------
  def ens_clim_score(self, clim: "NativeDenoiser", truth=None):
    """-> (sums [B, c_out, 12] float64, counts [B, c_out] uint64, invalid int): the raw, additive sums of
    gc_ens_clim_score over this handle's member store and the K climatological samples in the store of `clim`, another
    handle with the same graph, batch and c_out (`Denoiser.climatology_handle`; filled with `ens_reserve(K)` and
    `ens_push_host`).  `verification.ClimatologyScores` derives ACC, CRPSS and the rest.  `truth` [G, B, c_out], or None =
    the truth uploaded last (shared with `ens_score`)."""
    self._check_clim(clim)
    self._need_store()
    t = self._truth_arg(truth)
    B, C = self.cfg.batch, self.cfg.c_out
    sums = np.empty((B, C, 12), dtype=np.float64)
    counts = np.empty((B, C), dtype=np.uint64)
    invalid = np.zeros(1, dtype=np.uint64)
    self._check(self._lib.gc_ens_clim_score(self._h, _handle_of(clim), _opt(t, _f32p), _ptr(sums, _f64p), _ptr(counts, _u64p),
                                            _ptr(invalid, _u64p)))
    return sums, counts, int(invalid[0])

  # -- extreme forecast index (the members ranked in the samples of a climatology handle) ----------------
  def ens_efi_set(self, ranks=(), directions=(), n_bins: int = 20, node_weight_q=None) -> None:
    """The events and bins of `ens_efi_score` (gc_ens_efi_set; needs `set_graph` only and survives `ens_reserve`): `ranks` [T]
    int and `directions` [T] (> 0: the truth's event is lt(y) >= rank, < 0: le(y) <= rank), T in 0..4; `n_bins` E in 2..32
    equal EFI bins; `node_weight_q` [G] uint32 (`verification.quantize_node_weights`), not needed when T == 0.
    `verification.EfiSpec` builds the ranks from quantiles."""
    r = _i32(ranks).reshape(-1)
    T = int(r.shape[0])
    d = _directions(_i32(directions).reshape(-1), T)
    if isinstance(n_bins, bool) or int(n_bins) != n_bins:
      raise ValueError(f"n_bins must be an integer in 2..32, got {n_bins!r}")
    w = self._weights_q_arg(node_weight_q) if T else None
    self._check(self._lib.gc_ens_efi_set(self._h, T, _ptr(r, _i32p) if T else None, _ptr(d, _i32p) if T else None, int(n_bins),
                                         _opt(w, _u32p)))
    self._efi_plan = (T, int(n_bins))

  def _efi_args(self, clim, table):
    """-> `table` as float64 [K + 1] for the K samples in the store of `clim`, after the guards the two EFI calls share."""
    self._check_clim(clim)
    self._need_store()
    K = clim._ens_members  # pylint: disable=protected-access
    _need(K, "member store on the climatology handle", why="ens_reserve has not been called on that object")
    a = _f64(table)
    if a.shape != (K + 1,):
      raise ValueError(f"table must have shape ({K + 1},) for the {K} samples of the climatology handle, got {a.shape}")
    return a

  def ens_efi_score(self, clim: "NativeDenoiser", table, truth=None):
    """-> (sums [B, c_out, 6] float64, weighted [T, B, c_out, 2, E] uint64, counts (same shape), invalid int): the raw,
    additive results of gc_ens_efi_score over this handle's member store and the K samples in the store of `clim`
    (`Denoiser.climatology_handle`); `table` [K + 1] float64 is `verification.efi_table(K)`.  The EFI and the observed index
    stay on the device (`ens_efi_field`).  `truth` [G, B, c_out], or None = the truth uploaded last."""
    a = self._efi_args(clim, table)
    _need(self._efi_plan is not None, "events and bins", "ens_efi_set")
    t = self._truth_arg(truth)
    (T, E), B, C = self._efi_plan, self.cfg.batch, self.cfg.c_out
    sums = np.empty((B, C, 6), dtype=np.float64)
    weighted = np.zeros((T, B, C, 2, E), dtype=np.uint64)
    counts = np.zeros_like(weighted)
    invalid = np.zeros(1, dtype=np.uint64)
    self._check(self._lib.gc_ens_efi_score(self._h, _handle_of(clim), _ptr(a, _f64p), _opt(t, _f32p), _ptr(sums, _f64p),
                                           _ptr(weighted, _u64p) if T else None, _ptr(counts, _u64p) if T else None,
                                           _ptr(invalid, _u64p)))
    return sums, weighted, counts, int(invalid[0])

  def ens_efi_fields(self, clim: "NativeDenoiser", table) -> None:
    """The EFI field of the member store against the samples of `clim`, without truth, weights or events
    (gc_ens_efi_fields); `ens_efi_field(0)` downloads it."""
    a = self._efi_args(clim, table)
    self._check(self._lib.gc_ens_efi_fields(self._h, _handle_of(clim), _ptr(a, _f64p)))

  def ens_efi_field(self, which: int = 0) -> np.ndarray:
    """Field `which` [G, B, c_out] float32 of the last `ens_efi_score` / `ens_efi_fields`: 0 the EFI, 1 the observed index
    (gc_ens_efi_download; the observed index only after `ens_efi_score`)."""
    return self._download(self._lib.gc_ens_efi_download, int(which))

  # -- multivariate ensemble scores (energy over channel groups, variogram over grid offsets) -----------
  def ens_energy_set(self, n_groups: int, group, scale) -> None:
    """The plan of `ens_energy_score` (gc_ens_energy_set; needs `set_graph` only and survives `ens_reserve`): `group` [c_out]
    int, the group 0 .. n_groups - 1 of every channel or -1 for none; `scale` [c_out] float64, a[c] > 0 of the grouped
    channels.  `verification.EnergySpec` builds these arguments."""
    K = int(n_groups)
    g, a = _i32(group), _f64(scale)
    C = self.cfg.c_out
    if g.shape != (C,) or a.shape != (C,):
      raise ValueError(f"group and scale must be [{C}], got {g.shape} and {a.shape}")
    if not 1 <= K <= 32:
      raise ValueError("n_groups must be in 1..32")
    if g.min() < -1 or g.max() >= K or set(range(K)) - set(g.tolist()):
      raise ValueError("group must map every channel to -1 or 0 .. n_groups - 1 and leave no group empty")
    if not np.all(np.isfinite(a[g >= 0]) & (a[g >= 0] > 0.0)):
      raise ValueError("scale must be finite and > 0 for grouped channels")
    self._check(self._lib.gc_ens_energy_set(self._h, K, _ptr(g, _i32p), _ptr(a, _f64p)))
    self._energy_groups = K

  def ens_energy_score(self, truth=None):
    """-> (d2 [B, K, P] float64, s0 [B, K] float64, invalid int): the raw sums of gc_ens_energy_score over the member store,
    P = M (M + 1) / 2 pairs (i < j, index j (j - 1) / 2 + i, slot M the truth); `verification.EnergyScores` derives the
    scores.  `truth` [G, B, c_out], or None = the truth uploaded last (shared with `ens_score`)."""
    _need(self._energy_groups is not None, "plan", "ens_energy_set")
    self._need_store()
    t = self._truth_arg(truth)
    B, K, M = self.cfg.batch, self._energy_groups, self._ens_members
    d2 = np.empty((B, K, M * (M + 1) // 2), dtype=np.float64)
    s0 = np.empty((B, K), dtype=np.float64)
    invalid = np.zeros(1, dtype=np.uint64)
    self._check(self._lib.gc_ens_energy_score(self._h, _opt(t, _f32p), _ptr(d2, _f64p), _ptr(s0, _f64p), _ptr(invalid, _u64p)))
    return d2, s0, int(invalid[0])

  def ens_variogram_set(self, n_lat: int, n_lon: int, offsets, p: float) -> None:
    """The plan of `ens_variogram_score` (gc_ens_variogram_set; needs `set_graph` only and survives `ens_reserve`): the grid
    `n_lat` x `n_lon` (node = i n_lon + j), `offsets` [O, 2] int (di, dj), O in 1..16, and the order `p` in {0.5, 1, 2}."""
    o = _i32(offsets)
    if o.ndim != 2 or o.shape[1] != 2 or not 1 <= o.shape[0] <= 16:
      raise ValueError(f"offsets must be [O, 2] with O in 1..16, got {o.shape}")
    if float(p) not in (0.5, 1.0, 2.0):
      raise ValueError("p must be 0.5, 1 or 2")
    n_lat, n_lon = int(n_lat), int(n_lon)
    if n_lat * n_lon != self.num_grid_nodes:
      raise ValueError(f"n_lat * n_lon must be the number of grid nodes {self.num_grid_nodes}")
    if np.any((o == 0).all(axis=1)) or np.any(np.abs(o[:, 0]) >= n_lat) or np.any(np.abs(o[:, 1]) >= n_lon):
      raise ValueError("an offset is (0, 0) or reaches beyond the grid")
    self._check(self._lib.gc_ens_variogram_set(self._h, n_lat, n_lon, o.shape[0], _ptr(o, _i32p), float(p)))
    self._variogram_offsets = int(o.shape[0])

  def ens_variogram_score(self, truth=None):
    """-> (sums [4, B, c_out, O] float64: V0 .. V3, counts [B, c_out, O] uint64): the raw, additive sums of
    gc_ens_variogram_score over the member store; `verification.VariogramScores` derives the scores.  `truth` [G, B, c_out],
    or None = the truth uploaded last (shared with `ens_score`)."""
    _need(self._variogram_offsets is not None, "plan", "ens_variogram_set")
    self._need_store()
    t = self._truth_arg(truth)
    B, C, O = self.cfg.batch, self.cfg.c_out, self._variogram_offsets
    sums = np.empty((4, B, C, O), dtype=np.float64)
    counts = np.empty((B, C, O), dtype=np.uint64)
    self._check(self._lib.gc_ens_variogram_score(self._h, _opt(t, _f32p), _ptr(sums, _f64p), _ptr(counts, _u64p)))
    return sums, counts

  # -- score maps (the marginal scores per grid point, added up over dates on the device) ----------------
  def ens_map_set(self, channels=None, n_slots: int = 1, n_event_thresholds: int = 0) -> None:
    """The plan of the score maps (gc_ens_map_set; needs `set_graph` only, survives `ens_reserve`): `channels` [C'] ascending and
    distinct (None = all c_out), `n_slots` in 1..128 (a slot is a lead time), `n_event_thresholds` in 0..8 (0: no event
    planes).  Allocates and zeroes the accumulators; a repeated call replaces and zeroes them."""
    ch = None if channels is None else _i32(channels)
    if ch is not None and (ch.ndim != 1 or ch.size < 1):
      raise ValueError("channels must be a non-empty list of channel indices (or None for all)")
    n = self.cfg.c_out if ch is None else int(ch.size)
    self._check(self._lib.gc_ens_map_set(self._h, n, _opt(ch, _i32p), int(n_slots), int(n_event_thresholds)))
    self._map_plan = (n, int(n_slots), int(n_event_thresholds))

  def ens_map_accumulate(self, slot: int, truth=None) -> None:
    """Adds the date in the member store into the planes of `slot` (gc_ens_map_accumulate).  `truth` [G, B, c_out], or None =
    the truth uploaded last (shared with `ens_score`)."""
    t = self._truth_arg(truth)
    self._check(self._lib.gc_ens_map_accumulate(self._h, int(slot), _opt(t, _f32p)))

  def ens_map_accumulate_events(self, slot: int) -> None:
    """Adds the codes of the last `ens_event_score` into the event planes of `slot` (gc_ens_map_accumulate_events)."""
    self._check(self._lib.gc_ens_map_accumulate_events(self._h, int(slot)))

  def ens_map_download(self, slot: int, events: bool = None):
    """-> (sums [6, G, B, C'] float64, counts [3, G, B, C'] uint32, events [T, 5, G, B, C'] uint32 or None, dates [2] int64: field
    and event calls added): the planes of `slot` (gc_ens_map_download; `verification.ScoreMaps` / `EventMaps` derive the
    scores).  `events`: None = where the plan has event planes."""
    if self._map_plan is None:                   # the library says what is missing, in its order
      self._check(self._lib.gc_ens_map_download(self._h, int(slot), None, None, None, None))
      _need(False, "map plan", "ens_map_set")
    (C, _, T), G, B = self._map_plan, self.num_grid_nodes, self.cfg.batch
    want = T > 0 if events is None else bool(events)
    sums = np.empty((6, G, B, C), dtype=np.float64)
    counts = np.empty((3, G, B, C), dtype=np.uint32)
    ev = np.empty((T, 5, G, B, C), dtype=np.uint32) if want else None
    dates = np.zeros(2, dtype=np.int64)
    self._check(self._lib.gc_ens_map_download(self._h, int(slot), _ptr(sums, _f64p), _ptr(counts, _u32p), _opt(ev, _u32p),
                                              _ptr(dates, _i64p)))
    return sums, counts, ev, dates

  def ens_map_reset(self, slot: int = -1) -> None:
    """Zeroes the planes of `slot` (-1: of every slot) and forgets its M and its dates (gc_ens_map_reset)."""
    self._check(self._lib.gc_ens_map_reset(self._h, int(slot)))

  # -- threshold-weighted CRPS (one sort of the members per point, T thresholds) -------------------------
  def ens_tail_set(self, thresholds, directions) -> None:
    """`thresholds` [T, G, B, c_out] float32 (T in 1..8; NaN = not evaluated there), `directions` [T] (> 0: the upper tail,
    weight 1{z >= threshold}; < 0: the lower tail, 1{z <= threshold}): gc_ens_tail_set; needs `set_graph` only, survives
    `ens_reserve` and is independent of `ens_event_set`."""
    thr = self._thresholds_arg(thresholds)
    if not 1 <= thr.shape[0] <= 8:
      raise ValueError(f"thresholds must hold 1..8 fields, got {thr.shape[0]}")
    d = _directions(directions, thr.shape[0])
    if np.any(d == 0):
      raise ValueError("directions must be non-zero")
    self._check(self._lib.gc_ens_tail_set(self._h, thr.shape[0], _ptr(thr, _f32p), _ptr(d, _i32p)))
    self._tail_thresholds = int(thr.shape[0])

  def ens_tail_score(self, truth=None):
    """-> (sums [T, B, c_out, 4] float64: sum w, sum w ae, sum w d, sum w o; counts [T, B, c_out] uint64; invalid [T] uint64):
    the raw, additive sums of gc_ens_tail_score over the member store (`verification.TailScores` derives the scores).
    `truth` [G, B, c_out], or None = the truth uploaded last (shared with `ens_score`)."""
    _need(self._tail_thresholds, "thresholds", "ens_tail_set")
    self._need_store()
    t = self._truth_arg(truth)
    T, B, C = self._tail_thresholds, self.cfg.batch, self.cfg.c_out
    sums = np.empty((T, B, C, 4), dtype=np.float64)
    counts = np.empty((T, B, C), dtype=np.uint64)
    invalid = np.empty(T, dtype=np.uint64)
    self._check(self._lib.gc_ens_tail_score(self._h, _opt(t, _f32p), _ptr(sums, _f64p), _ptr(counts, _u64p), _ptr(invalid, _u64p)))
    return sums, counts, invalid

  # -- regional ensemble scores (the sums of ens_score per region of grid nodes, from one pass) ---------
  def ens_region_set(self, node_bits, n_regions: int) -> None:
    """`node_bits` [G] uint32, bit r set = grid node g belongs to region r < `n_regions` (1..32); regions may overlap, a node
    with no bit is never read: gc_ens_region_set; needs `set_graph` only and survives `ens_reserve`.  At most 256 distinct
    non-zero values.  `verification.RegionSpec.node_bits` builds the argument."""
    R = int(n_regions)
    if not 1 <= R <= 32:
      raise ValueError(f"n_regions must be in 1..32, got {R}")
    raw = np.asarray(node_bits)
    if raw.shape != (self.num_grid_nodes,):
      raise ValueError(f"node_bits must have shape ({self.num_grid_nodes},), got {raw.shape}")
    if raw.dtype.kind not in "ui" or (raw.size and (int(raw.min()) < 0 or int(raw.max()) >> R)):
      raise ValueError(f"node_bits must be unsigned integers below 2^{R}")
    bits = np.ascontiguousarray(raw, dtype=np.uint32)
    self._check(self._lib.gc_ens_region_set(self._h, R, _ptr(bits, _u32p)))
    self._regions = R

  def ens_region_score(self, truth=None):
    """-> (sums [R, B, c_out, 6] float64, hist [R, B, c_out, M + 1] uint64, invalid [R] uint64): per region the raw, additive
    sums, rank histogram and skipped points of `ens_score` restricted to the region's nodes (gc_ens_region_score;
    `verification.RegionScores` derives the scores).  `truth` [G, B, c_out], or None = the truth uploaded last."""
    _need(self._regions, "regions", "ens_region_set")
    self._need_store()
    t = self._truth_arg(truth)
    R, B, C = self._regions, self.cfg.batch, self.cfg.c_out
    sums = np.empty((R, 6, B, C), dtype=np.float64)
    hist = np.empty((R, B, C, self._ens_members + 1), dtype=np.uint64)
    invalid = np.empty(R, dtype=np.uint64)
    self._check(self._lib.gc_ens_region_score(self._h, _opt(t, _f32p), _ptr(sums, _f64p), _ptr(hist, _u64p), _ptr(invalid, _u64p)))
    return np.ascontiguousarray(np.moveaxis(sums, 1, -1)), hist, invalid

  # -- time-window ensemble fields (a ring of the last lead times, reduced into this handle's member store) --
  def ens_window_set(self, kind: int, length: int, coef=None) -> None:
    """The plan of `ens_window_emit` (gc_ens_window_set; needs `set_graph` only): `kind` 0 linear, 1 max, 2 min over the last
    `length` (1..64) pushes; `coef` [length] float64, oldest push first, for a linear window (sum: ones; mean: 1 / length;
    change: -1, 0, .., 0, +1) and None otherwise.  A new plan clears the push count.  `verification.WindowSpec` builds these
    arguments."""
    kind, length = int(kind), int(length)
    if kind not in (0, 1, 2):
      raise ValueError("kind must be 0 (linear), 1 (max) or 2 (min)")
    if not 1 <= length <= 64:
      raise ValueError("length must lie in 1 .. 64")
    a = None
    if kind == 0:
      if coef is None:
        raise ValueError("a linear window needs its coefficients")
      a = _f64(coef)
      if a.shape != (length,):
        raise ValueError(f"coef must have shape ({length},)")
      if not np.all(np.isfinite(a)):
        raise ValueError("coef must be finite")
    elif coef is not None:
      raise ValueError("only a linear window takes coefficients")
    self._check(self._lib.gc_ens_window_set(self._h, kind, length, _opt(a, _f64p)))
    self._window_length = length

  def ens_window_push(self, src: "NativeDenoiser", truth=None) -> None:
    """The ring of this handle <- the M members and the truth of `src`'s store as they stand, device to device
    (gc_ens_window_push).  `truth` [G, B, c_out] is uploaded into `src`, or None = the truth `src` holds.  On return `src`'s
    store may be overwritten."""
    _need(self._window_length, "plan", "ens_window_set")
    self._check_src(src)
    t = self._truth_arg(truth)
    self._check(self._lib.gc_ens_window_push(self._h, _handle_of(src), _opt(t, _f32p)))

  def ens_window_emit(self) -> None:
    """Every slot of this handle's member store and its truth <- the window over the last `length` pushes
    (gc_ens_window_emit): afterwards `ens_score(None)`, `ens_event_score(None)`, `ens_order_score(None)` and
    `ens_download_member` of THIS handle see the windowed fields.  The ring is unchanged."""
    _need(self._window_length, "plan", "ens_window_set")
    self._check(self._lib.gc_ens_window_emit(self._h))

  def ens_window_reset(self) -> None:
    """Forgets the pushes; the plan and the ring's memory stay (gc_ens_window_reset)."""
    self._check(self._lib.gc_ens_window_reset(self._h))

  # -- context store: one resident conditioning per ensemble member ----------------------------------
  def ctx_reserve(self, n: int) -> None:
    """A store of `n` (1..64) conditioning arrays on the handle; empties an earlier one (gc_ctx_reserve)."""
    self._check(self._lib.gc_ctx_reserve(self._h, int(n)))

  def ctx_save(self, slot: int, src: Optional["NativeDenoiser"] = None) -> None:
    """Slot <- the current conditioning of `src` (None: of this handle), device to device (gc_ctx_save)."""
    self._check(self._lib.gc_ctx_save(self._h, int(slot), _handle_of(src)))

  def ctx_load(self, slot: int, dst: Optional["NativeDenoiser"] = None) -> None:
    """The conditioning of `dst` (None: of this handle) <- slot, re-packed like `upload_cond_dev` (gc_ctx_load)."""
    self._check(self._lib.gc_ctx_load(self._h, int(slot), _handle_of(dst)))

  def ctx_download(self, slot: int) -> np.ndarray:
    return self._download(self._lib.gc_ctx_download, int(slot), shape=self._shape_in())

  # -- spherical-harmonic power spectra (analysed on the device) -------------------------------------
  def spec_set_tables(self, legendre_analysis, cos_a, sin_a) -> None:
    """`spectra.SphericalAnalysis.device_tables()`: legendre_analysis [lmax, lmax, n_lat], cos_a / sin_a [lmax, n_lon]
    (gc_spec_set_tables; needs `set_graph` only)."""
    q, c, s = _f32(legendre_analysis), _f32(cos_a), _f32(sin_a)
    if q.ndim != 3 or q.shape[0] != q.shape[1] or c.ndim != 2 or c.shape != s.shape or c.shape[0] != q.shape[0]:
      raise ValueError(f"tables must be [lmax, lmax, n_lat], [lmax, n_lon], [lmax, n_lon]; got {q.shape}, {c.shape}, {s.shape}")
    self._check(self._lib.gc_spec_set_tables(self._h, q.shape[2], c.shape[1], q.shape[0], _ptr(q, _f32p), _ptr(c, _f32p),
                                             _ptr(s, _f32p)))
    self._spec_lmax = int(q.shape[0])
    self._band_c_src = 0                       # (a band plan goes with the tables it was made for)

  def spec_field(self, field=None) -> np.ndarray:
    """-> power [B, c_out, lmax] float64 of `field` [G, B, c_out], or of the last resident sample (None): gc_spec_field."""
    _need(self._spec_lmax, "analysis tables", "spec_set_tables")
    x = None
    if field is not None:
      x = _f32(field)
      if x.shape != self._shape_out():
        raise ValueError(f"field must be {self._shape_out()}, got {x.shape}")
    power = np.empty((self.cfg.batch, self.cfg.c_out, self._spec_lmax), dtype=np.float64)
    self._check(self._lib.gc_spec_field(self._h, _opt(x, _f32p), _ptr(power, _f64p)))
    return power

  def ens_spectrum(self, truth=None, want_member_power: bool = False):
    """-> sums [B, c_out, lmax, 6] float64, the raw additive sums of gc_ens_spectrum over the member store
    (`spectra.EnsembleSpectra` derives the rest); with `want_member_power` also [M, B, c_out, lmax].
    `truth` [G, B, c_out], or None = the truth uploaded last (shared with `ens_score`)."""
    _need(self._spec_lmax, "analysis tables", "spec_set_tables")
    self._need_store()
    t = self._truth_arg(truth)
    B, C, L = self.cfg.batch, self.cfg.c_out, self._spec_lmax
    sums = np.empty((6, B, C, L), dtype=np.float64)
    mp = np.empty((self._ens_members, B, C, L), dtype=np.float64) if want_member_power else None
    self._check(self._lib.gc_ens_spectrum(self._h, _opt(t, _f32p), _ptr(sums, _f64p), _opt(mp, _f64p)))
    sums = np.ascontiguousarray(np.moveaxis(sums, 0, -1))
    return (sums, mp) if want_member_power else sums

  # -- ensemble exchange (RCCL inside the library) -------------------------------------------------
  def comm_init(self, unique_id: bytes, rank: int, world_size: int) -> None:
    if len(unique_id) != COMM_ID_BYTES:
      raise ValueError(f"unique id must be {COMM_ID_BYTES} bytes")
    buf = ctypes.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
    self._check(self._lib.gc_comm_init(self._h, buf, int(rank), int(world_size)))

  def comm_info(self):
    """(ranks, rank) as RCCL reports them for this handle's communicator; (0, -1) without one (gc_comm_info)."""
    n, r = ctypes.c_int32(), ctypes.c_int32()
    self._check(self._lib.gc_comm_info(self._h, ctypes.byref(n), ctypes.byref(r)))
    return n.value, r.value

  def comm_broadcast_cond(self, root: int = 0) -> None:
    self._check(self._lib.gc_comm_broadcast_cond(self._h, int(root)))

  def comm_allreduce_max(self, value: float) -> float:
    v = ctypes.c_double(float(value))
    self._check(self._lib.gc_comm_allreduce_max(self._h, ctypes.byref(v)))
    return v.value

  def comm_destroy(self) -> None:
    self._check(self._lib.gc_comm_destroy(self._h))

  def counter(self, name: str) -> int:
    """Named counters: range_fallbacks, launches_per_call, weights_f16_unsafe, loss_evaluations, ... (gc_get_counter);
    poison_allocs and poison_bytes: the device buffers GC_DEBUG_POISON=1 has filled on this handle (0 without it)."""
    v = ctypes.c_int64()
    self._check(self._lib.gc_get_counter(self._h, name.encode(), ctypes.byref(v)))
    return v.value

  # -- debug (tests) -------------------------------------------------------------------------------
  def debug_fetch(self, name: str) -> np.ndarray:
    r, c = ctypes.c_int64(), ctypes.c_int64()
    self._check(self._lib.gc_debug_fetch(self._h, name.encode(), None, 0, ctypes.byref(r),
                                         ctypes.byref(c)))
    out = np.empty((r.value, c.value), dtype=np.float32)
    self._check(self._lib.gc_debug_fetch(self._h, name.encode(), _ptr(out, _f32p), out.size,
                                         ctypes.byref(r), ctypes.byref(c)))
    return out

  def debug_set_layer_limit(self, n: int):
    self._check(self._lib.gc_debug_set_layer_limit(self._h, n))

  def debug_set_stop(self, layer: int, phase: int = 0):
    """Later forwards return inside block `layer` after phase 0 / 1 / 2 (gc_debug_set_stop); layer -1 = off."""
    self._check(self._lib.gc_debug_set_stop(self._h, int(layer), int(phase)))

  def debug_mesh_permutation(self) -> np.ndarray:
    p = np.empty(self.num_mesh_nodes, dtype=np.int32)
    self._check(self._lib.gc_debug_mesh_permutation(self._h, _ptr(p, _i32p)))
    return p

  def debug_attention_stats(self):
    a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    self._check(self._lib.gc_debug_attention_stats(self._h, ctypes.byref(a), ctypes.byref(b),
                                                   ctypes.byref(c)))
    return dict(n_tiles=a.value, n_chunks=b.value, khop_nnz=c.value)


def comm_unique_id() -> bytes:
  """rank 0: the ncclUniqueId blob every rank passes to `NativeDenoiser.comm_init`."""
  lib = load_library()
  buf = ctypes.create_string_buffer(COMM_ID_BYTES)
  rc = lib.gc_comm_unique_id(buf)
  if rc != GC_OK:
    raise GencastHipError(f"gc_comm_unique_id failed ({rc}): {lib.gc_last_error(None).decode()}")
  return buf.raw


def device_count() -> int:
  return int(load_library().gc_device_count())


def device_pci_bus_id(device_id: int) -> str:
  """PCI bus id of a visible device: what the ranks of a launch compare to see whether two of them share a GPU."""
  buf = ctypes.create_string_buffer(64)
  rc = load_library().gc_device_pci_bus_id(int(device_id), buf, 64)
  if rc != 0:
    raise GencastHipError(f"gc_device_pci_bus_id({device_id}) failed with code {rc}")
  return buf.value.decode()
