"""The definition of ensemble feature detection (include/gencast_hip.h, gc_ens_feature_*), restated in
NumPy operation for operation.  Test infrastructure: the product never imports it.

A field is [G, ...] float32 with G = n_lat n_lon, node = lat_i n_lon + lon_j; the trailing axes are independent columns.
Every window is written out node by node (`tests/derive_reference.window`): no keys, no separability, no scatter.  The
definition holds comparisons of float32 values and one float64 subtraction, so a device result equals this one bit for bit.
A `plan` is the keyword arguments of `NativeDenoiser.ens_feature_set`."""
import functools

import numpy as np

from tests import derive_reference as DR


@functools.lru_cache(maxsize=None)
def _windows(n_lat, n_lon, r_lat, r_lon):
  """Per node n, the nodes of window(n; r_lat, r_lon)."""
  return [DR.window(i, j, n_lat, n_lon, r_lat, r_lon)[1] for i in range(n_lat) for j in range(n_lon)]


@functools.lru_cache(maxsize=None)
def _rings(n_lat, n_lon, ring_lat, ring_lon):
  """Per node n = (i, j), the boundary of window(n; ring_lat, ring_lon): the rows i +- ring_lat that exist over all
  |t| <= ring_lon[i'], and in every row strictly between them the two nodes t = +-ring_lon[i']."""
  out = []
  for i in range(n_lat):
    for j in range(n_lon):
      nodes = []
      for ii in range(i - ring_lat, i + ring_lat + 1):
        if not 0 <= ii < n_lat:
          continue
        r = int(ring_lon[ii])
        ts = range(-r, r + 1) if ii in (i - ring_lat, i + ring_lat) else sorted({-r, r})
        nodes += [ii * n_lon + (j + t) % n_lon for t in ts]
      out.append(np.asarray(nodes, np.int64))
  return out


def signed(x, direction):
  """s = x for a minimum (direction < 0), -x for a maximum."""
  x = np.asarray(x, np.float32)
  return x if direction < 0 else -x


def centres(x, plan, d):
  """x [G, K] float32, the source channel of detector d in K columns -> flags [G, K] bool: node n is a centre."""
  n_lat, n_lon = int(plan["n_lat"]), int(plan["n_lon"])
  G = n_lat * n_lon
  s = signed(x, int(plan["direction"][d]))
  fin = np.isfinite(s)
  wins = _windows(n_lat, n_lon, int(plan["r_lat"][d]), tuple(int(v) for v in plan["r_lon"][d]))
  ring_lat = int(plan["ring_lat"][d])
  rings = _rings(n_lat, n_lon, ring_lat, tuple(int(v) for v in plan["ring_lon"][d])) if ring_lat > 0 else None
  t = np.float32(plan["threshold"][d])
  t = t if int(plan["direction"][d]) < 0 else -t
  depth = np.float64(plan["depth"][d])
  out = np.zeros(s.shape, bool)
  with np.errstate(invalid="ignore"):
    for n in range(G):
      other = wins[n][wins[n] != n]
      v = s[other]                                             # [P, K]
      later = (other > n).reshape((-1,) + (1,) * (s.ndim - 1))
      beats = (s[n] < v) | ((s[n] == v) & later)               # IEEE ==: -0.0 == +0.0
      ok = fin[n] & np.all(beats | ~fin[other], axis=0)        # non-finite neighbours are skipped
      if int(plan["use_threshold"][d]):
        ok &= s[n] <= t
      if rings is not None:
        rv, rf = s[rings[n]], fin[rings[n]]
        low = np.where(rf, rv, np.float32(np.inf)).min(axis=0)
        ok &= rf.any(axis=0) & (low.astype(np.float64) - s[n].astype(np.float64) >= depth)
      out[n] = ok
  return out


def strike(flags, finite, plan, d):
  """flags, finite [G, K] bool -> the strike field [G, K] float32: 1 where any centre lies in window(n; strike), else 0;
  NaN where the source value at n is not finite."""
  n_lat, n_lon = int(plan["n_lat"]), int(plan["n_lon"])
  wins = _windows(n_lat, n_lon, int(plan["strike_lat"][d]), tuple(int(v) for v in plan["strike_lon"][d]))
  hit = np.stack([flags[wins[n]].any(axis=0) for n in range(n_lat * n_lon)])
  return np.where(finite, hit.astype(np.float32), np.float32(np.nan)).astype(np.float32)


def apply(fields, plan):
  """fields [..., G, B, c_src] float32 (one field, or a stack: the members, then the truth) ->
  (count [..., B, D] int32, node [..., B, D, max_centres] int32, value [..., B, D, max_centres] float32,
  strike [..., G, B, D] float32).  The lists are in ascending node index; count is the true number, the first max_centres
  are kept, the entries behind them are node -1, value 0; value is the source value x, the same bits."""
  x = np.asarray(fields, np.float32)
  lead = x.ndim - 3
  xg = np.moveaxis(x, lead, 0)                                 # [G, ..., B, c_src]
  D, mc = len(plan["channel"]), int(plan["max_centres"])
  cols = xg.shape[1:-1]
  count = np.zeros(cols + (D,), np.int32)
  node = np.full(cols + (D, mc), -1, np.int32)
  value = np.zeros(cols + (D, mc), np.float32)
  out = np.empty(xg.shape[:-1] + (D,), np.float32)
  for d in range(D):
    xd = np.ascontiguousarray(xg[..., int(plan["channel"][d])])
    flags = centres(xd, plan, d)
    out[..., d] = strike(flags, np.isfinite(xd), plan, d)
    for col in np.ndindex(*cols):
      at = np.flatnonzero(flags[(slice(None),) + col])
      count[col + (d,)] = at.size
      k = min(at.size, mc)
      node[col + (d,)][:k] = at[:k]
      value[col + (d,)][:k] = xd[(at[:k],) + col]
  return count, node, value, np.moveaxis(out, 0, lead)


def plan_of(c_src, n_lat, n_lon, detectors, max_centres=64):
  """A plan from a list of per-detector dicts: channel, direction, threshold (None: not used), r_lat, r_lon, ring_lat
  (0: no ring), ring_lon, depth, strike_lat, strike_lon."""
  zeros = np.zeros(n_lat, np.int32)
  g = lambda k, dflt=None: [det.get(k, dflt) for det in detectors]
  return dict(c_src=c_src, channel=np.asarray(g("channel"), np.int32), direction=np.asarray(g("direction", -1), np.int32),
              use_threshold=np.asarray([det.get("threshold") is not None for det in detectors], np.int32),
              threshold=np.asarray([0.0 if det.get("threshold") is None else det["threshold"] for det in detectors], np.float32),
              n_lat=n_lat, n_lon=n_lon, r_lat=np.asarray(g("r_lat", 0), np.int32),
              r_lon=np.stack([np.asarray(det.get("r_lon", zeros), np.int32) for det in detectors]),
              ring_lat=np.asarray(g("ring_lat", 0), np.int32),
              ring_lon=np.stack([np.asarray(det.get("ring_lon", zeros), np.int32) for det in detectors]),
              depth=np.asarray(g("depth", 0.0), np.float64), strike_lat=np.asarray(g("strike_lat", 0), np.int32),
              strike_lon=np.stack([np.asarray(det.get("strike_lon", zeros), np.int32) for det in detectors]),
              max_centres=max_centres)
