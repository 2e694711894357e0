"""The definition of the derived and pooled ensemble fields (include/gencast_hip.h, gc_ens_derive_*),
restated in NumPy float64.  Test infrastructure: the product never imports it.

A field is [G, ...] float32 with G = n_lat n_lon, node = lat_i n_lon + lon_j; the trailing axes (batch, channel, and for a
stack of fields the member) are independent columns.  `pool_direct` is the definition literally: for every (i, j) the
window Win(i, j) is written out point by point, no separability.  `pool_separable` restates it as a row pass and a column
pass, the form the device takes.

The sums of MEAN are accumulated in np.longdouble (64 mantissa bits on x86) and the quotient is rounded to float64 once:
the yardstick then carries no summation error of its own worth speaking of, and the two restatements, which add the same
terms in different orders, agree to a few 2^-53 relative instead of to sqrt(window) 2^-53."""
import numpy as np

COPY, NORM2 = 0, 1
NONE, MAX, MIN, MEAN = 0, 1, 2, 3
WIDE = np.longdouble


def derive(x, op, src_a, src_b, affine):
  """x [..., c_src] float32 -> d [..., c_d] float32: COPY keeps the bits, NORM2 is sqrt(u u + v v) in double, rounded once."""
  x = np.asarray(x, np.float32)
  out = np.empty(x.shape[:-1] + (len(op),), np.float32)
  for j in range(len(op)):
    if op[j] == COPY:
      out[..., j] = x[..., src_a[j]]
    elif op[j] == NORM2:
      sa, la, sb, lb = (np.float64(v) for v in affine[j])
      with np.errstate(invalid="ignore", over="ignore"):
        u = x[..., src_a[j]].astype(np.float64) * sa + la
        v = x[..., src_b[j]].astype(np.float64) * sb + lb
        out[..., j] = np.sqrt(u * u + v * v).astype(np.float32)
    else:
      raise ValueError(f"op {op[j]}")
  return out


def window(i, j, n_lat, n_lon, r_lat, r_lon):
  """Win(i, j) as (rows, nodes): the longitude wraps, the latitude is clipped, the width is that of the row i'."""
  rows, nodes = [], []
  for ii in range(max(0, i - r_lat), min(n_lat - 1, i + r_lat) + 1):
    for t in range(-int(r_lon[ii]), int(r_lon[ii]) + 1):
      rows.append(ii)
      nodes.append(ii * n_lon + (j + t) % n_lon)
  return np.asarray(rows), np.asarray(nodes)


def _combine(pool, vals, w):
  """vals [P, ...] float32 (the window points), w [P] float64 -> the pooled value per column: float32 for MAX / MIN,
  float64 (not yet rounded) for MEAN.  Non-finite points are skipped; a window without a finite point gives NaN."""
  fin = np.isfinite(vals)
  if pool == MEAN:
    w = w.reshape((-1,) + (1,) * (vals.ndim - 1))
    num = np.where(fin, w.astype(WIDE) * vals.astype(WIDE), WIDE(0)).sum(axis=0)
    den = np.where(fin, w.astype(WIDE), WIDE(0)).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
      return (num / den).astype(np.float64)
  fill = np.float32(-np.inf if pool == MAX else np.inf)
  ext = np.where(fin, vals, fill)
  ext = ext.max(axis=0) if pool == MAX else ext.min(axis=0)
  return np.where(fin.any(axis=0), ext, np.float32(np.nan)).astype(np.float32)


def pool_direct(d, pool, n_lat, n_lon, r_lat, r_lon, row_weight):
  """d [G, ...] float32 -> out [G, ...]: float32 for NONE / MAX / MIN, float64 for MEAN (round it once to compare).
  NaN iff the centre is not finite."""
  d = np.asarray(d, np.float32)
  if pool == NONE:
    return d.copy()
  out = np.empty(d.shape, np.float64 if pool == MEAN else np.float32)
  rw = np.asarray(row_weight, np.float64)
  for i in range(n_lat):
    for j in range(n_lon):
      rows, nodes = window(i, j, n_lat, n_lon, r_lat, r_lon)
      c = i * n_lon + j
      out[c] = np.where(np.isfinite(d[c]), _combine(pool, d[nodes], rw[rows]), np.nan)
  return out


def pool_separable(d, pool, n_lat, n_lon, r_lat, r_lon, row_weight):
  """The same map as a row pass (each row pooled along its longitude) and a column pass over the row results."""
  d = np.asarray(d, np.float32)
  if pool == NONE:
    return d.copy()
  g = d.reshape((n_lat, n_lon) + d.shape[1:])
  fin = np.isfinite(g)
  rw = np.asarray(row_weight, np.float64)
  if pool == MEAN:
    rsum, rcnt = np.zeros(g.shape, WIDE), np.zeros(g.shape, WIDE)
    for i in range(n_lat):
      for t in range(-int(r_lon[i]), int(r_lon[i]) + 1):
        rsum[i] += np.roll(np.where(fin[i], g[i].astype(WIDE), WIDE(0)), -t, axis=0)
        rcnt[i] += np.roll(fin[i].astype(WIDE), -t, axis=0)
    out = np.empty(g.shape)
    for i in range(n_lat):
      num, den = np.zeros(g.shape[1:], WIDE), np.zeros(g.shape[1:], WIDE)
      for ii in range(max(0, i - r_lat), min(n_lat - 1, i + r_lat) + 1):
        num += WIDE(rw[ii]) * rsum[ii]
        den += WIDE(rw[ii]) * rcnt[ii]
      with np.errstate(invalid="ignore", divide="ignore"):
        out[i] = (num / den).astype(np.float64)
    return np.where(fin, out, np.nan).reshape(d.shape)
  sign = np.float32(1.0 if pool == MAX else -1.0)          # min x = -max(-x), exactly
  x = np.where(fin, sign * g, np.float32(-np.inf))
  rext = np.full(g.shape, -np.inf, np.float32)
  for i in range(n_lat):
    for t in range(-int(r_lon[i]), int(r_lon[i]) + 1):
      rext[i] = np.maximum(rext[i], np.roll(x[i], -t, axis=0))
  out = np.full(g.shape, -np.inf, np.float32)
  for i in range(n_lat):
    for ii in range(max(0, i - r_lat), min(n_lat - 1, i + r_lat) + 1):
      out[i] = np.maximum(out[i], rext[ii])
  return np.where(fin, sign * out, np.float32(np.nan)).astype(np.float32).reshape(d.shape)


def apply(fields, plan, *, separable=False):
  """fields [..., G, B, c_src] (one field, or a stack of members) -> the derived and pooled fields [..., G, B, c_d]: float32
  for NONE / MAX / MIN, the unrounded float64 for MEAN.  `plan`: the keyword arguments of NativeDenoiser.ens_derive_set."""
  x = np.asarray(fields, np.float32)
  d = derive(x, plan["op"], plan["src_a"], plan["src_b"], plan["affine"])
  if plan.get("pool", NONE) == NONE:
    return d
  lead = d.ndim - 3
  dg = np.moveaxis(d, lead, 0)                                # G first: every other axis is a column
  fn = pool_separable if separable else pool_direct
  out = fn(dg, plan["pool"], plan["n_lat"], plan["n_lon"], plan["r_lat"], plan["r_lon"], plan["row_weight"])
  return np.moveaxis(out, 0, lead)


def mean_bound(d, ref64, n_lon):
  """The tolerance of a device MEAN against the float64 reference `ref64` [..., G, B, C] of the float32 field d (same
  shape): one rounding to float32, np.spacing(float32(ref)), plus n_lon^2 2^-52 max|finite d| of the (field, b, c) column --
  a double prefix sum of n_lon terms, differenced."""
  d = np.asarray(d, np.float32)
  top = np.where(np.isfinite(d), np.abs(d.astype(np.float64)), 0.0).max(axis=-3, keepdims=True)
  with np.errstate(invalid="ignore"):
    return np.spacing(np.abs(np.asarray(ref64).astype(np.float32))).astype(np.float64) + float(n_lon) ** 2 * 2.0 ** -52 * top


def data(M, G, B, C, seed):
  """members [M, G, B, C] and truth [G, B, C] float32 with per-channel scales over eight decades, as event_reference.data."""
  rng = np.random.default_rng(seed)
  scale = np.logspace(-3, 5, C)
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  return members, truth
