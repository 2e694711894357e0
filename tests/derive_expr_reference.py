"""The definition of the derive ops of gc_ens_derive_set_expr (include/gencast_hip.h) restated in NumPy
float64, literally: the same operations in the same order on the same host tables, rounded to float32 once.  Test
infrastructure: the product never imports it.

A field is [..., G, B, c_src] float32 with G = n_lat n_lon, node = lat_i n_lon + lon_j.  `plan` is the keyword dict of
`NativeDenoiser.ens_derive_set` with the keys of a new-style plan (`DerivedSpec.plan`, or `raw_plan` here).  A source channel
enters in physical units, p(c) = (double) x[c] scale[c] + loc[c].

`derive` returns the float32 result and, beside it, the tolerance of a device result against it, computed from the inputs:

    bound = np.spacing(float32(ref)) + k 2^-52 A

A is the expression evaluated with every entering term replaced by its absolute value and every subtraction by an addition
(the running bound of a floating-point chain), k the count of double operations in the chain:
  SUM         k = T, the terms of the list (one addition each), A = sum_t |coef_t| |p|(a_t) |p|(b_t), |p|(c) = |x scale| + |loc|
  NORM        e_i = T_i 2^-52 A_i per list; through the square root |d sqrt(S1^2 + S2^2)| <= hypot(e_1, e_2) (Cauchy-Schwarz),
              plus K_ROOT = 3 operations (two squares added, one root) on the result itself
  NORM2       K_ROOT on the result: the legacy op, u and v being two operations each from exact inputs
  VORTICITY,  k = K_CURL = 16: four p() of two operations, two differences, two products with cos(lat), three products with
  DIVERGENCE  the row tables, one sum; A = ((|a+| + |a-|) |1/2dl| + (|b+| c+ + |b-| c-) |1/dphi|) |1/(R c)|
  a pole row  k = K_CURL + n_lon (the zonal sum, and the division), A = the mean over j of the adjacent row's A
  COPY        0: the same bits
No free constant."""
import numpy as np

COPY, NORM2, SUM, NORM, VORTICITY, DIVERGENCE = range(6)
EARTH_RADIUS_M = 6371000.0
K_CURL, K_ROOT = 16, 3
EPS = 2.0 ** -52


def row_tables(lat, lon):
  """The host tables of VORTICITY / DIVERGENCE from the coordinates in degrees, as the definition has them."""
  lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
  n = lat.size
  pole = np.abs(lat) >= 90.0 - 1e-9
  phi = np.deg2rad(lat)
  cos = np.cos(phi)
  cos[pole] = 0.0
  inv_rcos = np.zeros(n)
  inv_rcos[~pole] = 1.0 / (EARTH_RADIUS_M * cos[~pole])
  inv_dphi = np.array([1.0 / (phi[min(i + 1, n - 1)] - phi[max(i - 1, 0)]) for i in range(n)])
  return dict(coslat=cos, inv_rcos=inv_rcos, inv_dphi=inv_dphi, inv_2dlam=float(1.0 / (2.0 * np.deg2rad(lon[1] - lon[0]))),
              pole_row=pole.astype(np.int32))


def raw_plan(c_src, channels, n_lat, n_lon, scale=None, loc=None, lat=None, lon=None, **pool):
  """A new-style plan from a list of derived channels, each one of ("copy", a), ("norm2", a, b, (sa, la, sb, lb)),
  ("sum", terms), ("norm", terms_1, terms_2), ("vorticity", u, v), ("divergence", u, v); a term is (coef, a, b or -1)."""
  c_d = len(channels)
  op, a, b = np.zeros(c_d, np.int32), np.zeros(c_d, np.int32), np.zeros(c_d, np.int32)
  affine = np.tile([1.0, 0.0, 1.0, 0.0], (c_d, 1))
  start, coef, ta, tb = np.zeros((c_d, 3), np.int32), [], [], []
  for j, ch in enumerate(channels):
    op[j] = dict(copy=COPY, norm2=NORM2, sum=SUM, norm=NORM, vorticity=VORTICITY, divergence=DIVERGENCE)[ch[0]]
    if ch[0] in ("sum", "norm"):
      start[j, 0] = len(coef)
      for k, terms in enumerate(ch[1:]):
        coef += [t[0] for t in terms]
        ta += [t[1] for t in terms]
        tb += [t[2] for t in terms]
        start[j, k + 1:] = len(coef)
      continue
    a[j] = ch[1]
    if ch[0] != "copy":
      b[j] = ch[2]
    if ch[0] == "norm2":
      affine[j] = ch[3]
  plan = dict(c_src=c_src, op=op, src_a=a, src_b=b, affine=affine, pool=0, n_lat=n_lat, n_lon=n_lon, r_lat=0, r_lon=None,
              row_weight=None, scale=np.ones(c_src) if scale is None else np.asarray(scale, np.float64),
              loc=np.zeros(c_src) if loc is None else np.asarray(loc, np.float64), term_start=start,
              term_coef=np.asarray(coef, np.float64), term_a=np.asarray(ta, np.int32), term_b=np.asarray(tb, np.int32),
              coslat=None, inv_rcos=None, inv_dphi=None, inv_2dlam=None, pole_row=None)
  if lat is not None:
    plan.update(row_tables(lat, lon))
  plan.update(pool)
  return plan


def _p(x, c, plan):
  """(p(c), |p|(c)) of x [..., c_src] float32."""
  s, l = np.float64(plan["scale"][c]), np.float64(plan["loc"][c])
  xs = x[..., c].astype(np.float64) * s
  return xs + l, np.abs(xs) + np.abs(l)


def term_sum(x, plan, t0, t1):
  """(S, A, T) of the terms [t0, t1), added in ascending t."""
  S, A = np.zeros(x.shape[:-1]), np.zeros(x.shape[:-1])
  for t in range(t0, t1):
    coef, a, b = np.float64(plan["term_coef"][t]), int(plan["term_a"][t]), int(plan["term_b"][t])
    pa, ma = _p(x, a, plan)
    term, mag = coef * pa, np.abs(coef) * ma
    if b >= 0:
      pb, mb = _p(x, b, plan)
      term, mag = term * pb, mag * mb
    S, A = S + term, A + mag
  return S, A, t1 - t0


def curl(x, plan, vort, cu, cv):
  """(double result, k A) of VORTICITY (vort) or DIVERGENCE of u = p(cu), v = p(cv); x [..., G, B, c_src]."""
  n_lat, n_lon = int(plan["n_lat"]), int(plan["n_lon"])
  xg = x.reshape(x.shape[:-3] + (n_lat, n_lon) + x.shape[-2:])
  ca, cb = (cv, cu) if vort else (cu, cv)
  a, ma = _p(xg, ca, plan)                                    # [..., n_lat, n_lon, B]: differenced along the longitude
  b, mb = _p(xg, cb, plan)                                    # times cos(lat), differenced along the latitude
  idx = np.arange(n_lat)
  ip, im = np.minimum(idx + 1, n_lat - 1), np.maximum(idx - 1, 0)
  col = lambda v: np.asarray(v, np.float64)[:, None, None]
  cos, inv_rcos, inv_dphi, inv_2dlam = col(plan["coslat"]), col(plan["inv_rcos"]), col(plan["inv_dphi"]), np.float64(plan["inv_2dlam"])
  ap, am = np.roll(a, -1, axis=-2), np.roll(a, 1, axis=-2)
  bp, bm = np.take(b, ip, axis=-3) * cos[ip], np.take(b, im, axis=-3) * cos[im]
  x_, y_ = ap - am, bp - bm
  t1, t2 = x_ * inv_2dlam, y_ * inv_dphi
  r = (t1 - t2 if vort else t1 + t2) * inv_rcos
  mag = ((np.roll(ma, -1, axis=-2) + np.roll(ma, 1, axis=-2)) * abs(inv_2dlam)
         + (np.take(mb, ip, axis=-3) * np.abs(cos[ip]) + np.take(mb, im, axis=-3) * np.abs(cos[im])) * np.abs(inv_dphi)) * np.abs(inv_rcos)
  err = K_CURL * mag
  for i in np.flatnonzero(np.asarray(plan["pole_row"])):
    ia = 1 if i == 0 else n_lat - 2
    s = np.zeros(r.shape[:-3] + r.shape[-1:])
    for l in range(n_lon):                                    # ascending longitude
      s = s + r[..., ia, l, :]
    r[..., i, :, :] = (s / np.float64(n_lon))[..., None, :]
    err[..., i, :, :] = ((K_CURL + n_lon) * mag[..., ia, :, :].sum(axis=-2) / n_lon)[..., None, :]
  return r.reshape(x.shape[:-1]), err.reshape(x.shape[:-1])


def derive(x, plan):
  """x [..., G, B, c_src] float32 -> (d [..., G, B, c_d] float32, bound [..., G, B, c_d] float64)."""
  x = np.asarray(x, np.float32)
  c_d = len(plan["op"])
  out = np.empty(x.shape[:-1] + (c_d,), np.float32)
  slack = np.zeros(out.shape)                                 # the part of the bound beyond the rounding to float32
  with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
    for j in range(c_d):
      o, a, b = int(plan["op"][j]), int(plan["src_a"][j]), int(plan["src_b"][j])
      if o == COPY:
        out[..., j] = x[..., a]
        continue
      if o == NORM2:
        sa, la, sb, lb = (np.float64(v) for v in plan["affine"][j])
        u, v = x[..., a].astype(np.float64) * sa + la, x[..., b].astype(np.float64) * sb + lb
        r = np.sqrt(u * u + v * v)
        e = K_ROOT * EPS * np.abs(r)
      elif o in (SUM, NORM):
        s0, s1, s2 = (int(v) for v in plan["term_start"][j])
        r, A, T = term_sum(x, plan, s0, s1)
        e = T * EPS * A
        if o == NORM:
          r2, A2, T2 = term_sum(x, plan, s1, s2)
          r = np.sqrt(r * r + r2 * r2)
          e = np.hypot(e, T2 * EPS * A2) + K_ROOT * EPS * np.abs(r)
      elif o in (VORTICITY, DIVERGENCE):
        r, kA = curl(x, plan, o == VORTICITY, a, b)
        e = EPS * kA
      else:
        raise ValueError(f"op {o}")
      out[..., j] = r.astype(np.float32)
      slack[..., j] = e
    bound = np.where(plan["op"] == COPY, 0.0, np.spacing(np.abs(out)).astype(np.float64) + slack)
  return out, bound


def within(got, ref, bound):
  """The finite masks agree, NaN and the two infinities each for themselves, and the finite values lie within the bound.
  -> the largest error / bound, for the log."""
  got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
  np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
  np.testing.assert_array_equal(np.isposinf(got), np.isposinf(ref))
  np.testing.assert_array_equal(np.isneginf(got), np.isneginf(ref))
  ok = np.isfinite(ref)
  err = np.abs(got[ok].astype(np.float64) - ref[ok].astype(np.float64))
  lim = np.asarray(bound)[ok]
  assert np.all(err <= lim), f"largest error / bound {float(np.max(err / np.maximum(lim, 1e-300))):.3g}"
  return float(np.max(err / np.maximum(lim, 1e-300))) if err.size else 0.0
