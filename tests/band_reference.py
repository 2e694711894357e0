"""Float64 yardstick of the spectral band views (gc_ens_band_set / gc_ens_band).
TEST INFRASTRUCTURE ONLY: the product holds no NumPy transform.

The definition, for one field (a member or the truth) and one source column f on the grid of `spectrum_reference`:
  1  a = analysis(f)                                                    `spectrum_reference.analyse`
  2  b[part][m][l] = w[l] a[part][m][l]
  3  G[part][m][lat] = sum_{l = m .. L-1} S[m][lat][l] b[part][m][l]     l ascending;  S[m][lat][l] = N_lm P_l^m(sin lat)
  4  g(lat, j) = sum_m (cos_s[m][j] G[0][m][lat] + sin_s[m][j] G[1][m][lat])   m ascending, the cosine term before the sine term
     cos_s[m][j] = amp_m cos(m phi_j), sin_s likewise, amp_0 = 1, else sqrt 2
  5  d = g, or with `complement` d = f - g;  the device rounds d to float32 once
Straight loops over every summed index (j and lat inside `analyse`, l, m: ascending), vectorised over the others.  Two kinds
of tables: `synthesis_tables(lat, lon, lmax)`, built here from scipy.special.lpmv (no code shared with the product's
recurrence), or whatever float32 tables the device was given -- the GPU tests send the same float32 data through the same
float32 tables in binary64, so device and reference differ in summation order and in the fusing of multiply-adds only.

The bound, u = 2^-53, returned with the value BEFORE the final rounding; every rounding counted, one-sided, then doubled for
the reference's own rounding (`coef_tolerance` holds that factor already):
  a   da = coef_tolerance(Abar)                                          (n_lon - 1) + (n_lat + 1) roundings, doubled
  b   db = |w| da + 2 u |w a|                                            one rounded product
  G   dG = sum_l |S| db + 2 (n_l + 1) u sum_l |S| |b|,  n_l = L - m      n_l rounded products, n_l - 1 additions: at most
                                                                         n_l + 1 roundings, each of a partial sum that the
                                                                         nested sum of absolute terms Gbar bounds
  g   dg = sum_m (|cos_s| dG0 + |sin_s| dG1) + 2 (2 L + 1) u gbar        2 L products, 2 L - 1 additions; gbar = sum_m
                                                                         (|cos_s| Gbar0 + |sin_s| Gbar1): nested, it bounds
                                                                         every partial sum of the computed terms to first order
  d   dd = dg (+ 2 u (|f| + |g|) with complement)                        one subtraction of an exact float32 widened to double
The device forms steps 3 and 4 with fused multiply-adds (one rounding per term, fewer than counted) and in the order of
these loops, so no count grows.  The bound is derived, not measured.
"""
import numpy as np

from tests import spectrum_reference as R

U = R.U


def synthesis_tables(lat_deg, lon_deg, lmax):
  """(S [m, lat, l], cos_s [m, j], sin_s [m, j]) in float64, from lpmv: the plain A_m of every m (zero for l < m) and the
  Fourier synthesis rows."""
  S = np.ascontiguousarray(np.transpose(R.legendre(lat_deg, lmax), (0, 2, 1)))
  phi = np.deg2rad(np.asarray(lon_deg, np.float64))
  m = np.arange(lmax, dtype=np.float64)
  amp = np.where(m == 0, 1.0, np.sqrt(2.0))
  return S, np.cos(m[:, None] * phi[None, :]) * amp[:, None], np.sin(m[:, None] * phi[None, :]) * amp[:, None]


def synthesise(b, db, babs, S, cos_s, sin_s):
  """b, db, babs [2, L, L, N] (part, m, l, column): the weighted coefficients, their error and their absolute values ->
  (g [n_lat, n_lon, N], dg one-sided without the factor 2, of the same shape)."""
  S, cos_s, sin_s = (np.asarray(t, np.float64) for t in (S, cos_s, sin_s))
  L, n_lat = S.shape[0], S.shape[1]
  n_lon, N = cos_s.shape[1], b.shape[3]
  G = np.zeros((2, L, n_lat, N))
  Gabs, Gin = np.zeros_like(G), np.zeros_like(G)
  for l in range(L):                                       # S[m, :, l] is zero for m > l: those rows add exact zeros
    s = S[None, :, :, l, None]                             # [1, m, lat, 1]
    G += s * b[:, :, None, l, :]
    Gabs += np.abs(s) * babs[:, :, None, l, :]
    Gin += np.abs(s) * db[:, :, None, l, :]
  n_l = (L - np.arange(L, dtype=np.float64))[None, :, None, None]
  dG = Gin + (n_l + 1.0) * U * Gabs
  g = np.zeros((n_lat, n_lon, N))
  gabs, gin = np.zeros_like(g), np.zeros_like(g)
  for m in range(L):
    for part, t in ((0, cos_s), (1, sin_s)):
      row = t[m][None, :, None]                            # [1, j, 1]
      g += row * G[part, m][:, None, :]
      gabs += np.abs(row) * Gabs[part, m][:, None, :]
      gin += np.abs(row) * dG[part, m][:, None, :]
  return g, gin + (2.0 * L + 1.0) * U * gabs


def view(field, w, complement, atabs, stabs):
  """field [n_lat, n_lon, N] (finite), w [L] or [L, N] (a response per column), complement a bool or [N] ->
  (d [n_lat, n_lon, N] float64 before the final rounding, tolerance of the same shape)."""
  f = np.asarray(field, np.float64)
  n_lat, n_lon, N = f.shape
  a, A = R.analyse(f, *atabs)
  da = R.coef_tolerance(A, n_lat, n_lon) / 2.0             # one-sided: the factor 2 goes on at the end
  w = np.asarray(w, np.float64)
  w = np.broadcast_to(w[:, None] if w.ndim == 1 else w, (a.shape[2], N))[None, None, :, :]
  b = w * a
  db = np.abs(w) * da + U * np.abs(b)
  g, dg = synthesise(b, db, np.abs(b), *stabs)
  comp = np.broadcast_to(np.asarray(complement, bool), (N,))[None, None, :]
  d = np.where(comp, f - g, g)
  tol = dg + np.where(comp, U * (np.abs(f) + np.abs(g)), 0.0)
  return d, 2.0 * tol


def band_fields(field, n_lat, n_lon, response, complement, src_channel, band, atabs, stabs):
  """One field [G, B, c_src] float32 through a plan (response [K, L], complement [K], src_channel, band [c_d]) ->
  (d [G, B, c_d] float64, tol [G, B, c_d], bad [B, c_src]: the source columns with a value that is not finite).  A derived
  channel that reads such a column is NaN at every node.  (The analysis of a column gives the same bits however many bands
  read it: here it simply runs per derived column.)"""
  field = np.asarray(field)
  G, B, c_src = field.shape
  response, complement = np.asarray(response, np.float64), np.asarray(complement).astype(bool)
  src_channel, band = np.asarray(src_channel), np.asarray(band)
  c_d = len(band)
  f = field.reshape(n_lat, n_lon, B, c_src)
  bad = ~np.isfinite(f).all(axis=(0, 1))                   # [B, c_src]
  cols = f[:, :, :, src_channel]                           # [n_lat, n_lon, B, c_d]
  bad_d = bad[:, src_channel]                              # [B, c_d]
  clean = np.where(bad_d[None, None], 0.0, cols).reshape(n_lat, n_lon, B * c_d)
  w = np.tile(response[band].T, (1, B))                    # [L, B c_d]: column b c_d + j has band[j]
  d, tol = view(clean, w, np.tile(complement[band], B), atabs, stabs)
  d = d.reshape(n_lat, n_lon, B, c_d)
  d[:, :, bad_d] = np.nan
  return d.reshape(G, B, c_d), tol.reshape(G, B, c_d), bad


def check(got, ref, tol, what=""):
  """The assertion of the GPU tests: NaN patterns equal, and float32(ref - tol) <= got <= float32(ref + tol) at every finite
  point; prints the share of bit-equal values and the worst ratio to the bound first."""
  got = np.asarray(got)
  nan = np.isnan(ref)
  lo, hi = (ref - tol).astype(np.float32), (ref + tol).astype(np.float32)
  ok = ~nan
  with np.errstate(invalid="ignore", divide="ignore"):
    equal = float(np.mean(got[ok] == ref[ok].astype(np.float32))) if ok.any() else 1.0
    half_ulp = 0.5 * np.spacing(np.abs(ref[ok]).astype(np.float32)).astype(np.float64)
    ratio = np.abs(got[ok].astype(np.float64) - ref[ok]) / (tol[ok] + half_ulp)
  print(f"{what}: bit-equal to the rounded reference {equal:.4f}, worst |got - ref| / (bound + half a float32 ulp) "
        f"{float(ratio.max()) if ratio.size else 0.0:.3g}, largest bound / |ref| {float(np.max(tol[ok] / np.maximum(np.abs(ref[ok]), 1e-300))) if ok.any() else 0.0:.3g}")
  assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs"
  assert np.all((got[ok] >= lo[ok]) & (got[ok] <= hi[ok])), f"{what}: outside the bound"
