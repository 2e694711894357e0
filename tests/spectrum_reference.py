"""Float64 yardstick of the spherical-harmonic power spectra (gc_spec_field / gc_ens_spectrum).
TEST INFRASTRUCTURE ONLY: the product holds no NumPy transform (gencast-flax-nnx_amd/spectra.py).

Straight loops over every summed index (j, lat, m, members: ascending), vectorised over the others.  Two kinds of tables:
  * `tables(lat, lon, lmax)`: built here from scipy.special.lpmv, as oracle/noise_oracle.py builds its harmonics -- no code
    shared with the product's recurrence (noise._normalized_legendre);
  * whatever float32 tables the device was given (`SphericalAnalysis.device_tables()`): the GPU tests analyse the same
    float32 data with the same float32 tables in binary64, so device and reference differ in summation order only.

The bound the GPU tests assert, u = 2^-53.  A Fourier product (float32 x float32) is exact in binary64, so that step
errs by at most (n_lon - 1) u sum_j |T f|; the Legendre step adds (n_lat + 1) u sum_lat |Q| |F| and carries the
Fourier error with weight sum_lat |Q|.  With Abar_lm = sum_lat |Q| sum_j |T f| (the nested sum of absolute terms,
`analyse` returns it) and a factor 2 for the reference's own rounding:
    da_lm = 2 (n_lon + n_lat + 2) u Abar_lm                                                    (`coef_tolerance`)
    dpower_l(a, da) = sum_{m <= l, parts} (2 |a| da + da^2) / (4 pi) + (2 l + 3) u power_l     (`power_tolerance`)
(2 l + 2 rounded squares through at most 2 l + 1 additions and one division).  The ensemble sums compose it:
    mean       dmean = (sum_i da_i) / M + M u (sum_i |a_i|) / M           M - 1 additions and a division
    difference d(p - q) = dp + dq + u |p - q|
    P0 = dpower(y, dy)   P2 = dpower(mean, dmean)   P4 = dpower(mean - y, d(mean - y))
    P1, P3, P5 = sum_i dpower(.) + M u P_k                                 M additions of complete powers
The device forms the Legendre sums with fused multiply-adds (fewer roundings than counted) and everything else in the
order of these loops, so no count grows.
"""
import numpy as np
import scipy.special

U = 2.0 ** -53
FOUR_PI = 4.0 * np.pi
SUM_NAMES = ("P0 truth", "P1 members", "P2 mean", "P3 member error", "P4 mean error", "P5 spread")


# ---- tables, independent of the product ------------------------------------------------------------------------------
def legendre(lat_deg, lmax):
  """P[m, l, lat] = N_lm P_l^m(sin lat), orthonormal on the unit sphere (Condon-Shortley phase included), 0 for l < m."""
  x = np.sin(np.deg2rad(np.asarray(lat_deg, np.float64)))
  P = np.zeros((lmax, lmax, x.shape[0]))
  for m in range(lmax):
    for l in range(m, lmax):
      norm = np.sqrt((2 * l + 1) / FOUR_PI * np.exp(scipy.special.gammaln(l - m + 1) - scipy.special.gammaln(l + m + 1)))
      P[m, l] = norm * scipy.special.lpmv(m, l, x)
  return P


def tables(lat_deg, lon_deg, lmax):
  """(Q [m, l, lat], cos_a [m, j], sin_a [m, j]) in float64: the definition of the issue, from lpmv."""
  P = legendre(lat_deg, lmax)
  Q = np.zeros_like(P)
  for m in range(lmax):
    Q[m, m:, :] = np.linalg.pinv(P[m, m:, :].T)
  n_lon = len(lon_deg)
  phi = np.deg2rad(np.asarray(lon_deg, np.float64))
  m = np.arange(lmax, dtype=np.float64)
  amp = np.where(m == 0, 1.0, np.sqrt(2.0)) / n_lon
  return Q, np.cos(m[:, None] * phi[None, :]) * amp[:, None], np.sin(m[:, None] * phi[None, :]) * amp[:, None]


# ---- the analysis ---------------------------------------------------------------------------------------------------
def analyse(field, Q, cos_a, sin_a):
  """field [n_lat, n_lon, N] -> (a [2, L, L, N] (part, m, l, column), Abar of the same shape: the nested sum of the
  absolute values of the same terms).  Entries with l < m are zero."""
  f = np.asarray(field, np.float64)
  Q = np.asarray(Q, np.float64)
  T = np.concatenate([np.asarray(cos_a, np.float64), np.asarray(sin_a, np.float64)])      # [2 L, n_lon]
  L = Q.shape[0]
  n_lat, n_lon, N = f.shape
  F = np.zeros((2 * L, n_lat, N))
  Fa = np.zeros((2 * L, n_lat, N))
  for j in range(n_lon):
    term = T[:, j, None, None] * f[None, :, j, :]
    F += term
    Fa += np.abs(term)
  F, Fa = F.reshape(2, L, n_lat, N), Fa.reshape(2, L, n_lat, N)
  a = np.zeros((2, L, L, N))
  A = np.zeros((2, L, L, N))
  for m in range(L):
    for lat in range(n_lat):
      q = Q[m, m:, lat]
      a[:, m, m:] += q[None, :, None] * F[:, m, lat][:, None, :]
      A[:, m, m:] += np.abs(q)[None, :, None] * Fa[:, m, lat][:, None, :]
  return a, A


def power(a):
  """a [2, L, L, N] -> [N, L]: (sum_m a_lm^2 + b_lm^2) / (4 pi), m ascending, the cosine term before the sine term."""
  L, N = a.shape[1], a.shape[3]
  p = np.zeros((N, L))
  for l in range(L):
    s = np.zeros(N)
    for m in range(l + 1):
      s = s + a[0, m, l] * a[0, m, l]
      s = s + a[1, m, l] * a[1, m, l]
    p[:, l] = s / FOUR_PI
  return p


def coef_tolerance(A, n_lat, n_lon):
  return 2.0 * (n_lon + n_lat + 2) * U * A


def power_tolerance(a, da):
  """[N, L]: sum_{m <= l, parts} (2 |a| da + da^2) / (4 pi) + (2 l + 3) u power_l."""
  L = a.shape[1]
  keep = (np.arange(L)[:, None] <= np.arange(L)[None, :])[None, :, :, None]                # m <= l
  t = np.where(keep, 2.0 * np.abs(a) * da + da * da, 0.0).sum(axis=(0, 1)) / FOUR_PI        # [l, N]
  return t.T + (2.0 * np.arange(L)[None, :] + 3.0) * U * power(a)


def field_spectrum(field, n_lat, n_lon, tabs, cols=None):
  """field [G, B, C] float32 -> (power [n, L], tolerance [n, L]) over the flattened columns n = b C + c (or those listed
  in `cols`); a column with a value that is not finite is NaN."""
  f = np.asarray(field).reshape(n_lat, n_lon, -1)
  if cols is not None:
    f = f[:, :, np.asarray(cols)]
  bad = ~np.isfinite(f).all(axis=(0, 1))
  a, A = analyse(np.where(bad[None, None, :], 0.0, f), *tabs)
  p, tol = power(a), power_tolerance(a, coef_tolerance(A, n_lat, n_lon))
  p[bad] = np.nan
  return p, tol


def ensemble(members, truth, n_lat, n_lon, tabs, cols=None):
  """members [M, G, B, C], truth [G, B, C] (float32) -> dict: sums [n, L, 6], tol [n, L, 6], member_power [M, n, L],
  member_tol [M, n, L], bad [n], coefficients (y, [x_i], mean) for identities."""
  members = np.asarray(members)
  M = members.shape[0]
  pick = (lambda f: f.reshape(n_lat, n_lon, -1)) if cols is None else (lambda f: f.reshape(n_lat, n_lon, -1)[:, :, np.asarray(cols)])
  y_f = pick(np.asarray(truth))
  x_f = [pick(members[i]) for i in range(M)]
  bad = ~np.isfinite(y_f).all(axis=(0, 1))
  for f in x_f:
    bad |= ~np.isfinite(f).all(axis=(0, 1))
  clean = lambda f: np.where(bad[None, None, :], 0.0, f)
  y, Ay = analyse(clean(y_f), *tabs)
  dy = coef_tolerance(Ay, n_lat, n_lon)
  xs, dxs = [], []
  for f in x_f:
    a, A = analyse(clean(f), *tabs)
    xs.append(a)
    dxs.append(coef_tolerance(A, n_lat, n_lon))
  tot, tot_abs, dtot = np.zeros_like(y), np.zeros_like(y), np.zeros_like(y)
  for a, da in zip(xs, dxs):                                                   # ascending slot order
    tot = tot + a
    tot_abs += np.abs(a)
    dtot += da
  mean = tot / M
  dmean = dtot / M + M * U * tot_abs / M
  diff = lambda p, dp, q, dq: (p - q, dp + dq + U * np.abs(p - q))
  n, L = y.shape[3], y.shape[1]
  sums, tol = np.zeros((n, L, 6)), np.zeros((n, L, 6))
  sums[..., 0], tol[..., 0] = power(y), power_tolerance(y, dy)
  sums[..., 2], tol[..., 2] = power(mean), power_tolerance(mean, dmean)
  e, de = diff(mean, dmean, y, dy)
  sums[..., 4], tol[..., 4] = power(e), power_tolerance(e, de)
  member_power, member_tol = np.zeros((M, n, L)), np.zeros((M, n, L))
  for i, (a, da) in enumerate(zip(xs, dxs)):
    member_power[i], member_tol[i] = power(a), power_tolerance(a, da)
    sums[..., 1] += member_power[i]
    tol[..., 1] += member_tol[i]
    e, de = diff(a, da, y, dy)
    sums[..., 3] += power(e)
    tol[..., 3] += power_tolerance(e, de)
    e, de = diff(a, da, mean, dmean)
    sums[..., 5] += power(e)
    tol[..., 5] += power_tolerance(e, de)
  for k in (1, 3, 5):
    tol[..., k] += M * U * sums[..., k]
  sums[bad] = np.nan
  member_power[:, bad] = np.nan
  return dict(sums=sums, tol=tol, member_power=member_power, member_tol=member_tol, bad=bad, y=y, xs=xs, mean=mean)


# ---- the library's noise field: a spectrum known in closed form ----------------------------------------------------
def noise_coefficient_power(z):
  """z [2, L, L, N]: the normals of a noise field (part, m, l, column; noise.py / gc_noise.hip).  The field is
  sqrt(4 pi) sum_l sqrt(p_l / (2l+1)) sum_m z_lm Y_lm with p_l = 1 / L, so power[l] = p_l / (2l+1) sum_m z_lm^2
  (no sine term at m = 0) -> [N, L]; its expectation is 1 / L."""
  z = np.asarray(z, np.float64)
  L, N = z.shape[1], z.shape[3]
  p = np.zeros((N, L))
  for l in range(L):
    s = np.zeros(N)
    for m in range(l + 1):
      s = s + z[0, m, l] ** 2
      if m > 0:
        s = s + z[1, m, l] ** 2
    p[:, l] = (1.0 / L) / (2 * l + 1) * s
  return p


def noise_coefficients(z):
  """The harmonic coefficients a [2, L, L, N] of that field: sqrt(4 pi p_l / (2l+1)) z_lm, zero for l < m and for the
  sine part at m = 0."""
  z = np.asarray(z, np.float64)
  L = z.shape[1]
  l = np.arange(L, dtype=np.float64)
  a = z * np.sqrt(FOUR_PI * (1.0 / L) / (2.0 * l + 1.0))[None, None, :, None]
  a = np.where((np.arange(L)[:, None] <= np.arange(L)[None, :])[None, :, :, None], a, 0.0)
  a[1, 0] = 0.0
  return a


def pointwise_gain(Q, cos_a, sin_a):
  """S [2, L, L]: sum_lat |Q[m, l, lat]| sum_j |T[part, m, j]| -- a field error of at most eps at every node moves the
  coefficient a_lm by at most eps S_lm."""
  Q = np.abs(np.asarray(Q, np.float64)).sum(axis=2)                                         # [m, l]
  return np.stack([np.abs(np.asarray(cos_a, np.float64)).sum(axis=1)[:, None] * Q,
                   np.abs(np.asarray(sin_a, np.float64)).sum(axis=1)[:, None] * Q])
