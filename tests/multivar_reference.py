"""The float64 definition of the multivariate ensemble scores (include/gencast_hip.h, gc_ens_energy_*, gc_ens_variogram_*;
DESIGN.md section 8k): plain loops over pairs and offsets with `np.isfinite` masks.  The yardstick of tests/test_multivar.py
and tests/test_gpu_multivar*.py.

Members x_0 .. x_{M-1} and the truth y are [G, B, c_out] float32, w[g] the node weight.  A point (g, b, c) is valid iff y
and all M members are finite there.  Write x_M = y.

Energy.  The plan gives K groups (1 <= K <= 32) and a per-channel scale: group[c] in {-1, 0 .. K-1}, where -1 means the
channel is in no group; every group is non-empty; a[c] is finite and > 0 for grouped channels.  Per batch member b, group k
and pair 0 <= i < j <= M, with pair index p = j (j - 1) / 2 + i and P = M (M + 1) / 2:
  D2[b][k][p] = sum omega (d d) over the valid points of the group, omega = (double)w[g] a[c], d = (double)x_i - (double)x_j
  S0[b][k] = sum omega over the same points;  invalid = the number of skipped points of grouped channels.
Invalid points are skipped, not multiplied by zero.  On the host D[i][j] = sqrt(D2 / S0), err = mean_i D[i][M],
pair = mean_{i<j<M} D[i][j], fair ES = err - pair / 2, ensemble ES = err - (M - 1) / M pair / 2.

Variogram.  The plan gives the grid n_lat n_lon = G with node = i n_lon + j, O offsets (di, dj) and an order p in
{0.5, 1, 2}, formed with sqrt, identity and a product.  The partner of (i, j) is (i + di, (j + dj) mod n_lon); the pair is
skipped when i + di leaves [0, n_lat) and when either end is invalid.  Per valid pair, in double: omega = (w[g] + w[g']) / 2,
v(u) = |u_g - u_g'|^p, vx = (sum_i v(x_i)) / M in ascending slot order, vy = v(y).  Per (b, c, o): V0 = sum omega,
V1 = sum omega (vy - vx)^2, V2 = sum omega vx, V3 = sum omega vy, and a pair count."""
import numpy as np


def pair_index(i, j):
  assert 0 <= i < j
  return j * (j - 1) // 2 + i


def pairs(M):
  """[(i, j)] in the order of the pair index, over the M + 1 fields (slot M: the truth)."""
  return [(i, j) for j in range(1, M + 1) for i in range(j)]


def energy(members, truth, w, group, scale):
  """members [M, G, B, C] float32, truth [G, B, C] float32, w [G] float32, group [C] int, scale [C] float64 -> dict of
  d2 [B, K, P], s0 [B, K], invalid (int) and n [K]: the number of terms of a sum, G |group k|.  Every term is >= 0, so the
  sums are their own sums of absolute values."""
  members, truth = np.asarray(members, np.float32), np.asarray(truth, np.float32)
  M, G, B, C = members.shape
  group = np.asarray(group, np.int64)
  K = int(group.max()) + 1
  ok = np.isfinite(members).all(axis=0) & np.isfinite(truth)                       # [G, B, C]
  a = np.where(group >= 0, np.asarray(scale, np.float64), 0.0)
  omega = np.asarray(w, np.float32).astype(np.float64)[:, None, None] * a[None, None, :]
  member_of = np.zeros((C, K))
  for c in range(C):
    if group[c] >= 0:
      member_of[c, group[c]] = 1.0
  fields = [np.where(ok, x, np.float32(0.0)).astype(np.float64) for x in list(members) + [truth]]
  d2 = np.zeros((B, K, M * (M + 1) // 2))
  for p, (i, j) in enumerate(pairs(M)):
    d = fields[i] - fields[j]
    term = np.where(ok, omega * (d * d), 0.0)
    d2[:, :, p] = term.sum(axis=0) @ member_of
  s0 = np.where(ok, omega, 0.0).sum(axis=0) @ member_of
  invalid = int(((~ok) & (group >= 0)[None, None, :]).sum())
  return dict(d2=d2, s0=s0, invalid=invalid, n=G * member_of.sum(axis=0))


def energy_tolerance(ref):
  """(n + 8) 2^-53 sum |term| per sum, n = G |group| the number of terms: each term carries at most three roundings (omega,
  d d, their product), the difference is exact, and the additions of the two sides differ in order."""
  return (ref["n"][None, :, None] + 8.0) * 2.0 ** -53 * ref["d2"]


def energy_scores(d2, s0, M):
  """err, pair [B, K] and the fair and the ensemble energy score of every batch member, as the issue writes them."""
  d2, s0 = np.asarray(d2, np.float64), np.asarray(s0, np.float64)
  B, K, _ = d2.shape
  err, pair = np.zeros((B, K)), np.zeros((B, K))
  with np.errstate(invalid="ignore", divide="ignore"):
    for b in range(B):
      for k in range(K):
        D = lambda i, j: np.sqrt(d2[b, k, pair_index(i, j)] / s0[b, k])   # noqa: E731
        err[b, k] = np.mean([D(i, M) for i in range(M)])
        pair[b, k] = np.mean([D(i, j) for j in range(1, M) for i in range(j)])
  return dict(err=err, pair=pair, fair=err - 0.5 * pair, ensemble=err - 0.5 * (M - 1) / M * pair)


def vpow(u, p):
  a = np.abs(u)
  if p == 0.5:
    return np.sqrt(a)
  if p == 1.0:
    return a
  assert p == 2.0
  return a * a


def variogram(members, truth, w, n_lat, n_lon, offsets, p):
  """members [M, G, B, C] float32, truth [G, B, C] float32, w [G] float32 -> dict of sums [4, B, C, O], counts [B, C, O]
  uint64 and abs_sums [4, B, C, O] (every term is >= 0: the sums themselves)."""
  members, truth = np.asarray(members, np.float32), np.asarray(truth, np.float32)
  M, G, B, C = members.shape
  assert n_lat * n_lon == G
  ok = (np.isfinite(members).all(axis=0) & np.isfinite(truth)).reshape(n_lat, n_lon, B, C)
  x = [np.where(ok, f.reshape(n_lat, n_lon, B, C), np.float32(0.0)).astype(np.float64) for f in list(members) + [truth]]
  wd = np.asarray(w, np.float32).astype(np.float64).reshape(n_lat, n_lon)
  O = len(offsets)
  sums = np.zeros((4, B, C, O))
  counts = np.zeros((B, C, O), np.uint64)

  def ends(arr, di, dj):
    """(the points whose partner row exists, their partners): rows i with 0 <= i + di < n_lat, columns wrapped."""
    lo, hi = max(0, -di), min(n_lat, n_lat - di)
    return arr[lo:hi], np.roll(arr, -dj, axis=1)[lo + di:hi + di]

  for o, (di, dj) in enumerate(offsets):
    ok_a, ok_b = ends(ok, di, dj)
    both = ok_a & ok_b
    w_a, w_b = ends(wd, di, dj)
    omega = (0.5 * (w_a + w_b))[:, :, None, None]
    vsum = np.zeros(both.shape)
    for i in range(M):                                     # ascending slot order
      a, b = ends(x[i], di, dj)
      vsum = vsum + vpow(a - b, p)
    vx = vsum / float(M)
    a, b = ends(x[M], di, dj)
    vy = vpow(a - b, p)
    e = vy - vx
    for k, term in enumerate((omega + 0.0 * vx, omega * (e * e), omega * vx, omega * vy)):
      sums[k, :, :, o] = np.where(both, term, 0.0).sum(axis=(0, 1))
    counts[:, :, o] = both.sum(axis=(0, 1))
  return dict(sums=sums, counts=counts, abs_sums=sums.copy())


def variogram_tolerance(ref, G, M):
  """(G + M + 8) 2^-53 sum |term| per sum: at most G additions whose order differs, and a term that carries the M
  additions of vx (the same on both sides, in ascending slot order) and a handful of roundings."""
  return (G + M + 8) * 2.0 ** -53 * ref["abs_sums"]
