"""The float64 yardstick of the ensemble scores: DESIGN.md section 8c, restated literally.

Test infrastructure only (the product never imports it).  Loops run over members and member pairs; NumPy only
vectorises over the points.  `members` [M, G, B, C] and `truth` [G, B, C] are float32 (the device's inputs), `w` [G].
"""
import numpy as np

SUM_NAMES = ("S0", "S1", "S2", "S3", "S4", "S5")


def point_terms(members, truth):
  """Per point, in float64 from the float32 values: dict(valid, members_finite, m, s2, ae, d, r)."""
  members = np.asarray(members, dtype=np.float32)
  truth = np.asarray(truth, dtype=np.float32)
  M = members.shape[0]
  x = members.astype(np.float64)
  y = truth.astype(np.float64)
  members_finite = np.ones(truth.shape, bool)
  for i in range(M):
    members_finite &= np.isfinite(x[i])
  valid = members_finite & np.isfinite(y)
  with np.errstate(invalid="ignore", over="ignore"):
    s = np.zeros(truth.shape)
    for i in range(M):                                   # ascending slot order
      s = s + x[i]
    m = s / M
    s2 = np.zeros(truth.shape)
    for i in range(M):                                   # second pass
      s2 = s2 + (x[i] - m) ** 2
    s2 = s2 / (M - 1)
    ae = np.zeros(truth.shape)
    for i in range(M):
      ae = ae + np.abs(x[i] - y)
    ae = ae / M
    d = pair_sum_brute(x) / (M * (M - 1) / 2)
    r = np.zeros(truth.shape, np.int64)
    for i in range(M):
      r += members[i] < truth                             # a member equal to the truth is not below it
  return dict(valid=valid, members_finite=members_finite, m=m, s2=s2, ae=ae, d=d, r=r)


def pair_sum_brute(x):
  """sum_{i<j} |x_i - x_j| along axis 0, pair by pair."""
  x = np.asarray(x, dtype=np.float64)
  M = x.shape[0]
  out = np.zeros(x.shape[1:])
  with np.errstate(invalid="ignore"):
    for i in range(M):
      for j in range(i + 1, M):
        out = out + np.abs(x[i] - x[j])
  return out


def pair_sum_sorted(x):
  """The same sum from the order statistics: sum_k (2k - M + 1) x_(k)."""
  xs = np.sort(np.asarray(x, dtype=np.float64), axis=0)
  M = xs.shape[0]
  out = np.zeros(xs.shape[1:])
  for k in range(M):
    out = out + (2 * k - M + 1) * xs[k]
  return out


def reference(members, truth, w):
  """-> dict: sums [B, C, 6], abs_sums [B, C, 6] (the sums of the absolute values of the same terms: the scale of the
  tolerance), hist [B, C, M + 1] uint64, invalid (points skipped), mean / variance [G, B, C] float64 (NaN where a
  member is not finite)."""
  t = point_terms(members, truth)
  M = np.asarray(members).shape[0]
  G, B, C = np.asarray(truth).shape
  wg = np.asarray(w, dtype=np.float32).astype(np.float64).reshape(G, 1, 1)
  y = np.asarray(truth, dtype=np.float32).astype(np.float64)
  valid = t["valid"]
  with np.errstate(invalid="ignore", over="ignore"):
    e = t["m"] - y
    terms = [wg * np.ones((G, B, C)), wg * e, wg * (e * e), wg * t["s2"], wg * t["ae"], wg * t["d"]]
  sums = np.stack([np.where(valid, q, 0.0).sum(axis=0) for q in terms], axis=-1)
  abs_sums = np.stack([np.abs(np.where(valid, q, 0.0)).sum(axis=0) for q in terms], axis=-1)
  hist = np.zeros((B, C, M + 1), np.uint64)
  for r in range(M + 1):
    hist[..., r] = (valid & (t["r"] == r)).sum(axis=0)
  nan = np.float64("nan")
  return dict(sums=sums, abs_sums=abs_sums, hist=hist, invalid=int((~valid).sum()),
              mean=np.where(t["members_finite"], t["m"], nan), variance=np.where(t["members_finite"], t["s2"], nan))


def scores(ref, M):
  """The derived scores from a `reference` result, by the formulas of the issue."""
  S = [ref["sums"][..., k] for k in range(6)]
  rmse, spread = np.sqrt(S[2] / S[0]), np.sqrt(S[3] / S[0])
  return dict(rmse=rmse, spread=spread, spread_skill_ratio=np.sqrt((M + 1) / M) * spread / rmse,
              crps=(S[4] - 0.5 * S[5]) / S[0], crps_ensemble=(S[4] - 0.5 * (M - 1) / M * S[5]) / S[0],
              bias=S[1] / S[0], valid_weight=S[0])


def sum_tolerance(ref, G, M):
  """|device - reference| <= (G + M^2 + 8) 2^-53 A_k: G terms are added per column, at most about M^2 roundings go into
  one term, and summation order is the only difference between the two computations."""
  return (G + M * M + 8) * 2.0 ** -53 * ref["abs_sums"]


def float32_neighbours(a):
  """(lower, upper): the float32 neighbours of np.float32(a)."""
  f = np.asarray(a, dtype=np.float64).astype(np.float32)
  return np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
