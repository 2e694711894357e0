"""The definition of gc_ens_tail_score (include/gencast_hip.h) in float64 NumPy, written independently of
the kernel's form: no sort, the pair term as a sum over the pairs i < j in slot order, the error term as a mean over slots.

Members x_0..x_{M-1} (2 <= M <= 64) and truth y are [G,B,c_out] float32 in the sample layout.  w[g] are the float node
weights of gc_ens_set_node_weight.  There are T threshold fields thr_t (1 <= T <= 8), each [G,B,c_out] float32, with a
direction dir_t != 0.  This is the convention of gc_ens_event_set.
A point counts for threshold t when y, all M members and thr_t are finite there.  A NaN threshold means "not evaluated"
for that t only.
Per counted point, with x_(0) <= ... <= x_(M-1) the members in ascending order:
  v(z) = fmaxf(z, thr_t) when dir_t > 0.  This is the upper tail, weight 1{z >= thr}.
  v(z) = fminf(z, thr_t) when dir_t < 0.  Both are exact in float32.
  u_k = v(x_(k)), which is still ascending.
  AE = sum_{k=0}^{M-1} |(double)u_k - (double)v(y)|, added in ascending k.  ae = AE / M.
  PD = sum_{k=1}^{M-1} (double)(k (M-k)) ((double)u_k - (double)u_{k-1}), added in ascending k.  d = PD / (M(M-1)/2).
    This "gap form" equals sum_{i<j} |u_i - u_j|.  Every term is non-negative, so there is no cancellation.
  o = [y in the event], strict as in section 8f: y > thr_t for dir_t > 0, y < thr_t for dir_t < 0.
Per (t, b, c), over the counted nodes:
  sums[t][b][c][0..3] = sum w, sum w ae, sum w d, sum w o
  counts[t][b][c] = counted points (uint64)
  invalid[t] = points skipped
"""
import numpy as np


def clamp(z, thr, direction):
  """v(z) on float32 values (exact: the result is one of the two operands)."""
  z, thr = np.asarray(z, np.float32), np.asarray(thr, np.float32)
  return np.maximum(z, thr) if direction > 0 else np.minimum(z, thr)


def pair_form(u):
  """sum_{i<j} |u_i - u_j| over axis 0 in float64, pair after pair in slot order, no sort."""
  u = np.asarray(u, np.float64)
  out = np.zeros(u.shape[1:])
  for i in range(u.shape[0]):
    for j in range(i + 1, u.shape[0]):
      out += np.abs(u[i] - u[j])
  return out


def gap_form(u):
  """sum_{k=1}^{M-1} k (M - k) (u_(k) - u_(k-1)) over axis 0 in float64, from the sorted values: the kernel's form."""
  s = np.sort(np.asarray(u, np.float64), axis=0)
  M = s.shape[0]
  out = np.zeros(s.shape[1:])
  for k in range(1, M):
    out += float(k * (M - k)) * (s[k] - s[k - 1])
  return out


def point_terms(members, truth, thr, direction):
  """(ae, d, o, counted) per point [G, B, C] for one threshold field: ae the mean over slots of |v(x_i) - v(y)|, d the mean
  over pairs of |v(x_i) - v(x_j)|, o the strict event of the truth; zero where the point does not count."""
  members, truth, thr = np.asarray(members, np.float32), np.asarray(truth, np.float32), np.asarray(thr, np.float32)
  M = members.shape[0]
  counted = np.isfinite(truth) & np.isfinite(members).all(axis=0) & np.isfinite(thr)
  safe = lambda a: np.where(counted, a, np.float32(0.0))
  x, y, t = safe(members), safe(truth), safe(thr)
  u = clamp(x, t, direction).astype(np.float64)
  vy = clamp(y, t, direction).astype(np.float64)
  ae = np.abs(u - vy).mean(axis=0)
  d = pair_form(u) / float(M * (M - 1) // 2)
  o = (y > t) if direction > 0 else (y < t)
  return np.where(counted, ae, 0.0), np.where(counted, d, 0.0), (o & counted).astype(np.float64), counted


def reference(members, truth, node_w, thresholds, directions):
  """-> dict(sums [T, B, C, 4] float64, counts [T, B, C] uint64, invalid [T] uint64)."""
  members, truth = np.asarray(members, np.float32), np.asarray(truth, np.float32)
  thresholds = np.asarray(thresholds, np.float32)
  w = np.asarray(node_w, np.float32).astype(np.float64)[:, None, None]
  T = thresholds.shape[0]
  sums = np.zeros((T,) + truth.shape[1:] + (4,))
  counts = np.zeros((T,) + truth.shape[1:], np.uint64)
  invalid = np.zeros(T, np.uint64)
  for t in range(T):
    ae, d, o, counted = point_terms(members, truth, thresholds[t], directions[t])
    for k, term in enumerate((counted.astype(np.float64), ae, d, o)):
      sums[t, ..., k] = (w * term).sum(axis=0)
    counts[t] = counted.sum(axis=0)
    invalid[t] = counted.size - int(counted.sum())
  return {"sums": sums, "counts": counts, "invalid": invalid}


def sum_tolerance(ref, G, M):
  """(G + M (M - 1) / 2 + 8) 2^-53 sum |term| per sum.  The per-point sums have at most M (M - 1) / 2 non-negative terms on
  either side, and the node sums differ only in order.  Every term is >= 0, so sum |term| is the sum itself."""
  return (G + M * (M - 1) // 2 + 8) * 2.0 ** -53 * np.abs(ref["sums"])


def scores(ref, M):
  s = ref["sums"]
  with np.errstate(invalid="ignore", divide="ignore"):
    return {"twcrps": (s[..., 1] - 0.5 * s[..., 2]) / s[..., 0],
            "twcrps_ensemble": (s[..., 1] - 0.5 * (M - 1.0) / M * s[..., 2]) / s[..., 0],
            "abs_error": s[..., 1] / s[..., 0], "pair_distance": s[..., 2] / s[..., 0], "base_rate": s[..., 3] / s[..., 0]}
