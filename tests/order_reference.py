"""The float64 definition of the ensemble order statistics (include/gencast_hip.h, gc_ens_order_*):
`np.sort` along the member axis, then exactly the expressions of the header.  Bins are looped over, so the full-size
cases stay small in memory.  The yardstick of tests/test_order.py and tests/test_gpu_order*.py."""
import numpy as np


def plan(probs, M):
  """(lo, hi, f) per probability, all in double: h = p (M - 1), lo = min(floor(h), M - 1), hi = min(lo + 1, M - 1), f = h - lo."""
  p = np.asarray(probs, np.float64).reshape(-1)
  h = p * float(M - 1)
  lo = np.minimum(np.floor(h).astype(np.int64), M - 1)
  hi = np.minimum(lo + 1, M - 1)
  return lo, hi, h - lo.astype(np.float64)


def quantile_fields(members, probs):
  """[Q, G, B, C] float32: (float)(x_(lo+1) + f (x_(hi+1) - x_(lo+1))) in double where all members are finite, NaN elsewhere."""
  members = np.asarray(members, np.float32)
  M = members.shape[0]
  valid = np.isfinite(members).all(axis=0)
  s = np.sort(np.where(valid[None], members, np.float32(0.0)), axis=0)
  lo, hi, f = plan(probs, M)
  out = np.empty((len(lo),) + members.shape[1:], np.float32)
  for q in range(len(lo)):
    a, b = s[lo[q]].astype(np.float64), s[hi[q]].astype(np.float64)
    with np.errstate(over="ignore"):
      out[q] = np.where(valid, (a + f[q] * (b - a)).astype(np.float32), np.float32(np.nan))
  return out


def reference(members, truth, w, probs=()):
  """members [M, G, B, C] float32, truth [G, B, C] float32, w [G] float32 -> dict of
  bins [B, C, M + 1, 2], extra [B, C, 3], pinball [B, C, Q], counts [B, C, Q + 1] uint64, invalid (int), fields [Q, G, B, C]
  and abs_bins / abs_extra / abs_pinball: the sums of the absolute values of the same terms (for `sum_tolerance`)."""
  members, truth = np.asarray(members, np.float32), np.asarray(truth, np.float32)
  M, G, B, C = members.shape
  probs = np.asarray(probs, np.float64).reshape(-1)
  Q = len(probs)
  valid = np.isfinite(members).all(axis=0)
  ok = valid & np.isfinite(truth)
  s = np.sort(np.where(valid[None], members, np.float32(0.0)), axis=0).astype(np.float64)
  y = np.where(ok, truth, np.float32(0.0)).astype(np.float64)
  wk = np.asarray(w, np.float32).astype(np.float64)[:, None, None] * ok          # the weight of a counted point, else 0
  bins = np.zeros((B, C, M + 1, 2))
  abs_bins = np.zeros((B, C, M + 1, 2))
  for k in range(M + 1):
    if k == 0:
      alpha, beta = np.zeros_like(y), np.maximum(s[0] - y, 0.0)
    elif k == M:
      alpha, beta = np.maximum(y - s[M - 1], 0.0), np.zeros_like(y)
    else:
      c = np.minimum(np.maximum(y, s[k - 1]), s[k])
      alpha, beta = c - s[k - 1], s[k] - c
    for j, t in enumerate((alpha, beta)):
      term = np.where(ok, wk * t, 0.0)
      bins[:, :, k, j] = term.sum(axis=0)
      abs_bins[:, :, k, j] = np.abs(term).sum(axis=0)
  extra = np.stack([wk.sum(axis=0), (wk * (ok & (y < s[0]))).sum(axis=0), (wk * (ok & (y > s[M - 1]))).sum(axis=0)], axis=-1)
  fields = quantile_fields(members, probs)
  pinball, abs_pinball = np.zeros((B, C, Q)), np.zeros((B, C, Q))
  counts = np.zeros((B, C, Q + 1), np.uint64)
  for q in range(Q):
    fq = np.where(ok, fields[q], np.float32(0.0))
    u = y - fq.astype(np.float64)
    term = np.where(ok, wk * (u * (probs[q] - (u < 0.0))), 0.0)
    pinball[:, :, q] = term.sum(axis=0)
    abs_pinball[:, :, q] = np.abs(term).sum(axis=0)
    counts[:, :, q] = (ok & (np.where(ok, truth, np.float32(0.0)) < fq)).sum(axis=0)
  counts[:, :, Q] = ok.sum(axis=0)
  return dict(bins=bins, extra=extra, pinball=pinball, counts=counts, invalid=int((~ok).sum()), fields=fields,
              abs_bins=abs_bins, abs_extra=extra.copy(), abs_pinball=abs_pinball)


def sum_tolerance(ref, G):
  """Per sum: (G + 8) 2^-53 sum |term|.  w alpha is the same double product on both sides, so only the order of the G
  additions of a column differs between the device and the reference."""
  f = (G + 8) * 2.0 ** -53
  return dict(bins=f * ref["abs_bins"], extra=f * ref["abs_extra"], pinball=f * ref["abs_pinball"])


def scores(ref, M):
  """reliability, crps_potential, crps_ensemble [B, C] from the reference sums, as the issue writes them."""
  a, b = ref["bins"][..., 0], ref["bins"][..., 1]
  s0, olo, ohi = ref["extra"][..., 0], ref["extra"][..., 1], ref["extra"][..., 2]
  p = np.arange(M + 1) / float(M)
  with np.errstate(divide="ignore", invalid="ignore"):
    g = (a + b) / s0[..., None]
    o = np.where(a + b != 0.0, b / (a + b), 0.0)
    g[..., 0] = np.where(olo != 0.0, b[..., 0] / olo, 0.0)
    g[..., M] = np.where(ohi != 0.0, a[..., M] / ohi, 0.0)
    o[..., 0] = olo / s0
    o[..., M] = 1.0 - ohi / s0
  return dict(reliability=(g * (o - p) ** 2).sum(-1), crps_potential=(g * o * (1.0 - o)).sum(-1),
              crps_ensemble=((a * p ** 2 + b * (1.0 - p) ** 2).sum(-1)) / s0, bin_width=g, bin_frequency=o)


def crps_pairwise(members, truth, w):
  """[B, C]: sum w (mean_i |x_i - y| - sum_{i,j} |x_i - x_j| / (2 M^2)) / sum w over the counted points, in float64."""
  members, truth = np.asarray(members, np.float32), np.asarray(truth, np.float32)
  M = members.shape[0]
  ok = np.isfinite(members).all(axis=0) & np.isfinite(truth)
  x = np.where(ok[None], members, np.float32(0.0)).astype(np.float64)
  y = np.where(ok, truth, np.float32(0.0)).astype(np.float64)
  ae = np.abs(x - y[None]).mean(axis=0)
  d = np.zeros_like(y)
  for i in range(M):
    d += np.abs(x[i][None] - x).sum(axis=0)
  wk = np.asarray(w, np.float32).astype(np.float64)[:, None, None] * ok
  return (wk * (ae - d / (2.0 * M * M))).sum(axis=0) / wk.sum(axis=0)
