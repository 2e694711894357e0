"""The definition of the ensemble event tables (include/gencast_hip.h, gc_ens_event_*), restated
literally: loops over thresholds, members and bins, NumPy over the points only, integer sums.  Test infrastructure: the
product never imports it.  Below the tables, the derived scores, formula by formula."""
import numpy as np

U32_MAX = 2 ** 32 - 1


def quantize(w):
  """(wq uint32, scale): scale = 2^e, e the largest integer with max(w) 2^e <= 2^32 - 1 (found by search), wq = rint(w scale)."""
  w = np.asarray(w, dtype=np.float64)
  top = float(w.max())
  e = -1100
  while top * 2.0 ** (e + 1) <= U32_MAX:                   # (times a power of two: exact)
    e += 1
  scale = 2.0 ** e
  return np.rint(w * scale).astype(np.uint32), scale


def in_event(v, thr, direction):
  """Strict, on the float32 values."""
  v, thr = np.asarray(v, np.float32), np.asarray(thr, np.float32)
  with np.errstate(invalid="ignore"):
    return v > thr if direction > 0 else v < thr


def tables(members, truth, thresholds, directions, wq):
  """members [M, G, B, C], truth [G, B, C], thresholds [T, G, B, C] float32, wq [G] uint32 ->
  weighted, counts [T, B, C, 2, M + 1] uint64; invalid [T] uint64; code [T, G, B, C] uint8."""
  members, truth, thresholds = (np.asarray(a, np.float32) for a in (members, truth, thresholds))
  M, G, B, C = members.shape
  T = thresholds.shape[0]
  wq = np.asarray(wq).astype(np.uint64)
  weighted = np.zeros((T, B, C, 2, M + 1), np.uint64)
  counts = np.zeros((T, B, C, 2, M + 1), np.uint64)
  invalid = np.zeros(T, np.uint64)
  code = np.zeros((T, G, B, C), np.uint8)
  finite = np.isfinite(truth)
  for i in range(M):
    finite &= np.isfinite(members[i])
  for t in range(T):
    valid = finite & np.isfinite(thresholds[t])
    k = np.zeros((G, B, C), np.int64)
    for i in range(M):
      k += in_event(members[i], thresholds[t], directions[t])
    o = in_event(truth, thresholds[t], directions[t]).astype(np.int64)
    code[t] = np.where(valid, k | (o << 7), 255).astype(np.uint8)
    invalid[t] = np.uint64(int((~valid).sum()))
    for oo in (0, 1):
      for kk in range(M + 1):
        hit = valid & (o == oo) & (k == kk)                # [G, B, C]
        counts[t, :, :, oo, kk] = hit.sum(axis=0).astype(np.uint64)
        weighted[t, :, :, oo, kk] = (hit.astype(np.uint64) * wq[:, None, None]).sum(axis=0, dtype=np.uint64)
  return dict(weighted=weighted, counts=counts, invalid=invalid, code=code)


def _div(a, b):
  a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
  out = np.full(a.shape, np.nan)
  np.divide(a, b, out=out, where=b != 0)
  return out


def scores(weighted, scale, M, alphas=(0.05, 0.2, 0.5, 0.9)):
  """Every derived score from the table, bin by bin: {name: [T, B, C] (+ a trailing axis for curves)}."""
  weighted = np.asarray(weighted, np.uint64)
  n = [(weighted[..., 0, k] + weighted[..., 1, k]).astype(np.float64) / scale for k in range(M + 1)]
  o = [weighted[..., 1, k].astype(np.float64) / scale for k in range(M + 1)]
  p = [k / M for k in range(M + 1)]
  N, O = sum(n), sum(o)
  s = _div(O, N)
  brier = _div(sum((n[k] - o[k]) * p[k] ** 2 + o[k] * (1.0 - p[k]) ** 2 for k in range(M + 1)), N)
  fair = brier - _div(sum(n[k] * (k * (M - k) / (M * M * (M - 1.0))) for k in range(M + 1)), N)
  rel = np.zeros_like(N)
  res = np.zeros_like(N)
  for k in range(M + 1):
    ob = np.where(n[k] > 0, _div(o[k], n[k]), 0.0)
    rel = rel + n[k] * (p[k] - ob) ** 2
    res = res + np.where(n[k] > 0, n[k] * (ob - s) ** 2, 0.0)
  rel, res = _div(rel, N), _div(res, N)
  unc = s * (1.0 - s)
  H = [sum(o[k] for k in range(j, M + 1)) if j <= M else np.zeros_like(N) for j in range(M + 2)]
  F = [sum(n[k] - o[k] for k in range(j, M + 1)) if j <= M else np.zeros_like(N) for j in range(M + 2)]
  hr = np.stack([_div(H[j], O) for j in range(M + 2)], axis=-1)
  far = np.stack([_div(F[j], N - O) for j in range(M + 2)], axis=-1)
  roc = sum(0.5 * (far[..., j] - far[..., j + 1]) * (hr[..., j] + hr[..., j + 1]) for j in range(M + 1))
  value = []
  for a in alphas:
    e_clim, e_perf = np.minimum(a, s), a * s
    best = None
    for j in range(M + 2):
      e = _div(a * (H[j] + F[j]), N) + _div(O - H[j], N)
      v = _div(e_clim - e, e_clim - e_perf)
      best = v if best is None else np.where(np.isnan(v) | np.isnan(best), np.nan, np.maximum(best, v))
    value.append(best)
  return dict(base_rate=s, brier=brier, brier_fair=fair, reliability=rel, resolution=res, uncertainty=unc,
              brier_skill=1.0 - _div(brier, unc), hit_rate=hr, false_alarm_rate=far, roc_area=roc,
              economic_value=np.stack(value, axis=-1), valid_weight=N)


def brier_direct(members, truth, thresholds, directions, w):
  """The weighted mean of (k / M - o)^2 over the valid points, straight from the fields: [T, B, C] float64."""
  members, truth, thresholds = (np.asarray(a, np.float32) for a in (members, truth, thresholds))
  M = members.shape[0]
  w = np.asarray(w, np.float64)[:, None, None]
  finite = np.isfinite(truth) & np.isfinite(members).all(axis=0)
  out = []
  for t in range(thresholds.shape[0]):
    valid = finite & np.isfinite(thresholds[t])
    k = sum(in_event(members[i], thresholds[t], directions[t]).astype(np.float64) for i in range(M))
    o = in_event(truth, thresholds[t], directions[t]).astype(np.float64)
    out.append(_div((np.where(valid, w * (k / M - o) ** 2, 0.0)).sum(axis=0), np.where(valid, w, 0.0).sum(axis=0)))
  return np.stack(out)


LEVELS = np.array([0.0, 1.3, -1.3, 2.3, 0.6, -0.6, -2.3, 0.0])
DIRECTIONS = np.array([1, 1, -1, 1, -1, 1, -1, -1], np.int32)


def data(M, G, B, C, seed, T=4):
  """Members that share a signal with the truth, so that every bin fills: x_i = (s + e_i) / sqrt 2, y = (s + e_0) / sqrt 2,
  times a per-channel scale; weights uniform(0.1, 2) with a few exact zeros; thresholds LEVELS[:T] x scale with
  DIRECTIONS[:T] (the first four: {0, +1.3, -1.3 (below), +2.3})."""
  rng = np.random.default_rng(seed)
  scale = np.logspace(-3, 5, C)
  s = rng.standard_normal((G, B, C))
  members = ((s[None] + rng.standard_normal((M, G, B, C))) / np.sqrt(2.0) * scale).astype(np.float32)
  truth = ((s + rng.standard_normal((G, B, C))) / np.sqrt(2.0) * scale).astype(np.float32)
  w = rng.uniform(0.1, 2.0, G).astype(np.float32)
  w[[1, G // 3, G - 2]] = 0.0
  thresholds = np.broadcast_to((LEVELS[:T, None] * scale[None, :])[:, None, None, :], (T, G, B, C)).astype(np.float32)
  return members, truth, w, np.ascontiguousarray(thresholds), DIRECTIONS[:T].copy()


def every_bin_is_reached(weighted):
  """Bins k = 0 and k = M and both rows o hold something, for every threshold (summed over the columns)."""
  tot = np.asarray(weighted).sum(axis=(1, 2))              # [T, 2, M + 1]
  return bool((tot[:, :, 0].sum(axis=1) > 0).all() and (tot[:, :, -1].sum(axis=1) > 0).all()
              and (tot.sum(axis=2) > 0).all())
