"""The definition of the score maps (include/gencast_hip.h gc_ens_map_*) in NumPy float64: explicit
loops over the members in the stated orders, NumPy only vectorises over the points.  No `np.sum` over members or dates: its
pairwise order is not the definition's.

Test infrastructure only (the product never imports it).  `members` [M, G, B, C] and `truth` [G, B, C] are float32 (the
device's inputs).  A point counts when the truth and all M members are finite there.  Per counted point, every operation a
rounded float64 operation:
  m  = (sum_i x_i) / M                                 i ascending (slot order)
  s2 = (sum_i (x_i - m) (x_i - m)) / (M - 1)           the same order
  e  = m - y
  with the members sorted ascending:
  ae = (sum_k |x_(k) - y|) / M                         k ascending
  d  = (sum_{k=1}^{M-1} (k (M - k)) (x_(k) - x_(k-1))) / (M (M - 1) / 2)      k ascending (the gap form)
  c  = ae - 0.5 d
  r  = #{i : x_i < y}                                  on the float32 values; a member equal to y is not below it
Planes of a slot, per point, date after date (a left fold from zero):
  P0 += e  P1 += e e  P2 += s2  P3 += ae  P4 += d  P5 += c c      N0 += 1  N1 += [r == 0]  N2 += [r == M]
Event planes from the code bytes (k | o << 7, 255 = not counted):  E0 += 1  E1 += k  E2 += k k  E3 += k o  E4 += o
"""
import numpy as np


def gap_sum(xs):
  """sum_{k=1}^{M-1} (k (M - k)) (x_(k) - x_(k-1)) over axis 0 of SORTED float64 values, ascending k."""
  M = xs.shape[0]
  out = np.zeros(xs.shape[1:])
  for k in range(1, M):
    out = out + float(k * (M - k)) * (xs[k] - xs[k - 1])
  return out


def point_terms(members, truth, dtype=np.float32):
  """dict(counted, e, s2, ae, d, c, r) per point [G, B, C]; the float terms are float64 and meaningless where not counted.
  `dtype`: what the inputs are taken as -- float32, the device's; float64 for values that were mapped to other units on the
  host (a yardstick with a bound, not with equal bytes)."""
  members = np.asarray(members, dtype=dtype)
  truth = np.asarray(truth, dtype=dtype)
  M = members.shape[0]
  counted = np.isfinite(truth)
  for i in range(M):
    counted = counted & np.isfinite(members[i])
  x = np.where(counted[None], members, dtype(0.0)).astype(np.float64)     # (finite everywhere: no warnings, same values)
  y = np.where(counted, truth, dtype(0.0)).astype(np.float64)
  s = np.zeros(truth.shape)
  for i in range(M):
    s = s + x[i]
  m = s / float(M)
  s2 = np.zeros(truth.shape)
  for i in range(M):
    dx = x[i] - m
    s2 = s2 + dx * dx
  s2 = s2 / (float(M) - 1.0)
  e = m - y
  xs = np.sort(x, axis=0)
  ae = np.zeros(truth.shape)
  for k in range(M):
    ae = ae + np.abs(xs[k] - y)
  ae = ae / float(M)
  d = gap_sum(xs) / float(M * (M - 1) // 2)
  c = ae - 0.5 * d
  r = np.zeros(truth.shape, np.int64)
  for i in range(M):
    r += (members[i] < truth) & counted
  return dict(counted=counted, e=e, s2=s2, ae=ae, d=d, c=c, r=r)


def empty(G, B, C):
  """(sums [6, G, B, C] float64, counts [3, G, B, C] uint32): a slot nothing was added into."""
  return np.zeros((6, G, B, C)), np.zeros((3, G, B, C), np.uint32)


def accumulate(sums, counts, members, truth, channels=None):
  """One date into the planes, in place; -> the selected points that did not count."""
  members, truth = np.asarray(members, np.float32), np.asarray(truth, np.float32)
  if channels is not None:
    members, truth = members[..., list(channels)], truth[..., list(channels)]
  M = members.shape[0]
  t = point_terms(members, truth)
  ok = t["counted"]
  for k, term in enumerate((t["e"], t["e"] * t["e"], t["s2"], t["ae"], t["d"], t["c"] * t["c"])):
    sums[k] = np.where(ok, sums[k] + term, sums[k])
  counts[0] += ok
  counts[1] += ok & (t["r"] == 0)
  counts[2] += ok & (t["r"] == M)
  return int((~ok).sum())


def reference(dates, channels=None):
  """`dates`: [(members, truth), ..] in call order -> (sums, counts, [invalid of each date])."""
  _, G, B, C = np.asarray(dates[0][0]).shape
  sums, counts = empty(G, B, C if channels is None else len(channels))
  invalid = [accumulate(sums, counts, m, y, channels) for m, y in dates]
  return sums, counts, invalid


def accumulate_events(events, code, channels=None):
  """One date's code bytes [T, G, B, C] uint8 into the event planes [T, 5, G, B, C'] uint32, in place."""
  code = np.asarray(code, np.uint8)
  if channels is not None:
    code = code[..., list(channels)]
  ok = code != 255
  k = np.where(ok, code & 127, 0).astype(np.uint32)
  o = np.where(ok, code >> 7, 0).astype(np.uint32)
  events[:, 0] += ok
  events[:, 1] += k
  events[:, 2] += k * k
  events[:, 3] += k * o
  events[:, 4] += o
