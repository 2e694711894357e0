"""The definition of the fractions sums (include/gencast_hip.h, gc_ens_fss_*), restated twice.  Test
infrastructure: the product never imports it.

Inputs: the code bytes code [n_lat, n_lon] of one column (b, c) and one threshold -- a point COUNTS iff code != 255, there
k = code & 127 and o = code >> 7 -- the member count M, the integer node weights wq [G], and one scale of the plan: r_lat >= 0,
r_lon [n_lat] in 0 .. (n_lon - 1) / 2, integer row weights row_wq [n_lat] in 1 .. 2^24 - 1.  Win(i, j) is the window of
gc_ens_derive: latitude clipped, longitude wrapping, a row's width that of the row i'.  Per counted centre p = (i, j), over the
counted q in Win(p), in integers:
  A = sum row_wq[i'] k(q),   B = sum row_wq[i'] o(q),   N = sum row_wq[i']
then in double, each operation rounded once:  P = (double) A / ((double) M (double) N),  O = (double) B / (double) N,
and with w = (double) wq[g] four sums over the counted centres:
  w ((P - O)(P - O)),   w (P P + O O),   w P,   w O.

`literal`: window point by window point, Python integers, the float64 terms summed by math.fsum.
`separable`: a row pass and a column pass over whole arrays of columns (NumPy int64: A, B, N < 2^51), the same P and O to the
bit; it is what the device tests compare with, and tests/test_fss.py holds it to `literal`."""
import math

import numpy as np


def literal(code, M, r_lat, r_lon, row_wq, wq):
  """code [n_lat, n_lon] uint8 -> dict(A, B, N: int arrays (object), P, O: float64 [n_lat, n_lon] (NaN where the point does not
  count), sums: four floats)."""
  code = np.asarray(code, np.uint8)
  n_lat, n_lon = code.shape
  A = np.zeros((n_lat, n_lon), object)
  B = np.zeros((n_lat, n_lon), object)
  N = np.zeros((n_lat, n_lon), object)
  P = np.full((n_lat, n_lon), np.nan)
  O = np.full((n_lat, n_lon), np.nan)
  terms = [[], [], [], []]
  for i in range(n_lat):
    for j in range(n_lon):
      if code[i, j] == 255:
        continue
      a = b = n = 0
      for ii in range(max(0, i - int(r_lat)), min(n_lat - 1, i + int(r_lat)) + 1):
        for d in range(-int(r_lon[ii]), int(r_lon[ii]) + 1):
          c = int(code[ii, (j + d) % n_lon])
          if c != 255:
            a += int(row_wq[ii]) * (c & 127)
            b += int(row_wq[ii]) * (c >> 7)
            n += int(row_wq[ii])
      A[i, j], B[i, j], N[i, j] = a, b, n
      p = float(a) / (float(M) * float(n))
      o = float(b) / float(n)
      P[i, j], O[i, j] = p, o
      w = float(int(wq[i * n_lon + j]))
      terms[0].append(w * ((p - o) * (p - o)))
      terms[1].append(w * (p * p + o * o))
      terms[2].append(w * p)
      terms[3].append(w * o)
  return dict(A=A, B=B, N=N, P=P, O=O, sums=[math.fsum(t) for t in terms])


def point_fields(code, M, n_lat, n_lon, r_lat, r_lon, row_wq):
  """The row pass and the column pass.  code [G, ...] uint8 (any trailing axes: columns) -> (valid, A, B, N int64, P, O
  float64), each [G, ...]; P and O NaN where the point does not count."""
  code = np.asarray(code, np.uint8)
  grid = code.reshape((n_lat, n_lon) + code.shape[1:])
  valid = grid != 255
  fields = [np.where(valid, grid & 127, 0).astype(np.int64), np.where(valid, grid >> 7, 0).astype(np.int64),
            valid.astype(np.int64)]
  rows = [np.zeros_like(f) for f in fields]                 # row pass: the window of row i' along its own longitude
  for ii in range(n_lat):
    for d in range(-int(r_lon[ii]), int(r_lon[ii]) + 1):
      for f, r in zip(fields, rows):
        r[ii] += np.roll(f[ii], -d, axis=0)
  out = [np.zeros_like(f) for f in fields]                  # column pass: the rows above and below, weighted
  for i in range(n_lat):
    for ii in range(max(0, i - int(r_lat)), min(n_lat - 1, i + int(r_lat)) + 1):
      for r, acc in zip(rows, out):
        acc[i] += int(row_wq[ii]) * r[ii]
  A, B, N = (a.reshape(code.shape) for a in out)
  valid = valid.reshape(code.shape)
  assert int(max(A.max(), B.max(), N.max())) < 2 ** 51
  with np.errstate(invalid="ignore", divide="ignore"):
    P = np.where(valid, A.astype(np.float64) / (np.float64(M) * N.astype(np.float64)), np.nan)
    O = np.where(valid, B.astype(np.float64) / N.astype(np.float64), np.nan)
  return valid, A, B, N, P, O


def column_sums(valid, P, O, wq):
  """valid, P, O [G, ...], wq [G] -> sums [..., 4] float64, every sum by math.fsum over the counted centres."""
  w = np.asarray(wq).astype(np.float64).reshape((-1,) + (1,) * (P.ndim - 1))
  with np.errstate(invalid="ignore"):
    terms = np.stack([w * ((P - O) * (P - O)), w * (P * P + O * O), w * P, w * O], axis=-1)
  terms = np.where(valid[..., None], terms, 0.0)            # (a zero adds nothing to an exact sum)
  flat = terms.reshape(terms.shape[0], -1)
  return np.array([math.fsum(flat[:, e]) for e in range(flat.shape[1])]).reshape(terms.shape[1:])


def separable(code, M, n_lat, n_lon, r_lats, r_lons, row_wq, wq):
  """code [T, G, B, C] uint8; r_lats [S]; r_lons [S, n_lat] -> dict(sums [T, S, B, C, 4], prob, obs [T, S, G, B, C] float32)."""
  code = np.asarray(code, np.uint8)
  T, S = code.shape[0], len(r_lats)
  sums = np.zeros((T, S) + code.shape[2:] + (4,))
  prob = np.zeros((T, S) + code.shape[1:], np.float32)
  obs = np.zeros((T, S) + code.shape[1:], np.float32)
  for t in range(T):
    for s in range(S):
      valid, _, _, _, P, O = point_fields(code[t], M, n_lat, n_lon, r_lats[s], r_lons[s], row_wq)
      sums[t, s] = column_sums(valid, P, O, wq)
      prob[t, s], obs[t, s] = P.astype(np.float32), O.astype(np.float32)
  return dict(sums=sums, prob=prob, obs=obs)


def bound(ref, G):
  """|got - ref| <= G 2^-53 ref + spacing(ref): a sum of at most G non-negative doubles added in any order, against the
  correctly rounded sum."""
  ref = np.asarray(ref, np.float64)
  return G * 2.0 ** -53 * ref + np.spacing(ref)


def scores(sums, weight):
  """Every derived score, formula by formula: sums [T, S, B, C, 4], weight [T, B, C] (in the units of the sums)."""
  def div(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64))
    out = np.full(a.shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out
  W = np.asarray(weight, np.float64)[:, None]
  f0 = div(sums[..., 3], W)
  return dict(fss=1.0 - div(sums[..., 0], sums[..., 1]), fbs=div(sums[..., 0], W), forecast_fraction=div(sums[..., 2], W),
              observed_fraction=f0, fss_uniform=0.5 + f0 / 2.0, frequency_bias=div(sums[..., 2], sums[..., 3]))


def displacement_codes(n_lat, n_lon, M, shift):
  """Per row the truth in the event at one point, all M members in it `shift` columns east: code [n_lat, n_lon]."""
  code = np.zeros((n_lat, n_lon), np.uint8)
  for i in range(n_lat):
    j0 = (5 * i) % n_lon
    code[i, j0] |= 128
    code[i, (j0 + shift) % n_lon] |= M
  return code


def random_codes(n_lat, n_lon, M, seed):
  """k ~ Binomial(M, 0.2), o ~ Bernoulli(0.2), one non-counted row and ten scattered non-counted points."""
  rng = np.random.default_rng(seed)
  k = rng.binomial(M, 0.2, (n_lat, n_lon)).astype(np.uint8)
  o = (rng.random((n_lat, n_lon)) < 0.2).astype(np.uint8)
  code = k | (o << 7)
  code[4, :] = 255
  code[rng.integers(0, n_lat, 10), rng.integers(0, n_lon, 10)] = 255
  return code
