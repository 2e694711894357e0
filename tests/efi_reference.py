"""The Extreme Forecast Index of gc_ens_efi_score, restated in NumPy float64 -- the yardstick of
tests/test_efi.py, tests/test_gpu_efi.py and tests/test_gpu_efi_rollout.py.

Per point, from the float32 members x_0 .. x_{M-1}, the samples c_0 .. c_{K-1} and the truth y:
  le(v) = #{j : c_j <= v}     lt(v) = #{j : c_j < v}            comparisons on the float32 values
  f = (sum_i (a[le(x_i)] + a[lt(x_i)])) / M                     i ascending, in double
  o = a[le(y)] + a[lt(y)]
with a = verification.efi_table(K).  These are the device's operations one for one (comparisons, integer counts, lookups,
double additions in slot order, one division), so the fields are compared with ==.

Tolerance of the six column sums: the bound of section 8c, carried over.  Both sides hold identical per-point doubles
w, w f, w o, w (f o), w (f f), w (o o); only the order of the G additions of a column differs, so
  |device - reference| <= (G + 8) 2^-53 sum |term|.
It is derived, not tuned."""
import numpy as np

from gencast_flax_nnx_amd.verification import efi_table

NAMES = ("S0", "S1", "S2", "S3", "S4", "S5")


def ranks_of(values, clim):
  """(le, lt) of `values` [...] in the samples `clim` [K, ...]: integer counts, the samples in slot order."""
  le = np.zeros(values.shape, np.int64)
  lt = np.zeros(values.shape, np.int64)
  for j in range(clim.shape[0]):
    le += clim[j] <= values
    lt += clim[j] < values
  return le, lt


def efi_field(members, clim, table=None):
  """-> (f [G, B, C] float64, finite [G, B, C]): the index of every point in double, and where members and samples are all
  finite (f is meaningless elsewhere)."""
  members, clim = np.asarray(members, np.float32), np.asarray(clim, np.float32)
  M, K = members.shape[0], clim.shape[0]
  a = efi_table(K) if table is None else np.asarray(table, np.float64)
  acc = np.zeros(members.shape[1:], np.float64)
  with np.errstate(invalid="ignore"):
    for i in range(M):                                       # slot order
      le, lt = ranks_of(members[i], clim)
      acc = acc + (a[np.minimum(le, K)] + a[np.minimum(lt, K)])
  finite = np.isfinite(members).all(0) & np.isfinite(clim).all(0)
  return acc / float(M), finite


def reference(members, clim, truth, w, ranks=(), directions=(), n_bins=20, wq=None, table=None):
  """Everything gc_ens_efi_score returns, and both fields.  members [M, G, B, C], clim [K, G, B, C], truth [G, B, C]
  float32; w [G]; wq [G] uint32 (needed with events).  `abs`: sum |term| of every sum, for `tolerance`."""
  members, clim, truth = (np.asarray(x, np.float32) for x in (members, clim, truth))
  K = clim.shape[0]
  G, B, C = truth.shape
  a = efi_table(K) if table is None else np.asarray(table, np.float64)
  f, finite = efi_field(members, clim, a)
  valid = finite & np.isfinite(truth)
  with np.errstate(invalid="ignore"):
    le_y, lt_y = ranks_of(truth, clim)
  o = a[np.minimum(le_y, K)] + a[np.minimum(lt_y, K)]
  efi32 = np.where(valid, f, np.nan).astype(np.float32)
  obs32 = np.where(valid, o, np.nan).astype(np.float32)
  wd = np.asarray(w, np.float32).astype(np.float64)[:, None, None]
  terms = np.stack([np.broadcast_to(wd, f.shape), wd * f, wd * o, wd * (f * o), wd * (f * f), wd * (o * o)], axis=-1)
  terms = np.where(valid[..., None], terms, 0.0)
  sums = np.zeros((B, C, 6))
  for g in range(G):                                         # ascending node order
    sums += terms[g]
  T, E = len(ranks), int(n_bins)
  weighted = np.zeros((T, B, C, 2, E), np.uint64)
  counts = np.zeros((T, B, C, 2, E), np.uint64)
  e = np.minimum(E - 1, ((np.where(valid, f, 0.0) + 1.0) * (0.5 * E)).astype(np.int64))
  g, b, c = np.nonzero(valid)
  for t in range(T):
    inside = ((lt_y >= ranks[t]) if directions[t] > 0 else (le_y <= ranks[t])).astype(np.int64)
    np.add.at(weighted[t], (b, c, inside[g, b, c], e[g, b, c]), np.asarray(wq, np.uint64)[g])    # one point after the other
    np.add.at(counts[t], (b, c, inside[g, b, c], e[g, b, c]), np.uint64(1))
  return {"efi": efi32, "observed": obs32, "efi64": np.where(valid, f, np.nan), "observed64": np.where(valid, o, np.nan),
          "valid": valid, "le_y": le_y, "lt_y": lt_y, "sums": sums, "abs": np.abs(terms).sum(0), "weighted": weighted,
          "counts": counts, "invalid": int((~valid).sum())}


def fields_only(members, clim, table=None):
  """The EFI field of gc_ens_efi_fields (no truth): float32, NaN where a member or a sample is not finite."""
  f, finite = efi_field(members, clim, table)
  return np.where(finite, f, np.nan).astype(np.float32)


def tolerance(ref, G):
  """[B, C, 6]: (G + 8) 2^-53 sum |term| per sum."""
  return (G + 8) * 2.0 ** -53 * ref["abs"]


def quadrature(members, clim, n=20000):
  """(2 / pi) int_0^1 (p - F_f(p)) / sqrt(p (1 - p)) dp for ONE point (members [M], clim [K]) by the midpoint rule with n
  points: the climate quantile function is the empirical one, q(p) = c_(ceil(p K)) of the sorted samples, and F_f(p) is the
  fraction of the members below q(p), ties counted half: (#{x_i < q} + #{x_i <= q}) / (2 M).  The integrand has an
  inverse-square-root singularity at both ends, which is what limits the rule to 3-4 digits."""
  x, c = np.asarray(members, np.float64), np.sort(np.asarray(clim, np.float64))
  K = c.shape[0]
  p = (np.arange(n) + 0.5) / n
  q = c[np.minimum(K - 1, np.ceil(p * K).astype(np.int64) - 1)]          # the empirical quantile of the samples at p
  F = ((x[:, None] < q[None, :]).mean(0) + (x[:, None] <= q[None, :]).mean(0)) / 2.0   # ties counted half
  return float((2.0 / np.pi) * np.mean((p - F) / np.sqrt(p * (1.0 - p))))
