"""The definition of gc_ens_window_emit (include/gencast_hip.h) restated in NumPy float64: the same
IEEE operations in the same order, so the device is held to it bit for bit (only a NaN's payload is free).

`stack` [L, ...] float32: the values of the last L pushes, oldest first; every trailing axis is elementwise."""
import numpy as np

LINEAR, MAX, MIN = 0, 1, 2


def coefficients(kind: str, steps: int, coef=None):
  """(device kind, a [steps] float64 or None) of a `WindowSpec` kind, written out independently of the package."""
  if kind == "sum":
    return LINEAR, np.ones(steps)
  if kind == "mean":
    return LINEAR, np.full(steps, 1.0 / steps)
  if kind == "change":
    a = np.zeros(steps)
    a[0] = -1.0
    a[steps - 1] = 1.0
    return LINEAR, a
  if kind == "linear":
    return LINEAR, np.asarray(coef, np.float64)
  return {"max": MAX, "min": MIN}[kind], None


def window(stack, kind: int, coef=None) -> np.ndarray:
  """float32 [...]: the window over axis 0 of `stack` [L, ...] float32."""
  x = np.asarray(stack)
  assert x.dtype == np.float32 and x.shape[0] >= 1
  L = x.shape[0]
  bad = ~np.isfinite(x).all(axis=0)
  with np.errstate(all="ignore"):
    if kind == LINEAR:
      a = np.asarray(coef, np.float64)
      assert a.shape == (L,)
      acc = np.zeros(x.shape[1:], np.float64)
      for t in range(L):
        p = a[t] * x[t].astype(np.float64)                 # the product is rounded ...
        acc = acc + p                                      # ... then the sum
      out = acc.astype(np.float32)                         # rounded once; beyond float32 range: +-inf
    else:
      out = x[0].copy()
      for t in range(1, L):                                # the strict comparison keeps the older value on a tie
        out = np.where(x[t] > out if kind == MAX else x[t] < out, x[t], out)
  out = out.astype(np.float32, copy=True)
  out[bad] = np.nan
  return out


def last(pushes, L: int) -> np.ndarray:
  """[L, ...]: the last L entries of a sequence of pushed arrays, oldest first."""
  assert len(pushes) >= L
  return np.stack(pushes[len(pushes) - L:])


def same_bits(got, want) -> bool:
  """Bit equality of two float32 arrays, a NaN matching any NaN."""
  got, want = np.asarray(got), np.asarray(want)
  if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
    return False
  gn, wn = np.isnan(got), np.isnan(want)
  return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))
