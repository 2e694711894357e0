"""The definition of gc_ens_clim_score (include/gencast_hip.h) restated in float64, with plain loops
over the members and over the pairs.  The slot-order sums (m, cbar, ae, q_x) are formed in the order the definition
prescribes, so on either side they are the same IEEE double operations; the mean absolute difference d is formed the long
way, over all pairs -- the device forms it from the gaps of the sorted sample, which differs in rounding only.

`reference` returns, per (batch, channel), the twelve sums in the order of the header, the sum of the ABSOLUTE values of
the same terms (`abs`: what the error bound is relative to), the counted points and the points not counted."""
import numpy as np

NAMES = ("A0", "A1", "A2", "A3", "A4", "A5", "A6", "A7", "F4", "F5", "C4", "C5")


def slot_mean(x):
  """(sum_i x_i) / n over axis 0 in ascending slot order, in double."""
  s = np.zeros(x.shape[1:], np.float64)
  for i in range(x.shape[0]):
    s = s + x[i].astype(np.float64)
  return s / float(x.shape[0])


def mean_abs_error(x, y):
  s = np.zeros(x.shape[1:], np.float64)
  for i in range(x.shape[0]):
    s = s + np.abs(x[i].astype(np.float64) - y)
  return s / float(x.shape[0])


def pair_form(x):
  """The mean of |x_i - x_j| over the n (n - 1) / 2 pairs i < j of axis 0."""
  n = x.shape[0]
  xd = x.astype(np.float64)
  s, t = np.zeros(x.shape[1:], np.float64), np.empty(x.shape[1:], np.float64)
  for i in range(n):
    for j in range(i + 1, n):
      np.subtract(xd[i], xd[j], out=t)
      np.abs(t, out=t)
      s += t
  return s / (0.5 * n * (n - 1.0))


def gap_form(x):
  """The same number from the sorted sample: sum_k k (n - k) (x_(k+1) - x_(k)) over the n - 1 gaps, every term >= 0."""
  n = x.shape[0]
  v = np.sort(x, axis=0)
  s = np.zeros(x.shape[1:], np.float64)
  for k in range(1, n):
    s = s + float(k * (n - k)) * (v[k].astype(np.float64) - v[k - 1].astype(np.float64))
  return s / (0.5 * n * (n - 1.0))


def reference(members, clim, truth, w, d=pair_form):
  """members [M, G, B, C], clim [K, G, B, C], truth [G, B, C] float32, w [G] -> {"sums", "abs": [B, C, 12] float64,
  "counts": [B, C] uint64, "invalid": int}."""
  members, clim, truth = (np.asarray(a, np.float32) for a in (members, clim, truth))
  M, K = members.shape[0], clim.shape[0]
  valid = np.isfinite(truth) & np.isfinite(members).all(axis=0) & np.isfinite(clim).all(axis=0)
  # a point that is not counted adds nothing: its values are replaced by zeros so that no NaN is formed on the way
  x = np.where(valid[None], members, np.float32(0.0))
  c = np.where(valid[None], clim, np.float32(0.0))
  y = np.where(valid, truth, np.float32(0.0)).astype(np.float64)
  m, cbar = slot_mean(x), slot_mean(c)
  fa, oa, e = m - cbar, y - cbar, m - y
  q_x = np.zeros(y.shape, np.float64)
  for i in range(M):
    dx = x[i].astype(np.float64) - cbar
    q_x = q_x + dx * dx
  q_x = q_x / float(M)
  terms = [np.ones(y.shape), fa, oa, fa * oa, fa * fa, oa * oa, q_x, e * e, mean_abs_error(x, y), d(x), mean_abs_error(c, y),
           d(c)]
  wd = np.asarray(w, np.float32).astype(np.float64)[:, None, None]
  keep = valid.astype(np.float64)
  sums = np.stack([(wd * t * keep).sum(axis=0) for t in terms], axis=-1)
  mags = np.stack([(wd * np.abs(t) * keep).sum(axis=0) for t in terms], axis=-1)
  return {"sums": sums, "abs": mags, "counts": valid.sum(axis=0).astype(np.uint64), "invalid": int((~valid).sum()),
          "n_members": M, "n_climatology": K}


def tolerance(ref, G):
  """|device - reference| <= (G + max(M, K)^2 + 8) 2^-53 sum |term| per sum: the bound of DESIGN.md section 8c, carried over."""
  n = max(ref["n_members"], ref["n_climatology"])
  return (G + n * n + 8) * 2.0 ** -53 * ref["abs"]


def scores(ref):
  """The derived lines, written out from the sums (a zero denominator: NaN)."""
  s = {n: ref["sums"][..., k] for k, n in enumerate(NAMES)}
  M, K = float(ref["n_members"]), float(ref["n_climatology"])
  with np.errstate(invalid="ignore", divide="ignore"):
    mf, mo = s["A1"] / s["A0"], s["A2"] / s["A0"]
    crps = (s["F4"] - 0.5 * s["F5"]) / s["A0"]
    crps_c = (s["C4"] - 0.5 * s["C5"]) / s["A0"]
    crps_e = (s["F4"] - 0.5 * (M - 1.0) / M * s["F5"]) / s["A0"]
    crps_ce = (s["C4"] - 0.5 * (K - 1.0) / K * s["C5"]) / s["A0"]
    out = {"acc": s["A3"] / np.sqrt(s["A4"] * s["A5"]),
           "acc_centred": (s["A3"] / s["A0"] - mf * mo) / np.sqrt((s["A4"] / s["A0"] - mf * mf) * (s["A5"] / s["A0"] - mo * mo)),
           "acc_members": s["A3"] / np.sqrt(s["A6"] * s["A5"]),
           "crps": crps, "crps_climatology": crps_c, "crpss": 1.0 - crps / crps_c,
           "crps_ensemble": crps_e, "crps_climatology_ensemble": crps_ce, "crpss_ensemble": 1.0 - crps_e / crps_ce,
           "msss": 1.0 - s["A7"] / s["A5"], "rmse": np.sqrt(s["A7"] / s["A0"]), "rmse_climatology": np.sqrt(s["A5"] / s["A0"])}
  return {k: np.where(np.isfinite(v), v, np.nan) for k, v in out.items()}
