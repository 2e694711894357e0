"""The host side of the Extreme Forecast Index: the table, the definition of
tests/efi_reference.py against the integral it is the closed form of, `EfiSpec`, `EfiScores` against brute force on small
tables, and the way a `ScoredStore` and the rollout's results carry it.  No device, no library."""
import math

import numpy as np
import pytest

from gencast_flax_nnx_amd import rollout, verification
from gencast_flax_nnx_amd.verification import EfiScores, EfiSpec, EnsembleScores, efi_table, quantize_node_weights
from tests import efi_reference as R
from tests.helpers import RecordingHandle


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", range(2, 65))
def test_the_table_is_antisymmetric_to_the_bit(K):
  a = efi_table(K)
  assert a.shape == (K + 1,) and a.dtype == np.float64
  assert np.array_equal(a[::-1], -a) and a[0] == -0.5 and a[K] == 0.5
  assert np.all(np.diff(a) > 0.0)
  if K % 2 == 0:
    assert a[K // 2] == 0.0 and not np.signbit(a[K // 2])
  # the plain formula, whose argument rounds differently (2 n / K - 1 against (2 n - K) / K): one rounding of an argument
  # below 1, 1.1e-16, times asin' <= sqrt(K) / 2 <= 4 away from the ends, over pi, and three roundings of a value <= 0.5
  np.testing.assert_allclose(a, np.arcsin(2.0 * np.arange(K + 1) / K - 1.0) / np.pi, rtol=0, atol=5e-16)


def test_the_table_rejects_other_sizes():
  for K in (1, 65, 0):
    with pytest.raises(ValueError, match="2..64"):
      efi_table(K)


# ---- the closed form against the integral ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K", [(5, 7), (50, 30), (8, 64)])
def test_the_sum_over_the_members_is_the_integral(M, K):
  """The midpoint rule with n points on an integrand with inverse-square-root singularities at both ends misses the two end
  cells by O(sqrt(1 / n)) each: at n = 20 000 that is 7e-3 times the (2 / pi) in front and the jump of F_f there, |.| <= 1;
  the bound below is that, not a tuned figure."""
  rng = np.random.default_rng(M * K)
  n = 20000
  bound = (2.0 / np.pi) * 2.0 * math.sqrt(1.0 / n)
  for trial in range(4):
    x = rng.standard_normal(M).astype(np.float32) + np.float32(0.5 * trial)
    c = rng.standard_normal(K).astype(np.float32)
    if trial == 3:                                          # ties: members on samples, samples on samples
      x[:2], c[1] = c[:2], c[0]
    f, _ = R.efi_field(x[:, None, None, None], c[:, None, None, None])
    q = R.quadrature(x, c, n)
    print(f"M={M} K={K} trial {trial}: closed form {f.item():+.6f} quadrature {q:+.6f}")
    assert abs(f.item() - q) <= bound


def test_the_extremes_are_exactly_one_and_the_index_is_antisymmetric():
  rng = np.random.default_rng(3)
  for M, K in ((2, 2), (5, 7), (50, 30), (64, 64)):
    c = rng.standard_normal((K, 1, 1, 1)).astype(np.float32)
    above = (c.max() + 1.0 + rng.uniform(0, 1, (M, 1, 1, 1))).astype(np.float32)
    assert R.efi_field(above, c)[0].item() == 1.0 and R.efi_field(-above, -c)[0].item() == -1.0
    x = rng.standard_normal((M, 40, 1, 1)).astype(np.float32)
    cc = np.round(rng.standard_normal((K, 40, 1, 1)) * 2).astype(np.float32) / 2
    x[0] = cc[0]                                            # with ties
    f, g = R.efi_field(x, cc)[0], R.efi_field(-x, -cc)[0]
    assert np.array_equal(f + g, np.zeros_like(f))
    y = x[1]
    ref, neg = (R.reference(s * x, s * cc, s * y, np.ones(40, np.float32)) for s in (np.float32(1), np.float32(-1)))
    assert np.array_equal(ref["observed64"] + neg["observed64"], np.zeros_like(f))


# ---- the spec ---------------------------------------------------------------------------------------------------------------
def test_rank_rounding_where_q_times_k_is_integral():
  spec = EfiSpec()
  assert spec.quantiles == (0.9, 0.1) and spec.directions == (1, -1) and spec.bins == 20 and spec.n_events == 2
  assert 0.28 * 25 > 7.0 and 0.58 * 50 < 29.0               # (products that round off the integer: a bare ceil / floor is one off)
  assert EfiSpec((0.28,), (+1,)).ranks_for(25) == (7,) and EfiSpec((0.58,), (-1,)).ranks_for(50) == (29,)
  assert spec.ranks_for(30) == (27, 3) and spec.ranks_for(10) == (9, 1) and spec.ranks_for(64) == (58, 6)
  assert spec.ranks_for(7) == (7, 0)                        # ceil(6.3), floor(0.7)
  assert EfiSpec((0.7,), (+1,)).ranks_for(10) == (7,) and EfiSpec((0.3,), (-1,)).ranks_for(10) == (3,)
  assert EfiSpec(ranks=(5, 2), directions=(2, -3)).ranks_for(30) == (5, 2)
  assert EfiSpec((), ()).n_events == 0


@pytest.mark.parametrize("kw,exc,msg", [
    (dict(quantiles=(0.0,), directions=(1,)), ValueError, "quantiles must lie in"),
    (dict(quantiles=(0.5,) * 5, directions=(1,) * 5), ValueError, "at most 4 events"),
    (dict(quantiles=(0.5,), directions=(0,)), ValueError, "non-zero signs"),
    (dict(quantiles=(0.5, 0.6), directions=(1,)), ValueError, "non-zero signs"),
    (dict(bins=1), ValueError, "bins must be"), (dict(bins=33), ValueError, "bins must be"),
    (dict(bins=2.5), ValueError, "bins must be"), (dict(ranks=(1.5,), directions=(1,)), ValueError, "ranks must be integers")])
def test_spec_validation(kw, exc, msg):
  with pytest.raises(exc, match=msg):
    EfiSpec(**kw)


# ---- the scores against brute force ---------------------------------------------------------------------------------------
def _case(seed, G=60, B=2, C=2, M=6, K=10, E=8, ranks=(8, 2), dirs=(+1, -1)):
  rng = np.random.default_rng(seed)
  clim = rng.standard_normal((K, G, B, C)).astype(np.float32)
  truth = rng.standard_normal((G, B, C)).astype(np.float32)
  members = (truth + 0.6 * rng.standard_normal((M, G, B, C))).astype(np.float32)
  truth[3, 0, 0] = np.nan
  w = (rng.integers(1, 9, G) / 8.0).astype(np.float32)      # dyadic: every weighted sum below is exact
  wq, scale = quantize_node_weights(w)
  ref = R.reference(members, clim, truth, w, ranks, dirs, E, wq)
  sc = EfiScores(ref["sums"], ref["weighted"], ref["counts"], M, K, ranks, dirs, scale, ref["invalid"])
  return sc, ref, w


def test_scores_match_brute_force_on_small_tables():
  sc, ref, w = _case(0)
  f, o, valid = ref["efi64"], ref["observed64"], ref["valid"]
  B, C, E = 2, 2, 8
  for b in range(B):
    for c in range(C):
      v = valid[:, b, c]
      ww, ff, oo = w[v].astype(np.float64), f[v, b, c], o[v, b, c]
      mf, mo = (ww * ff).sum() / ww.sum(), (ww * oo).sum() / ww.sum()
      np.testing.assert_allclose(sc.efi_mean[b, c], mf, rtol=1e-12)
      np.testing.assert_allclose(sc.observed_mean[b, c], mo, rtol=1e-12)
      corr = (ww * (ff - mf) * (oo - mo)).sum() / math.sqrt((ww * (ff - mf) ** 2).sum() * (ww * (oo - mo) ** 2).sum())
      np.testing.assert_allclose(sc.correlation[b, c], corr, rtol=1e-10)
      for t, (rank, d) in enumerate(zip(sc.ranks, sc.directions)):
        inside = (ref["lt_y"][v, b, c] >= rank) if d > 0 else (ref["le_y"][v, b, c] <= rank)
        assert sc.base_rate[t, b, c] == ww[inside].sum() / ww.sum()
        hits, fars = [], []
        for j in range(E + 1):
          thr = -1.0 + 2.0 * j / E
          warn = (ff >= thr) if d > 0 else (ff < thr)
          if j == E and d > 0:
            warn = np.zeros_like(warn)                      # (f = 1 lies in the last bin: the warning above every bin is empty)
          if j == E and d < 0:
            warn = np.ones_like(warn)
          h, fa = ww[warn & inside].sum() / ww[inside].sum(), ww[warn & ~inside].sum() / ww[~inside].sum()
          assert sc.hit_rate(thr)[t, b, c] == h and sc.false_alarm_rate(thr)[t, b, c] == fa
          hits.append(h)
          fars.append(fa)
        order = np.lexsort((hits, fars))                    # by false-alarm rate, equal ones by hit rate: a monotone curve
        hs, fs = np.asarray(hits)[order], np.asarray(fars)[order]
        area = (0.5 * (fs[1:] - fs[:-1]) * (hs[1:] + hs[:-1])).sum()
        np.testing.assert_allclose(sc.roc_area[t, b, c], area, rtol=1e-12)
        assert sc.roc_area[t, b, c] > 0.6                   # (the members were drawn around the truth)
  with pytest.raises(ValueError, match="bin edge"):
    sc.hit_rate(0.1)


def test_merge_equals_scoring_the_concatenated_dates():
  a, ra, wa = _case(1)
  b, rb, wb = _case(2)
  both = EfiScores.merge([a, b])
  np.testing.assert_array_equal(both.weighted, ra["weighted"] + rb["weighted"])
  np.testing.assert_array_equal(both.counts, ra["counts"] + rb["counts"])
  np.testing.assert_array_equal(both.sums, ra["sums"] + rb["sums"])
  assert both.invalid == 2 and both.ranks == a.ranks and both.n_climatology == 10
  # the same as one date with the nodes of both (dyadic weights: the sums are exact in any order)
  rng1, rng2 = np.random.default_rng(1), np.random.default_rng(2)
  del rng1, rng2
  w = np.concatenate([wa, wb])
  assert both.valid_weight[1, 1] == w.astype(np.float64).sum() and both.valid_weight[0, 0] == w.sum() - wa[3] - wb[3]
  with pytest.raises(ValueError, match="merge: the parts differ"):
    EfiScores.merge([a, _case(3, ranks=(7, 2))[0]])
  with pytest.raises(ValueError, match="weighted must be"):
    EfiScores(ra["sums"], ra["weighted"][:1], ra["counts"][:1], 6, 10, (8, 2), (1, -1))


# ---- the store and the results --------------------------------------------------------------------------------------------
class _Handle(RecordingHandle):
  def ens_efi_set(self, ranks, directions, n_bins, node_weight_q=None):
    self._log("efi_set", tuple(ranks), tuple(directions), n_bins, node_weight_q is not None)
    self.T, self.E = len(ranks), n_bins

  def ens_efi_score(self, clim, table, truth=None):
    self._log("efi_score", clim.name, len(table), truth is None)
    return (self._filled("efi_score", (self.B, self.C, 6)), np.ones((self.T, self.B, self.C, 2, self.E), np.uint64),
            np.ones((self.T, self.B, self.C, 2, self.E), np.uint64), 0)

  def ens_efi_field(self, which=0):
    self._log("efi_field", which)
    return np.full((self.G, self.B, self.C), float(which), np.float32)


G, M, B, C = 4, 3, 2, 3


def _store(log, **kw):
  return verification.ScoredStore(_Handle("h", log, M=M, B=B, C=C, G=G), M, np.ones(G, np.float32), **kw)


def test_store_validation_and_score():
  log = []
  clim = _Handle("clim", log, M=M, B=B, C=C, G=G)
  wq = quantize_node_weights(np.ones(G))
  with pytest.raises(ValueError, match="needs a climatology handle"):
    _store(log, efi=EfiSpec())
  with pytest.raises(ValueError, match="need the quantised node weights"):
    _store(log, efi=EfiSpec(), climatology=clim)
  with pytest.raises(TypeError, match="must be an EfiSpec"):
    _store(log, efi=(0.9, 0.1), climatology=clim)
  assert _store(log, climatology=clim).score_efi() is None
  st = _store(log, efi=EfiSpec(), climatology=clim, weight_q=wq)
  fields = [np.zeros((G, B, C), np.float32)] * 30
  st.score_climatology(fields, "truth")
  del log[:]
  sc = st.score_efi()
  assert [c[1:] for c in log] == [("efi_set", (27, 3), (1, -1), 20, True), ("efi_score", "clim", 31, True)]
  assert isinstance(sc, EfiScores) and sc.ranks == (27, 3) and sc.n_climatology == 30 and sc.scale == wq[1]
  st.score_efi()
  assert [c[1] for c in log].count("efi_set") == 1          # K has not changed: the score alone
  st.score_climatology(fields[:10], None)
  st.score_efi()
  assert log[-2][1:] == ("efi_set", (9, 1), (1, -1), 20, True)
  assert [f.mean() for f in st.efi_fields()] == [0.0, 1.0]
  none = _store(log, efi=EfiSpec((), ()), climatology=clim)   # no events: no quantised weights needed
  none.score_climatology(fields[:4], "truth")
  assert none.score_efi().weighted.shape == (0, B, C, 2, 20)


def test_the_row_reaches_the_rollout_results():
  row = verification.EFI_SCORER
  assert row.name == "efi" and row.word == "extreme forecast index" and not row.scaled and row.series == ("efi",)
  assert row.carried_by == ("ensemble", "derived") and verification.scorer("efi") is row
  assert row not in verification.SCORERS                    # the table's series are a recorded surface: the row stands beside it
  log = []
  clim = _Handle("clim", log, M=M, B=B, C=C, G=G)
  st = _store(log, efi=EfiSpec(), climatology=clim, weight_q=quantize_node_weights(np.ones(G)))
  st.setup()
  series = rollout._StoreSeries(st, np.ones(C), None, keep_efi=True)
  fields = [np.zeros((G, B, C), np.float32)] * 5
  del log[:]
  for _ in range(2):
    series.score_lead("truth", clim_fields=fields)
  assert [c[1] for c in log if c[1].startswith(("clim_", "efi_", "score"))] == \
      ["score", "clim_score", "efi_set", "efi_score", "efi_field", "efi_field", "score", "clim_score", "efi_score", "efi_field",
       "efi_field"]
  assert len(series.efi) == 2 and len(series.efi_fields) == 2 and len(series.efi_fields[0]) == 2
  rng = np.random.default_rng(0)
  ens = lambda: [EnsembleScores(rng.uniform(1, 2, (B, C, 6)), rng.integers(0, 9, (B, C, M + 1)).astype(np.uint64), M) for _ in range(2)]
  # (`plain`: the same series without the index -- the results differ in it alone)
  for res, plain in ((series.derived_result(), rollout.DerivedRolloutResult(**series.carried(rollout.DerivedRolloutResult))),
                     (rollout.EnsembleRolloutResult(n_members=M, efi=series.efi, efi_fields=series.efi_fields,
                                                    **series.carried(rollout.EnsembleRolloutResult)),
                      rollout.EnsembleRolloutResult(n_members=M, **series.carried(rollout.EnsembleRolloutResult)))):
    assert res.efi == series.efi and res.efi_fields is series.efi_fields
    both = res.merge(res)
    for k in range(2):
      np.testing.assert_array_equal(both.efi[k].sums, 2 * res.efi[k].sums)
      np.testing.assert_array_equal(both.efi[k].counts, 2 * res.efi[k].counts)
    assert both.efi_fields is None                          # fields belong to one date
    assert plain.efi is None and plain.efi_fields is None and "efi" not in vars(plain) and "efi_fields" not in vars(plain)
    with pytest.raises(ValueError, match="carries the extreme forecast index"):
      res.merge(plain)
    with pytest.raises(ValueError, match="carries the extreme forecast index"):
      plain.merge(res)
  with pytest.raises(ValueError, match="must cover the same lead times"):
    rollout.EnsembleRolloutResult(ens(), n_members=M, efi=series.efi[:1])
  with pytest.raises(TypeError, match="unexpected keyword argument 'efi'"):
    rollout.WindowRolloutResult([0, 1], 1, ens(), ens(), efi=series.efi)
