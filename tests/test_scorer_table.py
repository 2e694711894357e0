"""A per-store scorer is declared once, as a row of `verification.SCORERS`: a made-up row "probe", appended to the table and to
nothing else, is configured and scored by `ScoredStore`, appended per lead time by the rollout's `_StoreSeries`, and carried and
merged by the three results.  The second half pins the public result surface the real rows declare.  No device, no library:
the handles record (`helpers.RecordingHandle`)."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import rollout, verification
from gencast_flax_nnx_amd.verification import AdditiveScores, EnsembleScores, RegionSpec, Scorer
from tests.helpers import RecordingHandle

G, M, B, C = 4, 4, 2, 3
REGIONS = RegionSpec({"south": np.array([True, True, False, False]), "east": np.array([False, True, False, True])})
BITS = np.array([1, 3, 0, 2], np.uint32)
SCALE = np.array([4.0, 1.0, 0.25])


class ProbeScores(AdditiveScores):
  """A tiny additive score: one raw sum per (batch, channel)."""
  _adds = ("sums",)

  def __init__(self, sums, n_members):
    self.sums, self.n_members = np.asarray(sums, np.float64), int(n_members)

  def scaled(self, channel_scale):
    return ProbeScores(self.sums * np.asarray(channel_scale)[None, :], self.n_members)


class _Handle(RecordingHandle):
  """The recording handle with the regions' two calls and the probe's."""

  def ens_region_set(self, bits, n_regions):
    self._log("region_set", n_regions)

  def ens_region_score(self, truth):
    self._log("region_score", truth is None)
    return (self._filled("region_score", (2, self.B, self.C, 6)),
            self._filled("region_score", (2, self.B, self.C, self.M + 1), np.uint64), np.zeros(2, np.uint64))

  def ens_probe_set(self, setting):
    self._log("probe_set", setting)

  def ens_probe_score(self, truth):
    self._log("probe_score", truth is None)
    return self._filled("probe_score", (self.B, self.C))


PROBE = Scorer("probe", "probe scores", ("probe_setting",), set=lambda s: s.handle.ens_probe_set(s.probe_setting),
               score=lambda s, truth: ProbeScores(s.handle.ens_probe_score(truth), s.n_members))


@pytest.fixture
def probe(monkeypatch):
  """The table with the probe row appended, for one test (monkeypatch puts the table back)."""
  monkeypatch.setattr(verification, "SCORERS", verification.SCORERS + [PROBE])
  return PROBE


def _store(log, **kw):
  return verification.ScoredStore(_Handle("h", log, M=M, B=B, C=C, G=G), M, np.ones(G, np.float32), **kw)


def _ens(rng):
  return EnsembleScores(rng.uniform(1, 2, (B, C, 6)), rng.integers(0, 9, (B, C, M + 1)).astype(np.uint64), M)


def test_a_store_sets_the_probe_after_the_regions_and_scores_it(probe):
  """(`configure()` itself sets whatever is switched on, per score or not, as it always has: the store that sets per score is
  the one whose `setup()` does not configure.)"""
  log = []
  st = _store(log, regions=REGIONS, region_bits=BITS, probe="spec", probe_setting=7)
  assert st.probe == "spec" and st.probe_setting == 7
  st.configure()
  assert [c[1:] for c in log] == [("region_set", 2), ("probe_set", 7)]
  got = st._score(probe, "truth")
  assert isinstance(got, ProbeScores) and got.n_members == M and log[-1][1:] == ("probe_score", False)
  st._score(probe, None)
  assert log[-1][1:] == ("probe_score", True) and [c[1] for c in log].count("probe_set") == 1      # the score alone
  # set per score: not by setup, but by every scoring call, before it
  log2 = []
  per = _store(log2, regions=REGIONS, region_bits=BITS, probe="spec", probe_setting=7, set_per_score=True)
  per.setup()
  assert [c[1] for c in log2] == ["reserve", "weight"]
  per._score(probe, None)
  per._score(probe, None)
  assert [c[1:] for c in log2[2:]] == [("probe_set", 7), ("probe_score", True)] * 2
  # a store without the probe: None, and no call
  log3 = []
  plain = _store(log3)
  plain.setup()
  assert plain.probe is None and plain._score(probe, None) is None
  assert [c[1] for c in log3] == ["reserve", "weight"]


def test_the_probe_is_a_keyword_of_the_store_only_while_its_row_is_in_the_table():
  with pytest.raises(TypeError, match="unexpected keyword argument 'probe'"):
    _store([], probe="spec")
  with pytest.raises(TypeError, match="unexpected keyword argument"):
    rollout.DerivedRolloutResult([], [], probe=[])


def _series(log):
  st = _store(log, regions=REGIONS, region_bits=BITS, probe="spec", probe_setting=7)
  st.setup()
  series = rollout._StoreSeries(st, SCALE, None, keep_members=True)
  del log[:]
  series.score_lead("truth")
  series.score_lead("truth")
  return series


def test_a_lead_scores_the_probe_after_the_regions_and_before_the_members(probe):
  log = []
  series = _series(log)
  assert [c[1] for c in log] == (["score", "region_score", "probe_score"] + ["download"] * M) * 2
  assert log[2][1:] == ("probe_score", True)                         # on the truth already on the device
  raw, scaled = series.lists["probe_normalized"], series.lists["probe"]
  assert len(raw) == len(scaled) == 2 and series.probe is scaled and series.raw_probe is raw
  for k in range(2):                                                 # in the order of the calls; physical = `scaled` of the raw
    np.testing.assert_array_equal(raw[k].sums, float(k + 1))
    np.testing.assert_array_equal(scaled[k].sums, raw[k].sums * SCALE[None, :])


def test_the_three_results_carry_and_merge_the_probe(probe):
  series = _series([])
  raw, scaled = series.lists["probe_normalized"], series.lists["probe"]
  rng = np.random.default_rng(0)
  pair = lambda: ([_ens(rng) for _ in range(2)], [_ens(rng) for _ in range(2)])
  rest = {"regions": series.regions, "regions_normalized": series.raw_regions}        # (the series differ in the probe alone)
  window = rollout._WindowEntry(verification.WindowSpec("sum", 1), series, None, 2)
  for res, without, kind in (
      (series.derived_result(), rollout.DerivedRolloutResult(*pair(), **rest), "derived results"),
      (window.result(), rollout.WindowRolloutResult([0, 1], 1, *pair(), **rest), "window results"),
      (rollout.EnsembleRolloutResult(n_members=M, **series.carried(rollout.EnsembleRolloutResult)),
       rollout.EnsembleRolloutResult(pair()[0], n_members=M, **rest), "results")):
    assert "probe" in vars(res) and "probe_normalized" in vars(res)
    both = res.merge(res)
    for k in range(2):
      assert res.probe[k] is scaled[k] and res.probe_normalized[k] is raw[k]
      np.testing.assert_array_equal(both.probe[k].sums, 2 * scaled[k].sums)
      np.testing.assert_array_equal(both.probe_normalized[k].sums, 2 * raw[k].sums)
      np.testing.assert_array_equal(both.regions[k].sums, 2 * res.regions[k].sums)
    # a result that was not given the series has neither name, reads them as None and does not merge with one that has
    assert without.probe is None and without.probe_normalized is None
    assert "probe" not in vars(without) and "probe_normalized" not in vars(without)
    assert "probe" not in vars(without.merge(without))
    with pytest.raises(ValueError, match=f"merge: only one of the two {kind} carries probe scores"):
      res.merge(without)
    with pytest.raises(ValueError, match=f"merge: only one of the two {kind} carries probe scores"):
      without.merge(res)
  with pytest.raises(ValueError, match="scores and probe scores must cover the same lead times"):
    rollout.EnsembleRolloutResult([_ens(rng)], n_members=M, probe=scaled, probe_normalized=raw)


def test_with_the_row_removed_again_a_plain_result_is_what_it_was(monkeypatch):
  rng = np.random.default_rng(1)
  with monkeypatch.context() as m:
    m.setattr(verification, "SCORERS", verification.SCORERS + [PROBE])
    assert "probe" in rollout.EnsembleRolloutResult._carries()
  assert "probe" not in rollout.EnsembleRolloutResult._carries() and PROBE not in verification.SCORERS
  plain = rollout.EnsembleRolloutResult([_ens(rng) for _ in range(2)], n_members=M)
  assert sorted(vars(plain)) == sorted(["scores", "scores_normalized", "spectra", "spectra_normalized", "events", "order",
                                        "order_normalized", "climatology", "climatology_normalized", "derived", "windows",
                                        "mean", "variance", "members", "quantiles", "n_members"])
  with pytest.raises(AttributeError):
    plain.probe  # pylint: disable=pointless-statement


# ---- the real rows: the record of the public result surface --------------------------------------------------------------------
SERIES = ["scores", "scores_normalized", "spectra", "spectra_normalized", "events", "order", "order_normalized", "climatology",
          "climatology_normalized", "energy", "variogram", "variogram_normalized", "tails", "tails_normalized", "regions",
          "regions_normalized"]
OPTIONAL = ["energy", "variogram", "variogram_normalized", "tails", "tails_normalized", "regions", "regions_normalized"]
WORDS = {"scores": None, "spectra": "spectra", "events": "events", "order": "order statistics",
         "climatology": "climatology scores", "energy": "energy scores", "variogram": "variogram scores", "tails": "tail scores",
         "regions": "region scores"}


def test_the_table_declares_the_series_the_results_have_always_had():
  rows = verification.SCORERS
  assert [name for row in rows for name in row.series] == SERIES
  assert [name for row in rows if row.optional for name in row.series] == OPTIONAL
  assert {row.name: row.word for row in rows} == WORDS
  assert rollout.EnsembleRolloutResult._carries() == SERIES
  assert rollout.DerivedRolloutResult._carries() == [s for s in SERIES if not s.startswith("spectra")]
  assert rollout.WindowRolloutResult._carries() == [s for s in SERIES if not s.startswith(("spectra", "climatology"))]
  # what a store is configured with and scores through the table, in the order it is configured
  assert [row.name for row in rows if row.score is not None] == ["events", "order", "energy", "variogram", "tails", "regions"]
  assert all((row.set is None) == (row.score is None) for row in rows)
  assert {row.name: row.settings for row in rows if row.settings} == {
      "events": ("thresholds", "weight_q"), "tails": ("tail_thresholds",), "regions": ("region_bits",)}
