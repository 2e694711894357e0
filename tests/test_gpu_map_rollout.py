"""Score maps through the ensemble rollout and the sampler (EnsembleRollout.run(maps=), GenCast.ensemble_maps; DESIGN.md
section 8u) against tests/map_reference.py on the members the device itself kept.  Size: the tiny model of
tests/test_gpu_order_rollout.py (9 x 16 grid, G = 144, batch 2, 82 channels), horizon 2, M = 3, both `norm` settings.

The raw (normalised) planes equal the reference byte for byte.  The physical ones are `scaled` from the raw ones, which is
asserted as an equality, and lie within the affine-map bound of section 8c of the planes of the members mapped to physical
float64 values: that map rounds each value by at most delta = 4 2^-53 max|value|, which moves e, ae and d by at most 2 delta
(differences of two values, averaged) and the square of a value q known to within dq by at most 2 |q| dq + dq^2 (dq = 2 delta
for e, 3 delta plus the roundings of ae and d for c = ae - d / 2); s2 is a mean of squares of
differences over M - 1: Cauchy-Schwarz gives 4 delta sqrt(M s2 / (M - 1)) + 4 delta^2 M / (M - 1).  On top: the (M^2 + 8)
2^-53 |term| that the term's own roundings may differ by."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import EnsembleSampler, rollout, verification
from gencast_flax_nnx_amd.verification import EventMaps, EventSpec, MapSpec, ScoreMaps
from tests import map_reference as R
from tests import window_reference as WR
from tests.test_gpu_derived_rollout import _device_derive
from tests.test_gpu_ensemble_rollout import _Setup, B, C
from tests.test_gpu_verification import _small_model, _stack

pytestmark = pytest.mark.gpu

HORIZON, M = 2, 3
U10, V10 = "10m_u_component_of_wind", "10m_v_component_of_wind"
SPEC = MapSpec(variables=["2m_temperature", "geopotential", U10])
EVENTS = EventSpec({"2m_temperature": np.array([0.5, -0.5]), U10: np.array([1.0, -1.0])}, (+1, -1))


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  for lane in getattr(s.gc.denoiser, "_lanes", None) or []:
    lane.close()
  s.gc.denoiser.native.close()


@pytest.fixture(scope="module")
def runs(setup):
  """One run with the maps and one without, the same members: computed once and left unchanged."""
  out = {}
  for which in ("wrapper", "none"):
    er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
    kw = dict(init_noise=setup.noises[:M], keep_members=True)
    plain = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, **kw)
    with_maps = er.run(setup.inp, setup.targets, setup.forcings, HORIZON, M, maps=SPEC, **kw)
    out[which] = (plain, with_maps)
  return out


def _same(tag, got, want):
  assert got.shape == want.shape and got.dtype == want.dtype, f"{tag}: {got.shape} {got.dtype} against {want.shape} {want.dtype}"
  assert got.tobytes() == want.tobytes(), f"{tag}: {int((got != want).sum())} of {got.size} values differ"


def _physical_bound(members, truth, s, l):
  """(the six per-point terms of the members mapped to physical float64 values, the bound of the module docstring on each)."""
  xp, yp = members.astype(np.float64) * s + l, truth.astype(np.float64) * s + l
  Mn = members.shape[0]
  t = R.point_terms(xp, yp, dtype=np.float64)
  delta = 4.0 * 2.0 ** -53 * np.maximum(np.abs(xp).max(axis=0), np.abs(yp))
  own = (Mn * Mn + 8) * 2.0 ** -53
  square = lambda q, dq: 2.0 * np.abs(q) * dq + dq * dq + own * q * q      # of a value q known to within dq
  terms = [t["e"], t["e"] * t["e"], t["s2"], t["ae"], t["d"], t["c"] * t["c"]]
  f = Mn / (Mn - 1.0)
  dc = 3.0 * delta + own * (t["ae"] + t["d"])                # c = ae - d / 2 cancels: its own roundings are those of ae and d
  bounds = [2.0 * delta + own * np.abs(t["e"]), square(t["e"], 2.0 * delta),
            4.0 * delta * np.sqrt(f * t["s2"]) + 4.0 * delta * delta * f + own * t["s2"],
            2.0 * delta + own * t["ae"], 2.0 * delta + own * t["d"], square(t["c"], dc)]
  return terms, bounds


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_maps_per_lead_equal_the_reference_on_the_kept_members(setup, runs, which):
  _, res = runs[which]
  s, l = setup.stats_per_channel(which)
  ch = SPEC.channels(setup.template0).tolist()
  assert 0 < len(ch) < C and len(res.maps) == len(res.maps_normalized) == HORIZON and res.event_maps is None
  for k in range(HORIZON):
    members, truth = np.stack(res.members[k]), setup.truth(setup.targets, k, which)
    raw = res.maps_normalized[k]
    assert isinstance(raw, ScoreMaps) and raw.n_members == M and raw.channels == tuple(ch) and raw.dates == 1
    ref_sums, ref_counts, _ = R.reference([(members, truth)], ch)
    _same(f"{which} lead {k} counts", raw.counts, ref_counts)
    _same(f"{which} lead {k} sums", raw.sums, ref_sums)
    phys = res.maps[k]
    _same(f"{which} lead {k} physical", phys.sums, raw.scaled(s[ch]).sums)
    terms, bounds = _physical_bound(members[..., ch], truth[..., ch], s[ch], l[ch])
    for j in range(6):
      err = np.abs(phys.sums[j] - terms[j])
      print(f"{which} lead {k} P{j}: worst error / bound {float(np.max(err / np.maximum(bounds[j], 1e-300))):.3f}")
      assert np.all(err <= bounds[j]), f"P{j}"
  ds = res.maps[0].to_dataset(setup.template0, "crps")
  assert np.isfinite(np.asarray(ds["geopotential"].data)).all() and np.isnan(np.asarray(ds[V10].data)).all()


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_a_run_without_maps_is_byte_identical_and_two_runs_merge(runs, which):
  plain, res = runs[which]
  assert plain.maps is None and plain.maps_normalized is None and plain.event_maps is None
  assert not {"maps", "maps_normalized", "event_maps"} & set(vars(plain)) and "event_maps" not in vars(res)
  for k in range(HORIZON):
    for a, b in ((plain.scores[k], res.scores[k]), (plain.scores_normalized[k], res.scores_normalized[k])):
      assert a.sums.tobytes() == b.sums.tobytes() and a.rank_histogram.tobytes() == b.rank_histogram.tobytes()
    for m in range(M):                                            # the member states: bit-identical with and without `maps=`
      assert plain.members[k][m].tobytes() == res.members[k][m].tobytes()
  merged = res.merge(res)
  for k in range(HORIZON):
    _same("merged", merged.maps_normalized[k].sums, res.maps_normalized[k].sums + res.maps_normalized[k].sums)
    assert merged.maps[k].dates == 2 and np.array_equal(merged.maps[k].counts, 2 * res.maps[k].counts)
  with pytest.raises(ValueError, match="score maps"):
    res.merge(plain)


def test_resident_maps_over_two_start_dates_equal_the_merge_of_two_runs(setup):
  which = "wrapper"
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
  args = (setup.inp, setup.targets, setup.forcings, HORIZON, M)
  starts = [dict(init_noise=setup.noises[:M]), dict(init_noise=setup.noises[1:M + 1])]
  per_run = [er.run(*args, maps=SPEC, **kw) for kw in starts]
  assert per_run[0].maps_normalized[1].sums.tobytes() != per_run[1].maps_normalized[1].sums.tobytes()
  merged = per_run[0].merge(per_run[1])
  er.reset_maps()
  for kw in starts:
    res = er.run(*args, maps=SPEC, maps_resident=True, **kw)
    assert res.maps is None and "maps" not in vars(res)
  got = er.download_maps()
  assert sorted(got, key=str) == [None]
  sc = setup.stats_per_channel(which)[0][SPEC.channels(setup.template0)]
  for k in range(HORIZON):
    for name in ("maps", "maps_normalized"):
      _same(f"resident {name} {k} counts", got[None][name][k].counts, getattr(merged, name)[k].counts)
    _same(f"resident {k}", got[None]["maps_normalized"][k].sums, merged.maps_normalized[k].sums)
    # in physical units the resident sums are scaled once, (a + b) s, the merged results date by date, a s + b s
    _same(f"resident physical {k}", got[None]["maps"][k].sums, merged.maps_normalized[k].scaled(sc).sums)
    a, b = per_run[0].maps[k].sums, per_run[1].maps[k].sums
    assert np.all(np.abs(got[None]["maps"][k].sums - merged.maps[k].sums) <= 4.0 * 2.0 ** -53 * (np.abs(a) + np.abs(b)))
    assert got[None]["maps"][k].dates == 2
  again = er.download_maps()                                      # a download changes nothing
  _same("again", again[None]["maps_normalized"][0].sums, got[None]["maps_normalized"][0].sums)
  with pytest.raises(ValueError, match="another plan or horizon"):
    er.run(setup.inp, setup.targets, setup.forcings, 1, M, maps=SPEC, maps_resident=True, **starts[0])
  with pytest.raises(ValueError, match="another plan or horizon"):
    er.run(*args, maps=MapSpec(), maps_resident=True, **starts[0])
  er.reset_maps()
  assert not er.download_maps()[None]["maps_normalized"][0].counts.any()
  res = er.run(setup.inp, setup.targets, setup.forcings, 1, M, maps=MapSpec(), **starts[0])       # cleared: another plan goes
  assert len(res.maps) == 1 and res.maps[0].sums.shape[-1] == C
  with pytest.raises(ValueError, match="maps_resident goes with maps"):
    er.run(*args, maps_resident=True, **starts[0])


def test_a_derived_view_a_window_and_the_event_planes(setup):
  """`maps={None: ..., "wind": ..., "sum2": ...}`: the view's maps cover ITS channels, the window's one slot per window.  The
  derived truth has no download: it is formed by the same device call on two handles of the test's own, as in
  tests/test_gpu_derived_rollout.py.  The main store also keeps the event planes of its EventSpec."""
  which = "wrapper"
  dspec = verification.DerivedSpec([("norm2", "wind10", U10, V10), ("copy", "2m_temperature")])
  wspec = verification.WindowSpec("sum", 2)
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which))
  args = (setup.inp, setup.targets, setup.forcings, HORIZON, M)
  spec_w = MapSpec(variables=["2m_temperature"])
  res = er.run(*args, init_noise=setup.noises[:M], keep_members=True, derived={"wind": dspec}, windows={"sum2": wspec},
               events=EVENTS, maps={None: MapSpec(variables=SPEC.variables, events=True), "wind": MapSpec(), "sum2": spec_w})
  s, l = setup.stats_per_channel(which)
  ch = SPEC.channels(setup.template0).tolist()
  # the main store: the field planes as before, the event planes against the tables of the same leads
  for k in range(HORIZON):
    members, truth = np.stack(res.members[k]), setup.truth(setup.targets, k, which)
    ref_sums, ref_counts, _ = R.reference([(members, truth)], ch)
    _same(f"main {k}", res.maps_normalized[k].sums, ref_sums)
    ev = res.event_maps[k]
    assert isinstance(ev, EventMaps) and ev.directions == (1, -1) and ev.channels == tuple(ch) and ev.dates == 1
    table = res.events[k].counts[:, :, ch]                         # [T, B, C', 2, M + 1]
    kk = np.arange(M + 1, dtype=np.uint64)
    e = ev.events.sum(axis=2, dtype=np.uint64)                     # [T, 5, B, C']
    assert np.array_equal(e[:, 0], table.sum(axis=(-1, -2))) and np.array_equal(e[:, 1], (table * kk).sum(axis=(-1, -2)))
    assert np.array_equal(e[:, 2], (table * kk * kk).sum(axis=(-1, -2))) and np.array_equal(e[:, 4], table[..., 1, :].sum(axis=-1))
    assert np.array_equal(e[:, 3], (table[..., 1, :] * kk).sum(axis=-1)) and e[:, 0].any() and e[:, 3].any()
  # the view
  d = res.derived["wind"]
  assert len(d.maps) == len(d.maps_normalized) == HORIZON and d.event_maps is None
  dplan = dspec.plan(setup.template0, s, l)
  sd, _ = dspec.channel_stats(setup.template0, s, l)
  for k in range(HORIZON):
    members = np.stack(d.members[k])                              # the device's own derived members
    truth_raw = setup.truth(setup.targets, k, which)
    truth_d = _device_derive(setup.gc.denoiser.graph, dplan, np.stack([truth_raw, truth_raw]))[0]
    ref_sums, ref_counts, _ = R.reference([(members, truth_d)])
    _same(f"derived {k} counts", d.maps_normalized[k].counts, ref_counts)
    _same(f"derived {k}", d.maps_normalized[k].sums, ref_sums)
    _same(f"derived {k} physical", d.maps[k].sums, d.maps_normalized[k].scaled(sd).sums)
  # the window: the sum over both leads of the main store, one slot
  win = res.windows["sum2"]
  assert win.leads == [1] and len(win.maps) == len(win.maps_normalized) == 1
  sw, _ = wspec.channel_stats(s, l)
  cw = spec_w.channels(setup.template0).tolist()
  kind, coef = WR.coefficients("sum", 2)
  truth_w = WR.window(np.stack([setup.truth(setup.targets, k, which) for k in range(2)]), kind, coef)
  ref_sums, ref_counts, _ = R.reference([(np.stack(win.members[0]), truth_w)], cw)
  _same("window counts", win.maps_normalized[0].counts, ref_counts)
  _same("window", win.maps_normalized[0].sums, ref_sums)
  _same("window physical", win.maps[0].sums, win.maps_normalized[0].scaled(sw[cw]).sums)
  # an entry that was given no spec carries no maps; an unknown key and event planes without events are refused
  only = er.run(*args, init_noise=setup.noises[:M], derived={"wind": dspec}, maps={"wind": MapSpec()})
  assert only.maps is None and len(only.derived["wind"].maps) == HORIZON
  _same("only", only.derived["wind"].maps_normalized[1].sums, d.maps_normalized[1].sums)
  with pytest.raises(ValueError, match="nope"):
    er.run(*args, init_noise=setup.noises[:M], derived={"wind": dspec}, maps={"nope": SPEC})
  with pytest.raises(ValueError, match="need the store's EventSpec"):
    er.run(*args, init_noise=setup.noises[:M], maps=MapSpec(events=True))


def test_single_date_ensemble_maps_equal_the_reference_on_the_samplers_own_members():
  gc, inp, tgt, frc = _small_model()
  try:
    n = 4
    ens = EnsembleSampler(gc._sampler, base_seed=5)
    fields = [_stack(d) for _, d in sorted(ens(inp, tgt.map(np.zeros_like), frc, n), key=lambda t: t[0])]
    truth = _stack(tgt)
    spec = MapSpec(variables=["2m_temperature", "geopotential"])
    ch = spec.channels(tgt).tolist()
    got = gc.ensemble_maps(inp, tgt, frc, num_members=n, spec=spec, rngs=5)
    ref_sums, ref_counts, _ = R.reference([(np.stack(fields), truth)], ch)
    assert isinstance(got, ScoreMaps) and got.channels == tuple(ch) and got.n_members == n and got.dates == 1
    _same("ensemble_maps counts", got.counts, ref_counts)
    _same("ensemble_maps", got.sums, ref_sums)
    q = {"2m_temperature": np.quantile(np.asarray(tgt["2m_temperature"].data, np.float64), [0.75, 0.25])}
    events = EventSpec(q, (+1, -1))
    maps, ev = gc.ensemble_maps(inp, tgt, frc, num_members=n, spec=MapSpec(variables=["2m_temperature"], events=True),
                                events=events, rngs=5)
    c0 = maps.channels[0]
    _same("with events", maps.sums, ref_sums[..., [ch.index(c0)]])
    table = gc.ensemble_events(inp, tgt, frc, num_members=n, spec=events, rngs=5).counts[:, :, [c0]]
    assert np.array_equal(ev.events[:, 0].sum(axis=1, dtype=np.uint64), table.sum(axis=(-1, -2))) and ev.events[:, 0].any()
    with pytest.raises(ValueError, match="needs an EventSpec"):
      gc.ensemble_maps(inp, tgt, frc, num_members=n, spec=MapSpec(events=True), rngs=5)
    with pytest.raises(ValueError, match="ens_push_host"):
      EnsembleSampler(gc._sampler, rank=0, world_size=2).maps(inp, tgt, frc, n, spec)
  finally:
    gc.denoiser.native.close()
