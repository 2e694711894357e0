"""Spherical-harmonic power spectra on the device (gc_spec_*, gc_ens_spectrum) against the float64 definition
(tests/spectrum_reference.py).

Tolerances are derived, not measured: device and reference analyse the same float32 data with the same float32 tables in
binary64 and differ in summation order only.  With u = 2^-53 and Abar_lm the reference's nested sum of absolute terms,
    da_lm = 2 (n_lon + n_lat + 2) u Abar_lm,
    |dpower_l| <= sum_{m, parts} (2 |a| da + da^2) / (4 pi) + (2 l + 3) u power_l,
and the ensemble sums compose these as the docstring of tests/spectrum_reference.py states (M of them per member sum plus
M u for the additions, M roundings for the mean).  Every test prints the worst ratio error / bound before it asserts.
At the full sizes the reference is evaluated on a strided subset of the 82 columns (every 9th at 2.5 degrees, every 27th
at 1 degree): the device result of those columns is compared; all columns are checked to be finite."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import EnsembleSpectra, SphericalAnalysis, _lib, geometry
from tests import helpers
from tests.helpers import graph_handle as _handle, small_graph as _graph
from tests import spectrum_reference as R

pytestmark = pytest.mark.gpu


def _latlon(n_lat, n_lon):
  return np.linspace(-90, 90, n_lat), np.arange(n_lon) * (360.0 / n_lon)


def _data(M, G, B, C, seed, scale):
  rng = np.random.default_rng(seed)
  members = (rng.standard_normal((M, G, B, C)) * scale).astype(np.float32)
  truth = (rng.standard_normal((G, B, C)) * scale).astype(np.float32)
  return members, truth


def _push_all(nd, members):
  nd.ens_reserve(len(members))
  for i, x in enumerate(members):
    nd.ens_push_host(i, x)


def _check(tag, got, want, tol, names=("power",)):
  """got / want / tol [..., k]; NaN entries must coincide, the others lie within the bound."""
  nan = np.isnan(want)
  np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f"{tag}: NaN entries")
  err = np.where(nan, 0.0, np.abs(got - want))
  ratio = err / np.maximum(tol, 1e-300)
  for k, name in enumerate(names):
    r = ratio[..., k] if len(names) > 1 else ratio
    e = err[..., k] if len(names) > 1 else err
    print(f"{tag} {name}: max |device - reference| {e.max():.3e}, worst ratio to the bound {r.max():.4f}")
  assert np.all(err <= tol), f"{tag}: outside the derived bound (worst ratio {ratio.max():.3f})"


def _run_case(tag, n_lat, n_lon, B, C, M, scale, cols, hw=None, gr=None):
  gr = gr or _graph(n_lat, n_lon)
  G, N = gr.num_grid_nodes, B * C
  assert G == n_lat * n_lon
  sa = SphericalAnalysis(*_latlon(n_lat, n_lon))
  tabs = sa.device_tables()
  L = sa.lmax
  members, truth = _data(M, G, B, C, seed=M + n_lat, scale=scale)
  ref = R.ensemble(members, truth, n_lat, n_lon, tabs, cols=cols)
  pick = (lambda a: a) if cols is None else (lambda a: a[np.asarray(cols)])
  nd = _handle(gr, B, C, **(hw or {}))
  try:
    nd.spec_set_tables(*tabs)
    _push_all(nd, members)
    sums, mp = nd.ens_spectrum(truth, want_member_power=True)
    assert sums.shape == (B, C, L, 6) and mp.shape == (M, B, C, L) and sums.dtype == mp.dtype == np.float64
    assert np.isfinite(sums).all() and np.isfinite(mp).all()
    _check(tag, pick(sums.reshape(N, L, 6)), ref["sums"], ref["tol"], R.SUM_NAMES)
    _check(tag + " member power", np.stack([pick(p.reshape(N, L)) for p in mp]), ref["member_power"], ref["member_tol"])
    # member_power adds up to P1 (the device adds the same numbers in the same order; the bound is what is promised)
    tot = np.zeros((N, L))
    for p in mp:
      tot = tot + p.reshape(N, L)
    _check(tag + " sum of member power vs P1", pick(tot), pick(sums.reshape(N, L, 6)[..., 1]), ref["tol"][..., 1])
    # one field on its own: the truth, and the same call twice
    p0 = nd.spec_field(truth)
    _check(tag + " spec_field(truth)", pick(p0.reshape(N, L)), ref["sums"][..., 0], ref["tol"][..., 0])
    assert nd.spec_field(truth).tobytes() == p0.tobytes()
    again = nd.ens_spectrum(None)                                  # the truth stays on the device; no member power asked
    assert again.tobytes() == sums.tobytes()
    assert nd.counter("spec_invalid_columns") == 0 and nd.counter("spec_calls") == 4
    print(f"{tag}: spec_device_us {nd.counter('spec_device_us')} (M = {M})")
    # the derived spectra are finite and positive where the sums are
    sp = EnsembleSpectra(sums, M)
    assert (sp.truth_power > 0).all() and (sp.spread_power > 0).all() and np.isfinite(sp.spectral_spread_skill).all()
  finally:
    nd.close()


# ---- 1. tiny grid, channel scales over eight decades ----------------------------------------------------------------------
@pytest.mark.parametrize("M", [2, 8])
def test_spectra_match_the_float64_definition_tiny(M):
  _run_case(f"tiny M={M}", 13, 24, 2, 6, M, np.logspace(-3, 5, 6), None)


# ---- 2. full-size grids, set_graph only -----------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [8, 50])
def test_spectra_match_the_float64_definition_nano(M):
  gr = _graph(73, 144, mesh_size=4, k_hop=8)
  _run_case(f"nano M={M}", 73, 144, 1, 82, M, np.logspace(-2, 4, 82), list(range(0, 82, 9)),
            hw=dict(latent=256, heads=4, ffw=2048), gr=gr)


def test_spectra_match_the_float64_definition_one_degree():
  lat, lon = np.arange(-90.0, 90.0 + 1e-9, 1.0), np.arange(0.0, 360.0, 1.0)
  gr = geometry.build_denoiser_graph(grid_lat=lat, grid_lon=lon, mesh_size=5, attention_k_hop=8)
  assert gr.num_grid_nodes == 65160
  _run_case("one_degree M=4", 181, 360, 1, 82, 4, np.logspace(-2, 4, 82), list(range(0, 82, 27)),
            hw=dict(latent=512, heads=4, ffw=2048), gr=gr)


# ---- 3. the library's own noise: a spectrum known in closed form ---------------------------------------------------------
def test_noise_field_has_its_closed_form_spectrum():
  """gc_noise_draw for (seed, stream), then the analysis of that field, against p_l / (2l+1) sum_m z_lm^2 of the oracle's
  Philox normals.  The existing noise test pins the field to 2e-5 (unit scale) of the exact synthesis at every node; a
  node error of eps moves a_lm by at most eps S_lm, S_lm = sum_lat |Q| sum_j |T| (R.pointwise_gain).  The float32
  analysis tables add 2 * 2^-24 max|f| S_lm, the binary64 sums (n_lon + n_lat + 2) 2u max|f| S_lm.  That da goes through
  the power bound of the module docstring, around the exact coefficients sqrt(4 pi p_l / (2l+1)) z_lm."""
  from oracle import noise_oracle as NO
  from gencast_flax_nnx_amd import noise
  gr, dims, params, _, _ = helpers.tiny_setup(batch=2)                      # 13 x 24 grid: equiangular with poles
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    lat, lon = _latlon(13, 24)
    gen = noise.SphericalNoise(lat, lon)
    sa = SphericalAnalysis(lat, lon)
    L, N = sa.lmax, 2 * dims.c_out
    assert L == gen.lmax
    nd.noise_set_tables(13, 24, *gen.device_tables())
    tabs = sa.device_tables()
    nd.spec_set_tables(*tabs)
    S = R.pointwise_gain(*tabs)[..., None]
    for seed, stream in ((5, 0), (2 ** 40 + 3, 7)):
      nd.noise_seed(seed, stream)
      nd.noise_draw()
      field = nd.download_noise()
      got = nd.spec_field(field).reshape(N, L)
      z = NO.philox_normals(2 * L * L * N, seed, stream).reshape(2, L, L, N)
      fmax = float(np.abs(field).max())
      da = (2e-5 + 2 * 2.0 ** -24 * fmax + 2 * (24 + 13 + 2) * R.U * fmax) * S * np.ones((1, 1, 1, N))
      tol = R.power_tolerance(R.noise_coefficients(z), da)
      want = R.noise_coefficient_power(z)
      _check(f"noise ({seed}, {stream})", got, want, tol)
      print(f"noise ({seed}, {stream}): mean power x L = {got.mean() * L:.4f} (expectation 1), worst relative bound {np.max(tol / want):.2e}")
  finally:
    nd.close()


# ---- 4. non-finite values --------------------------------------------------------------------------------------------------
def test_non_finite_values_poison_exactly_their_columns():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 4
  N = B * C
  tabs = SphericalAnalysis(*_latlon(13, 24)).device_tables()
  members, truth = _data(M, G, B, C, seed=21, scale=np.ones(6))
  clean = R.ensemble(members, truth, 13, 24, tabs)
  members[2, 100, 1, 2] = np.nan                                          # column 1 * 6 + 2 = 8
  members[0, 311, 0, 5] = np.inf                                          # column 5
  members[3, 0, 0, 5] = -np.inf                                           # the same column again: counted once
  truth[7, 1, 0] = np.nan                                                 # column 6
  ref = R.ensemble(members, truth, 13, 24, tabs)
  assert sorted(np.flatnonzero(ref["bad"]).tolist()) == [5, 6, 8]
  nd = _handle(gr, B, C)
  try:
    nd.spec_set_tables(*tabs)
    _push_all(nd, members)
    sums, mp = nd.ens_spectrum(truth, want_member_power=True)
    _check("non-finite", sums.reshape(N, -1, 6), ref["sums"], ref["tol"], R.SUM_NAMES)
    _check("non-finite member power", mp.reshape(M, N, -1), ref["member_power"], ref["member_tol"])
    assert np.isnan(sums.reshape(N, -1)[[5, 6, 8]]).all() and np.isnan(mp.reshape(M, N, -1)[:, [5, 6, 8]]).all()
    keep = [n for n in range(N) if n not in (5, 6, 8)]
    assert np.isfinite(sums.reshape(N, -1)[keep]).all()
    _check("non-finite, untouched columns", sums.reshape(N, -1, 6)[keep], clean["sums"][keep], clean["tol"][keep], R.SUM_NAMES)
    assert nd.counter("spec_invalid_columns") == 3
    # one field: the truth has one bad column, member 1 none
    p = nd.spec_field(truth).reshape(N, -1)
    assert np.isnan(p[6]).all() and np.isfinite(np.delete(p, 6, axis=0)).all() and nd.counter("spec_invalid_columns") == 1
    assert np.isfinite(nd.spec_field(members[1])).all() and nd.counter("spec_invalid_columns") == 0
  finally:
    nd.close()


# ---- 5. determinism and ownership ---------------------------------------------------------------------------------------------
def test_spectra_are_deterministic_and_the_buffers_are_replaced_not_grown():
  gr = _graph()
  G, B, C, M = gr.num_grid_nodes, 2, 6, 8
  tabs = SphericalAnalysis(*_latlon(13, 24)).device_tables()
  members, truth = _data(M, G, B, C, seed=31, scale=np.logspace(-3, 5, 6))
  nd = _handle(gr, B, C)
  try:
    base = nd.counter("device_allocations")
    nd.spec_set_tables(*tabs)
    _push_all(nd, members)
    a = nd.ens_spectrum(truth, want_member_power=True)
    held = nd.counter("device_allocations")
    assert held > base
    b = nd.ens_spectrum(truth, want_member_power=True)
    for x, y in zip(a, b):
      assert x.tobytes() == y.tobytes()
    for _ in range(3):
      nd.ens_reserve(M)                                                   # a re-reserve: the store is replaced
      for i in reversed(range(M)):
        nd.ens_push_host(i, members[i])
      c = nd.ens_spectrum(None, want_member_power=True)
      for x, y in zip(a, c):
        assert x.tobytes() == y.tobytes()
      nd.spec_field(members[0])
      assert nd.counter("device_allocations") == held
    nd.ens_reserve(3)                                                     # fewer members: the coefficient sets are kept
    for i in range(3):
      nd.ens_push_host(i, members[i])
    nd.ens_spectrum(None)
    assert nd.counter("device_allocations") == held
    nd.spec_set_tables(*tabs)                                             # the same tables again: replaced
    nd.ens_spectrum(None)
    assert nd.counter("device_allocations") == held
    small = SphericalAnalysis(*_latlon(13, 24), lmax=7).device_tables()  # the caller's band limit
    nd.spec_set_tables(*small)
    s7 = nd.ens_spectrum(None)
    assert s7.shape == (B, C, 7, 6) and nd.counter("device_allocations") == held
    ref = R.ensemble(members[:3], truth, 13, 24, small)
    _check("lmax 7", s7.reshape(B * C, 7, 6), ref["sums"], ref["tol"], R.SUM_NAMES)
    assert nd.counter("spec_calls") == 2 + 6 + 3
  finally:
    nd.close()


# ---- 6. the resident sample ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", ["on", "off"])
def test_spectrum_of_the_resident_sample_leaves_the_sampler_state_alone(graphs):
  from oracle import gencast_oracle as O
  gr, dims, params, cond, _ = helpers.tiny_setup(batch=2, seed=2)
  rng = np.random.default_rng(8)
  G = gr.num_grid_nodes
  noise = rng.standard_normal((G, 2, dims.c_out)).astype(np.float32)
  truth = rng.standard_normal((G, 2, dims.c_out)).astype(np.float32)
  tabs = SphericalAnalysis(*_latlon(13, 24)).device_tables()
  nd = helpers.make_native(gr, dims, params, 2)
  try:
    nd.set_option("graphs", graphs)
    nd.set_noisy_slots(np.arange(dims.c_in - dims.c_out, dims.c_in, dtype=np.int32))
    nd.upload_cond(cond)
    nd.upload_noise(noise)
    nd.spec_set_tables(*tabs)
    with pytest.raises(_lib.GencastHipError, match="sample"):      # no sample yet
      nd.spec_field(None)
    sched = O.noise_schedule(80.0, 0.03, 4, 7.0).astype(np.float32)
    nd.sample_resident(sched)
    first = nd.download_sample()
    nd.sample_resident(sched)                                      # with graphs on: captured here
    np.testing.assert_array_equal(nd.download_sample(), first)
    nd.stash_sample()
    replays, captures = nd.counter("graph_replays"), nd.counter("graph_captures")
    resident = nd.spec_field(None)                                 # analysed where it lies
    assert resident.tobytes() == nd.spec_field(first).tobytes()    # = the spectrum of the downloaded sample
    p, tol = R.field_spectrum(first, 13, 24, tabs)
    _check("resident sample", resident.reshape(p.shape), p, tol)
    nd.ens_reserve(2)
    nd.ens_push(0)
    nd.ens_push_host(1, truth)
    sums = nd.ens_spectrum(truth)
    ref = R.ensemble(np.stack([first, truth]), truth, 13, 24, tabs)
    _check("pushed sample", sums.reshape(-1, sums.shape[2], 6), ref["sums"], ref["tol"], R.SUM_NAMES)
    np.testing.assert_array_equal(nd.download_sample(), first)      # the last sample is still there
    np.testing.assert_array_equal(nd.download_stash(), first)
    np.testing.assert_array_equal(nd.download_cond(), cond)
    np.testing.assert_array_equal(nd.download_noise(), noise)
    nd.sample_resident(sched)                                      # a replay of the captured graph: the same bytes
    np.testing.assert_array_equal(nd.download_sample(), first)
    assert nd.counter("graph_captures") == captures
    if graphs == "on":
      assert nd.counter("graph_replays") == replays + 1
  finally:
    nd.close()


# ---- 7. sampler and Dataset level -------------------------------------------------------------------------------------------
def test_sampler_scores_and_spectra_with_the_dataset_wrappers(monkeypatch):
  import sys
  from gencast_flax_nnx_amd import EnsembleSampler, NaNCleaner, config, datasets, rollout
  from gencast_flax_nnx_amd.datasets import Dataset, Variable
  from tests import fake_xarray
  from tests.test_gpu_verification import _small_model, _stack
  monkeypatch.setitem(sys.modules, "xarray", fake_xarray)
  gc, inp, tgt, frc = _small_model()
  M = 4
  try:
    tabs = SphericalAnalysis.for_template(tgt).device_tables()
    ens = EnsembleSampler(gc._sampler, base_seed=5, concurrent_members=2)
    fields = [_stack(d) for _, d in sorted(ens(inp, tgt.map(np.zeros_like), frc, M), key=lambda t: t[0])]
    ref = R.ensemble(np.stack(fields), _stack(tgt), 13, 24, tabs)
    scores, sp = ens.scores_and_spectra(inp, tgt, frc, M)
    assert isinstance(sp, EnsembleSpectra) and sp.n_members == M and sp.sums.shape == (2, 82, 12, 6)
    _check("sampler", sp.sums.reshape(164, 12, 6), ref["sums"], ref["tol"], R.SUM_NAMES)
    np.testing.assert_array_equal(scores.sums, ens.scores(inp, tgt, frc, M).sums)        # the scores of scores()
    np.testing.assert_array_equal(ens.spectra(inp, tgt, frc, M).sums, sp.sums)
    both = gc.ensemble_spectra(inp, tgt, frc, num_members=M, rngs=5, concurrent_members=2, scores=True)
    np.testing.assert_array_equal(both[1].sums, sp.sums)
    np.testing.assert_array_equal(both[0].sums, scores.sums)
    # the resident sample of the plain sampler
    gc._sampler(inp, tgt.map(np.zeros_like), frc, rngs=3)
    p = gc._sampler.sample_spectrum()
    assert p.shape == (2, 82, 12) and np.isfinite(p).all() and (p >= 0).all()
    want, tol = R.field_spectrum(gc.denoiser.native.download_sample(), 13, 24, tabs)
    _check("sample_spectrum", p.reshape(164, 12), want, tol)
    # physical units through InputsAndResiduals: a^2 on the spectra of the normalised members (every target is an input)
    srng = np.random.default_rng(5)
    def stat(lo, hi):
      names = set(config.TASK.input_variables) | set(config.TASK.target_variables)
      return Dataset({n: (Variable(("level",), srng.uniform(lo, hi, 13).astype(np.float32)) if n in config.ALL_ATMOSPHERIC_VARS
                          else Variable((), np.float32(srng.uniform(lo, hi)))) for n in sorted(names)})
    stats = (stat(0.5, 2.0), stat(-1.0, 1.0), stat(0.1, 0.5))
    norm = rollout.InputsAndResiduals(gc, *stats)
    phys = norm.ensemble_spectra(inp, tgt, frc, num_members=M, rngs=5)
    _, ni, nt, nf = norm._normalized_loss_args(inp, tgt, frc)
    members_n = [_stack(d) for _, d in sorted(EnsembleSampler(gc._sampler, base_seed=5)(ni, nt.map(np.zeros_like), nf, M),
                                              key=lambda t: t[0])]
    a = np.concatenate([rollout._per_channel_stat(stats[2], name, tgt[name], 1.0) for name, _, _ in datasets.channel_layout(tgt)])
    a2 = np.tile(a.astype(np.float64) ** 2, 2)[:, None, None]                             # columns n = b C + c
    refn = R.ensemble(np.stack(members_n), _stack(nt), 13, 24, tabs)
    _check("dataset", phys.sums.reshape(164, 12, 6), refn["sums"] * a2, refn["tol"] * a2 + 4 * R.U * refn["sums"] * a2, R.SUM_NAMES)
    pv = phys.per_variable(tgt)
    assert pv["power_ratio"]["temperature"].shape == (2, 13, 12) and (pv["spread_power"]["temperature"] > 0).all()
    # NaNCleaner on top: nothing to clean here, so the same bytes; with NaN targets the cleaned variable stays finite
    k = "2m_temperature"
    nc = NaNCleaner(norm, k, Dataset({k: Variable((), np.float32(0.25))}))
    np.testing.assert_array_equal(nc.ensemble_spectra(inp, tgt, frc, num_members=M, rngs=5).sums, phys.sums)
    land = np.zeros((13, 24), bool)
    land[2:6, 3:11] = True
    dirty_t = tgt.assign(Dataset({k: Variable(tgt[k].dims, np.where(land, np.nan, tgt[k].data).astype(np.float32))}))
    got = nc.ensemble_spectra(inp, dirty_t, frc, num_members=M, rngs=5)
    assert np.isfinite(got.sums).all() and gc.denoiser.native.counter("spec_invalid_columns") == 0
    assert np.isnan(norm.ensemble_spectra(inp, dirty_t, frc, num_members=M, rngs=5).sums).any()   # uncleaned: NaN columns
  finally:
    gc.denoiser.native.close()


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------
def test_state_and_argument_errors():
  gr = _graph()
  G, B, C = gr.num_grid_nodes, 2, 6
  members, truth = _data(3, G, B, C, seed=41, scale=np.ones(6))
  q, c, s = SphericalAnalysis(*_latlon(13, 24)).device_tables()
  bare = _lib.NativeDenoiser(latent_size=128, d_model=128, num_heads=2, ffw_hidden=256, num_layers=1, c_in=C + 4, c_out=C, batch=B)
  nd = _handle(gr, B, C)
  try:
    with pytest.raises(_lib.GencastHipError, match="gc_set_graph"):
      bare.spec_set_tables(q, c, s)
    with pytest.raises(_lib.GencastHipError, match="tables"):      # nothing handed over yet
      nd.spec_field(truth)
    with pytest.raises(_lib.GencastHipError, match="tables"):
      nd.ens_spectrum(truth)
    with pytest.raises(ValueError, match="n_lat"):                 # another grid
      nd.spec_set_tables(q[:, :, :12], c, s)
    with pytest.raises(ValueError, match="lmax"):                  # a band limit beyond n_lon / 2
      nd.spec_set_tables(np.zeros((13, 13, 13), np.float32), np.zeros((13, 24), np.float32), np.zeros((13, 24), np.float32))
    with pytest.raises(ValueError):
      nd.spec_set_tables(q, c[:5], s[:5])
    nd.spec_set_tables(q, c, s)
    with pytest.raises(_lib.GencastHipError, match="sample"):      # no resident sample (no weights at all)
      nd.spec_field(None)
    with pytest.raises(ValueError):
      nd.spec_field(truth[:, :1])
    with pytest.raises(_lib.GencastHipError, match="member store"):
      nd.ens_spectrum(truth)
    nd.ens_reserve(3)
    for i in (0, 1):
      nd.ens_push_host(i, members[i])
    with pytest.raises(_lib.GencastHipError, match="slot 2"):      # an unfilled slot
      nd.ens_spectrum(truth)
    nd.ens_push_host(2, members[2])
    with pytest.raises(_lib.GencastHipError, match="truth"):       # no truth yet
      nd.ens_spectrum(None)
    with pytest.raises(ValueError):
      nd.ens_spectrum(truth[:-1])
    assert nd.counter("spec_calls") == 0
    nd.ens_spectrum(truth)
    nd.ens_reserve(3)                                              # empties the store
    with pytest.raises(_lib.GencastHipError, match="slot 0"):
      nd.ens_spectrum(None)
    assert nd.counter("spec_calls") == 1
  finally:
    nd.close()
    bare.close()
