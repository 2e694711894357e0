"""The case table of the f16x3 domain-guard tests (tests/domain_cases.py), checked with the oracle alone: every row does
to the operand magnitudes what it says, has a finite float64 answer, and is a question any float32 implementation can
answer to a tenth of the project's tolerance -- so a failure of tests/test_gpu_domain_guard.py is the kernels'."""
import numpy as np
import pytest

from oracle import gencast_oracle as O
from tests import domain_cases as DC


def _well_conditioned(case, res):
  y32 = DC.forward(case, res["params"], dtype=np.float32)
  err = float(np.abs(y32 - res["y"]).max())
  bound = DC.TOL / 10 * max(1.0, float(np.abs(res["y"]).max()))
  print(f"{case.id}: scale {res['scale']:.6g}, site {DC.site_value(case, res):.6g}, max|y| {np.abs(res['y']).max():.4g}, "
        f"float32 - float64 {err:.3g} (bound {bound:.3g})")
  assert np.isfinite(res["y"]).all()
  assert err <= bound, (case.id, err, bound)


def _weights_in_range(res):
  assert max(float(np.abs(v).max()) for v in res["params"].values()) <= DC.F16_MAX      # weights_f16_unsafe must read 0


def test_the_recorder_changes_nothing_and_lists_every_operand_in_forward_order():
  gr, dims, params, x, sigma, g, attn = DC.setup("A")
  kw = dict(num_layers=dims.num_layers, num_heads=dims.num_heads, attention=attn)
  rec = {}
  y = O.denoiser_forward(params, g, x, sigma, operand_max=rec, **kw)
  np.testing.assert_array_equal(y, O.denoiser_forward(params, g, x, sigma, **kw))
  kernels = [k for k in params if k.endswith(".kernel")]
  assert set(kernels) <= set(rec)                                          # every kernel multiplies a recorded operand
  extra = [k for k in rec if k not in params]
  assert extra == [DC.blk(i, n) for i in range(dims.num_layers) for n in ("q", "k", "v", "x")]
  order = list(rec)
  before = lambda a, b: order.index(a) < order.index(b)
  assert before(DC.w1("grid_embed"), DC.w2("grid_embed")) and before(DC.w2("g2m_edge"), DC.w1("g2m_mesh"))
  assert before(DC.w2("g2m_grid"), DC.proj(0, "q")) and before(DC.proj(0, "v"), DC.blk(0, "q"))
  assert before(DC.blk(0, "x"), DC.ffw(0, 0)) and before(DC.ffw(1, 2), DC.FINAL_COND)
  assert before(DC.FINAL_COND, DC.w1("m2g_edge")) and order[-1] == DC.w2("decoder")
  # known magnitudes: the Fourier features are sines and cosines, the grid embedder's operand is [structure | x]
  assert rec[f"{O.P_NOISE}.linear_0.kernel"] <= 1.0
  assert rec[DC.w1("grid_embed")] == max(float(np.abs(x).max()), float(np.abs(gr.grid_struct).max()))
  assert O._REC is None and not O._REC_NAMES                               # nothing left switched on


def test_the_table_covers_what_it_says():
  ids = [c.id for c in DC.CASES]
  for letter in "abcdefghijk":
    assert any(i.startswith(f"A-{letter}-") for i in ids), letter              # every site runs at A
  assert sum(c.static for c in DC.CASES if c.shape == "A") == 3               # the three static embedders
  assert len(DC.NOFALLBACK) == 2
  for c in DC.CASES:
    assert c.param in DC.setup(c.shape)[2] and c.form and c.consumer


@pytest.mark.parametrize("case_id", [c.id for c in DC.PAIRS])
def test_out_case(case_id):
  case, res = DC.BY_ID[case_id], DC.evaluate(case_id, "out")
  _weights_in_range(res)
  assert DC.site_value(case, res) >= case.out_floor
  assert DC.first_site_above(res["rec"]) == case.site
  _well_conditioned(case, res)


@pytest.mark.parametrize("case_id", [c.id for c in DC.PAIRS])
def test_in_case(case_id):
  case, res = DC.BY_ID[case_id], DC.evaluate(case_id, "in")
  _weights_in_range(res)
  assert DC.IN_LO <= DC.site_value(case, res) <= DC.IN_HI
  assert max(res["rec"].values()) <= DC.IN_HI
  assert res["scale"] < DC.evaluate(case_id, "out")["scale"]
  _well_conditioned(case, res)


@pytest.mark.parametrize("case_id", [c.id for c in DC.NOFALLBACK])
def test_nofallback_case(case_id):
  case, res = DC.BY_ID[case_id], DC.evaluate(case_id, "nofallback")
  _weights_in_range(res)
  assert DC.site_value(case, res) >= DC.OUT_FLOOR                             # the residual stream / the output leaves the range
  assert max(DC.operand_sites(res["rec"]).values()) <= DC.IN_HI               # ... and no operand does
  _well_conditioned(case, res)
