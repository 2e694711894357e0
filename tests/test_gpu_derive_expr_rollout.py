"""Derived fields across levels and along the grid through the stack: `EnsembleRollout.run(derived=...)` with an entry of
integrated vapour transport, geopotential thickness and 850 hPa vorticity, and a window over it, on the small model of
tests/test_gpu_events.py (9 x 16 grid with pole rows, batch 2, HORIZON = 2, M = 3, both `norm` settings).

The kept derived members are held to tests/derive_expr_reference.py applied to the kept raw members, within the bound that
file computes.  The scores and the event tables of the view are then compared with verification_reference / event_reference
applied to THOSE kept derived members; the derived truth has no download, so the test forms it by the same device call on two
handles of its own, as tests/test_gpu_derived_rollout.py does, and holds it to the reference too.  That a run without the new
forms makes the recorded calls is tests/test_rollout_call_sequence.py, unchanged; tests/test_derive_expr.py holds what a run
with them hands to its handles."""
import numpy as np
import pytest

from gencast_flax_nnx_amd import DerivedSpec, EventSpec, WindowSpec, rollout, verification
from gencast_flax_nnx_amd.verification import quantize_node_weights
from tests import derive_expr_reference as X
from tests import event_reference as ER
from tests import verification_reference as VR
from tests import window_reference as WR
from tests.test_gpu_derived_rollout import _device_derive
from tests.test_gpu_events import HORIZON, SB, _Setup
from tests.test_gpu_verification import _check_sums

pytestmark = pytest.mark.gpu

M = 3
LEVELS = (50, 100, 150, 200, 250, 300, 400, 500, 600, 700, 850, 925, 1000)
U, V, Q, Z = "u_component_of_wind", "v_component_of_wind", "specific_humidity", "geopotential"


@pytest.fixture(scope="module")
def setup():
  s = _Setup()
  yield s
  s.gc.denoiser.close()


def _specs():
  spec = DerivedSpec([DerivedSpec.ivt("ivt", Q, U, V, LEVELS), DerivedSpec.thickness("thickness", Z, 5, 7), ("vorticity", "vort850", U, V, 10)])
  events = EventSpec({"ivt": np.array([1e4, 3e4, 5e3]), "thickness": np.array([0.0, 0.1, -0.1]), "vort850": np.array([0.0, 2e-7, -2e-7])},
                     [1, 1, -1])
  return spec, events, WindowSpec("max", 2, stride=1, source="moist")


def _check_fields(tag, got, raw, plan):
  ref, bound = X.derive(raw, plan)
  worst = [X.within(got[..., j], ref[..., j], bound[..., j]) for j in range(got.shape[-1])]
  print(f"{tag}: largest error / bound per channel {[f'{w:.2g}' for w in worst]}")


@pytest.mark.parametrize("which", ["wrapper", "none"])
def test_rollout_with_the_new_forms_equals_the_definitions_on_the_kept_members(setup, which):
  spec, events, gust = _specs()
  er = rollout.EnsembleRollout(setup.gc, setup.norm(which), base_seed=3, concurrent_members=2)
  args = (setup.inp, setup.targets, setup.forcings, HORIZON, M)
  res = er.run(*args, keep_members=True, derived={"moist": (spec, events)}, windows={"peak": gust})
  plain = er.run(*args, keep_members=True)
  s, l = setup.stats_per_channel(which)
  w = verification.node_weights(setup.template0)
  wq, wq_scale = quantize_node_weights(w)
  plan = spec.plan(setup.template0, s, l)
  sd, ld = spec.channel_stats(setup.template0, s, l)
  np.testing.assert_array_equal(sd, 1.0)
  np.testing.assert_array_equal(ld, 0.0)
  assert list(plan["op"]) == [3, 2, 4] and plan["pole_row"].sum() == 2 and len(plan["term_coef"]) == 28
  part = res.derived["moist"]
  assert len(part.scores) == len(part.members) == len(part.events) == HORIZON
  thr = events.packed(spec.template(setup.template0))             # physical units, and so are the derived members
  truth_d = []
  for k in range(HORIZON):
    raw, got = np.stack(res.members[k]), np.stack(part.members[k])
    assert got.shape == (M, setup.G, SB, 3) and got.dtype == np.float32 and np.isfinite(got).all()
    _check_fields(f"{which} lead {k}", got, raw, plan)
    g = got.reshape(M, 9, 16, SB, 3)
    assert np.all(g[:, [0, 8], :, :, 2] == g[:, [0, 8], :1, :, 2])                   # one vorticity per pole
    truth_raw = setup.truth(k, which)
    truth_d.append(_device_derive(setup.gc.denoiser.graph, plan, np.stack([truth_raw, truth_raw]))[0])
    _check_fields(f"{which} lead {k} truth", truth_d[k][None], truth_raw[None], plan)
    ref = VR.reference(got, truth_d[k], w)
    sn = part.scores_normalized[k]
    _check_sums(f"{which} lead {k}", sn.sums, sn.rank_histogram, ref, setup.G, M)
    np.testing.assert_array_equal(part.scores[k].sums, sn.scaled(sd).sums)
    tab = ER.tables(got, truth_d[k], thr, events.directions, wq)
    e = part.events[k]
    np.testing.assert_array_equal(e.weighted, tab["weighted"], err_msg=f"{which} lead {k}")
    np.testing.assert_array_equal(e.counts, tab["counts"])
    np.testing.assert_array_equal(e.invalid, tab["invalid"])
    assert e.n_members == M and e.scale == wq_scale
  pv = part.scores[0].per_variable(spec.template(setup.template0))
  assert pv["crps"]["ivt"].shape == pv["crps"]["vort850"].shape == (SB, 1)
  # the window over the view: the maximum over the two leads of the kept derived members, bit for bit
  peak = res.windows["peak"]
  assert peak.leads == [1] and len(peak.members) == 1
  got = np.stack(peak.members[0])
  want = WR.window(np.stack([np.stack(part.members[0]), np.stack(part.members[1])]), WR.MAX)
  assert WR.same_bits(got, want)
  ref = VR.reference(got, WR.window(np.stack(truth_d), WR.MAX), w)
  _check_sums(f"{which} peak", peak.scores_normalized[0].sums, peak.scores_normalized[0].rank_histogram, ref, setup.G, M)
  # everything else of the same run: the bytes of a run without `derived`
  for k in range(HORIZON):
    assert res.scores[k].sums.tobytes() == plain.scores[k].sums.tobytes()
    assert res.scores[k].rank_histogram.tobytes() == plain.scores[k].rank_histogram.tobytes()
    for m in range(M):
      assert res.members[k][m].tobytes() == plain.members[k][m].tobytes()
