"""The algebra of the edge-term route ("edge terms"), in NumPy float64 against the oracle.

The first layer of an edge MLP is `concat([e, n[senders], n[receivers]]) @ W1 + b1`.  Split by input block it is
`T + P_snd[senders] + P_rcv[receivers] + b1` with `T = e @ W1[:L]`, `P_snd = n_snd @ W1[L:2L]`, `P_rcv = n_rcv @ W1[2L:]`,
and `e` -- a static embedding under the conditioning affine -- depends on the noise level alone, so `T` does too."""
import numpy as np
import pytest

from oracle import gencast_oracle as O
from tests import helpers

EDGES = 40            # a few dozen edges of each edge set are enough for the algebra


@pytest.fixture(scope="module")
def stages():
  gr, dims, params, x, _ = helpers.tiny_setup(batch=1, seed=7)
  gd = helpers.graph_dict(gr)
  p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
  out = {}
  for sigma in (0.05, 11.0):
    for tag, feats in (("x", x), ("other", x[::-1] * 0.5)):
      _, inter = O.denoiser_forward(params, gd, feats, np.array([sigma], np.float32), num_layers=dims.num_layers,
                                    num_heads=dims.num_heads, attention="neighbour", return_intermediates=True)
      out[sigma, tag] = inter
  return gr, dims, p64, out


CASES = [("grid2mesh", O.P_G2M, "e0", "g0", "m0", "g2m_senders", "g2m_receivers"),
         ("mesh2grid", O.P_M2G, "f0", "m2", "g1", "m2g_senders", "m2g_receivers")]


@pytest.mark.parametrize("sigma", [0.05, 11.0])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_first_layer_is_the_sum_of_an_edge_term_and_two_node_terms(stages, case, sigma):
  gr, dims, p, out = stages
  name, gnn, e_key, snd_key, rcv_key, snd_name, rcv_name = case
  L = dims.latent
  base = f"{gnn}.processor_networks.0.graph_network.update_edge_fns.{name}.edge_fn.network.network.layers.0"
  W1, b1 = p[base + ".kernel"], p[base + ".bias"]
  assert W1.shape == (3 * L, L)
  inter = out[sigma, "x"]
  snd, rcv = getattr(gr, snd_name)[:EDGES], getattr(gr, rcv_name)[:EDGES]
  e, n_snd, n_rcv = inter[e_key][:EDGES], inter[snd_key], inter[rcv_key]
  # the oracle's first layer: one product over the 3 L-wide concatenation (typed_graph_net.py:303)
  want = O.linear(np.concatenate([e, n_snd[snd], n_rcv[rcv]], axis=-1), W1, b1)
  T = O.linear(e, W1[:L])
  P_snd, P_rcv = O.linear(n_snd, W1[L:2 * L]), O.linear(n_rcv, W1[2 * L:])
  got = ((T + P_snd[snd]) + P_rcv[rcv]) + b1            # the order the kernel adds in
  assert got.shape == want.shape == (EDGES, 1, L)
  assert np.abs(got - want).max() < 1e-12 * max(1.0, np.abs(want).max())
  # the edge block sees the noise level alone: other grid inputs, the same conditioned embedding, bit for bit
  np.testing.assert_array_equal(out[sigma, "other"][e_key], inter[e_key])
  assert np.abs(out[sigma, "other"][snd_key] - n_snd).max() > 1e-3       # ... while the node blocks follow the state


def test_the_conditioned_mesh_embedding_follows_the_noise_level_alone(stages):
  _, _, _, out = stages
  for sigma in (0.05, 11.0):
    np.testing.assert_array_equal(out[sigma, "other"]["m0"], out[sigma, "x"]["m0"])
  assert np.abs(out[0.05, "x"]["m0"] - out[11.0, "x"]["m0"]).max() > 1e-3
  assert np.abs(out[0.05, "x"]["e0"] - out[11.0, "x"]["e0"]).max() > 1e-3
