"""The f16x3 domain guard at every intermediate operand: the case table shared by tests/test_domain_cases.py (CPU: the
table itself, with the oracle alone) and tests/test_gpu_domain_guard.py (the kernels).

The f16x3 kernels split every matrix operand into fp16 hi / lo halves and never clamp (csrc/gc_dev_common.inc): an
operand beyond +-65504 becomes Inf / NaN, the poison has to reach the output of the call, and one finite check of the
output re-runs the call on the exact-f32 kernels.  That is a claim about every producer -> consumer pair of a forward.  A
case makes ONE of them leave the range by scaling ONE parameter, every weight staying <= 65504 (`weights_f16_unsafe`
stays 0, so the handle does run f16x3):

  out  the targeted operand site reaches >= 2 x 65504 and is the first site in forward order above 65504;
  in   the same parameter scaled less: the targeted site lies in [16384, 60000] and every recorded site is <= 60000;
  nofallback (two cases)  a value that is never split leaves the range (the residual stream, the output): no re-run.

"Site" = an entry of `oracle.gencast_oracle.denoiser_forward(operand_max=...)`: the largest |value| of the left operand
of a matrix product, keyed by the parameter path of the kernel it multiplies, plus q / k / v and the residual stream per
block.  The scales are not written down anywhere: `evaluate` derives them from the recorder (see there).

Static embedders, site (k): their inputs are 3 or 4 structural features with |value| <= 1 and the first-layer kernel is
scaled as a whole, so with every weight <= 65504 the hidden activation cannot exceed (sum over the live input rows of
|feature| x 65504).  With the weights of `weights.random_params` the reach is 1.02 (mesh nodes), 1.24 (grid2mesh
edges) and 1.49 (mesh2grid edges) x 65504 at shape A: 2 x 65504 does not exist for these rows.  Their out case takes
the largest scale the weight bound allows, and the floor asserted for the site is `STATIC_OUT_FLOOR` = 65520 (the
smallest float32 that rounds to fp16 infinity) + 1 %: 1e5 float32 roundings of the site's value away from the threshold.

Shapes (the smallest that select each kernel form; `Case.form` says what a row is there for):
  A  tiny_setup default, latent 128, ffw 256: 4-wave weight-streaming MLP, fused FFW (1 slab), QKV plane epilogue,
     out-projection with row pass, mesh2grid triple-sum epilogue; re-run on the weight-streaming exact-f32 family
  B  latent 128, 1 head of 128, ffw 384: FFW-1 a weight-streaming GEMM with gelu, FFW-2 the LDS-staged f16 GEMM;
     f32_ws is false, so the re-run takes the LDS-staged exact-f32 family
  C  latent 256, 2 heads of 128, ffw 512: 8-wave MLP forms, the paired grid2mesh launch, two FFW slabs
  D  latent 512, 4 heads, ffw 512, mesh 2: split edge MLPs (per-node GEMMs + add terms), the 64-row MLP, FFW as two
     weight-streaming GEMMs
  Cq, Dq  C and D on a 42-node mesh (mesh 1, 1-hop) for the q / k / v rows: at 162 nodes the softmax over logits of 1e5
     is an arg-max that near ties decide differently in float32 (float32 against float64 oracle 3e-5 .. 6e-5, over the
     1e-5 every row must meet), so those rows were replaced.  Attention on 162 nodes sees an out-of-range q / k at A only.
  E  37 x 72 grid, batch 4, latent 128: 31 968 mesh2grid edge rows >= kMlpMt2Rows, the 64-row form of the 4-wave MLP
Every site runs at A; at B..E a site runs only where its consuming kernel form differs from A's.

fp16-feature mode is out of scope: there an overflow is the reference's own behaviour.
"""
import dataclasses
import functools

import numpy as np

from oracle import gencast_oracle as O
from tests import helpers

F16_MAX = 65504.0
OUT_FLOOR = 2 * F16_MAX                      # out: the targeted site reaches this ...
OUT_GOAL = 3 * F16_MAX                       # ... by aiming here
STATIC_OUT_FLOOR = 65520.0 * 1.01            # site (k): see the module docstring
IN_LO, IN_HI = 16384.0, 60000.0              # in: the targeted site lies in [IN_LO, IN_HI], every site <= IN_HI
IN_GOAL = 48000.0                            # ... by putting the largest site here
PROBE_SCALE = 1.0e4                          # where the recorder is read to derive the scales
TOL = 1e-4                                   # the project's bound (tests/test_gpu_parity.py)

SHAPES = {
    "A": dict(batch=2),
    "B": dict(batch=3, seed=7, latent=128, heads=1, ffw=384, layers=2, k_hop=3, mesh_size=2),
    "C": dict(batch=1, seed=7, latent=256, heads=2, ffw=512, layers=1, k_hop=2, mesh_size=2),
    "D": dict(batch=1, seed=7, latent=512, heads=4, ffw=512, layers=1, k_hop=2, mesh_size=2),
    "Cq": dict(batch=1, seed=7, latent=256, heads=2, ffw=512, layers=1, k_hop=1, mesh_size=1),
    "Dq": dict(batch=1, seed=7, latent=512, heads=4, ffw=512, layers=1, k_hop=1, mesh_size=1),
    "E": dict(batch=4, seed=7, latent=128, heads=2, ffw=256, layers=1, k_hop=2, mesh_size=2, n_lat=37, n_lon=72),
}

# ---- parameter paths (weights.random_params) ----------------------------------------------------------------------
_EMB1 = f"{O.P_G2M}.embedder_network"
_GN1 = f"{O.P_G2M}.processor_networks.0.graph_network"
_GN2 = f"{O.P_M2G}.processor_networks.0.graph_network"
MLP = dict(
    grid_embed=f"{_EMB1}.embed_node_fns.grid_nodes",
    mesh_embed=f"{_EMB1}.embed_node_fns.mesh_nodes",
    g2m_edge_embed=f"{_EMB1}.embed_edge_fns.grid2mesh",
    g2m_edge=f"{_GN1}.update_edge_fns.grid2mesh.edge_fn",
    g2m_mesh=f"{_GN1}.update_node_fns.mesh_nodes.node_fn",
    g2m_grid=f"{_GN1}.update_node_fns.grid_nodes.node_fn",
    m2g_edge_embed=f"{O.P_M2G}.embedder_network.embed_edge_fns.mesh2grid",
    m2g_edge=f"{_GN2}.update_edge_fns.mesh2grid.edge_fn",
    m2g_grid=f"{_GN2}.update_node_fns.grid_nodes.node_fn",
    decoder=f"{O.P_M2G}.decoder_network.embed_node_fns.grid_nodes",
)
w1 = lambda mlp: f"{MLP[mlp]}.network.network.layers.0.kernel"
w2 = lambda mlp: f"{MLP[mlp]}.network.network.layers.2.kernel"
wc = lambda mlp: f"{MLP[mlp]}.norm_conditioning_layer.conditional_linear_layer.kernel"
blk = lambda i, rest: f"{O.P_TR}.blocks.{i}.{rest}"
proj = lambda i, which: blk(i, f"attn_module.{which}_proj.linear.kernel")
ffw = lambda i, layer: blk(i, f"ffw_module.mlp.layers.{layer}.kernel")
ncond = lambda i, which: blk(i, f"{which}.conditional_linear_layer.kernel")
FINAL_COND = f"{O.P_TR}.final_norm_cond.conditional_linear_layer.kernel"


@dataclasses.dataclass(frozen=True)
class Case:
  id: str          # "<shape>-<site letter>-<what>"
  shape: str       # key of SHAPES
  param: str       # the one parameter that is scaled
  site: str        # the recorder entry meant to leave the range ("y": the output itself)
  consumer: str    # the kernel that consumes that operand
  form: str        # the kernel form this row is there for
  kind: str = "pair"            # "pair": an out and an in case; "nofallback": one case that must not re-run
  static: bool = False          # site (k): the operand lives in compute_static_embeddings, not in the call

  @property
  def out_floor(self):
    return STATIC_OUT_FLOOR if self.static else OUT_FLOOR


def _c(shape, letter, what, param, site, consumer, form, **kw):
  return Case(f"{shape}-{letter}-{what}", shape, param, site, consumer, form, **kw)


def _static_cases(shape, names, form):
  return [_c(shape, "k", f"{n}_hidden", w1(n), w2(n), "second layer of the fused MLP, at gc_finalize", form, static=True)
          for n in names]


CASES = [
    # ---- A: every site --------------------------------------------------------------------------------------------
    _c("A", "a", "grid_embed_hidden", w1("grid_embed"), w2("grid_embed"), "second layer of the fused MLP (hidden in LDS)",
       "4-wave weight-streaming MLP, 32 rows"),
    _c("A", "b", "g2m_edge_hidden", w1("g2m_edge"), w2("g2m_edge"), "second layer of the fused MLP", "4-wave MLP, 3 gathered segments"),
    _c("A", "c", "g2m_mesh_hidden", w1("g2m_mesh"), w2("g2m_mesh"), "second layer of the fused MLP", "4-wave MLP, 2 segments + residual"),
    _c("A", "d", "q", proj(0, "q"), blk(0, "q"), "attention (splits q per tile, no check)", "QKV plane epilogue, heads of 64"),
    _c("A", "e", "k", proj(1, "k"), blk(1, "k"), "attention (reads the fp16 planes)", "QKV plane epilogue, heads of 64"),
    _c("A", "f", "v", proj(0, "v"), blk(0, "v"), "attention (reads the fp16 planes)", "QKV plane epilogue, heads of 64"),
    _c("A", "g", "ffw_hidden", ffw(0, 0), ffw(0, 2), "second product of the fused FFW (hidden in LDS)", "fused FFW, 1 slab"),
    _c("A", "h", "h_attn", ncond(0, "norm_cond_attn"), proj(0, "q"), "QKV projection", "row pass -> weight-streaming GEMM, plane epilogue"),
    _c("A", "h", "h_ffw", ncond(1, "norm_cond_ffw"), ffw(1, 0), "first product of the fused FFW",
       "out-projection with row pass -> fused FFW"),
    _c("A", "h", "m2", FINAL_COND, w1("m2g_edge"), "mesh2grid edge MLP, gathered segment", "final row pass -> 4-wave MLP, triple-sum epilogue"),
    _c("A", "i", "agg1", wc("g2m_edge"), w1("g2m_mesh"), "grid2mesh mesh-node MLP, segment 1", "edge MLP -> segment-sum launch -> 4-wave MLP"),
    _c("A", "i", "agg2", wc("m2g_edge"), w1("m2g_grid"), "mesh2grid grid-node MLP, segment 1", "triple-sum epilogue -> 4-wave MLP"),
    _c("A", "j", "decoder_hidden", w1("decoder"), w2("decoder"), "second layer of the fused MLP", "4-wave MLP, no LayerNorm, n_out 6"),
    *_static_cases("A", ["mesh_embed", "g2m_edge_embed", "m2g_edge_embed"], "4-wave MLP, broadcast segment"),
    _c("A", "n", "residual_stream", ffw(0, 2), blk(0, "x"), "float32 row pass only", "fused FFW slabs -> row pass", kind="nofallback"),
    _c("A", "n", "output", w2("decoder"), "y", "nothing (the result)", "decoder MLP output", kind="nofallback"),
    # ---- B: the GEMM forms of the FFW, the LDS-staged exact-f32 re-run ----------------------------------------------
    _c("B", "g", "ffw_hidden", ffw(0, 0), ffw(0, 2), "FFW-2", "LDS-staged f16 GEMM; re-run on the LDS-staged exact-f32 family"),
    _c("B", "h", "h_ffw", ncond(1, "norm_cond_ffw"), ffw(1, 0), "FFW-1", "weight-streaming GEMM with gelu"),
    # ---- C: the 8-wave MLP forms, the paired launch, two FFW slabs ---------------------------------------------------
    _c("C", "a", "grid_embed_hidden", w1("grid_embed"), w2("grid_embed"), "second layer of the fused MLP", "8-wave MLP, 32 rows"),
    _c("C", "b", "g2m_edge_hidden", w1("g2m_edge"), w2("g2m_edge"), "second layer of the fused MLP", "paired launch, edge half"),
    _c("C", "c", "g2m_mesh_hidden", w1("g2m_mesh"), w2("g2m_mesh"), "second layer of the fused MLP", "8-wave MLP, 2 segments + residual"),
    _c("Cq", "d", "q", proj(0, "q"), blk(0, "q"), "attention", "QKV plane epilogue, heads of 128"),
    _c("Cq", "e", "k", proj(0, "k"), blk(0, "k"), "attention", "QKV plane epilogue, heads of 128"),
    _c("Cq", "f", "v", proj(0, "v"), blk(0, "v"), "attention", "QKV plane epilogue, heads of 128"),
    _c("C", "g", "ffw_hidden", ffw(0, 0), ffw(0, 2), "second product of the fused FFW", "fused FFW, 2 slabs"),
    _c("C", "i", "agg1", wc("g2m_edge"), w1("g2m_mesh"), "grid2mesh mesh-node MLP, segment 1", "paired launch -> segment sum -> 8-wave MLP"),
    _c("C", "i", "agg2", wc("m2g_edge"), w1("m2g_grid"), "mesh2grid grid-node MLP, segment 1", "triple-sum epilogue of the 8-wave MLP"),
    _c("C", "j", "decoder_hidden", w1("decoder"), w2("decoder"), "second layer of the fused MLP", "8-wave MLP, 4 output waves"),
    *_static_cases("C", ["g2m_edge_embed"], "8-wave MLP, broadcast segment"),
    # ---- D: split edge MLPs, the 64-row MLP, FFW as two weight-streaming GEMMs ---------------------------------------
    _c("D", "a", "grid_embed_hidden", w1("grid_embed"), w2("grid_embed"), "second layer of the fused MLP", "latent 512: 8 waves x 64 rows"),
    _c("D", "b", "g2m_edge_hidden", w1("g2m_edge"), w2("g2m_edge"), "second layer of the fused MLP",
       "split edge MLP: node products as float32 add terms, paired launch"),
    _c("Dq", "e", "k", proj(0, "k"), blk(0, "k"), "attention", "QKV n = 1536, 4 heads of 128"),
    _c("D", "g", "ffw_hidden", ffw(0, 0), ffw(0, 2), "FFW-2", "weight-streaming GEMM, split-K slabs"),
    _c("D", "h", "h_ffw", ncond(0, "norm_cond_ffw"), ffw(0, 0), "FFW-1", "weight-streaming GEMM with gelu, d_model 512"),
    _c("D", "h", "m2", FINAL_COND, w1("m2g_edge"), "per-node GEMM of the split mesh2grid edge MLP", "weight-streaming node GEMM -> add terms"),
    _c("D", "i", "agg2", wc("m2g_edge"), w1("m2g_grid"), "mesh2grid grid-node MLP, segment 1", "triple-sum epilogue of the split edge MLP"),
    _c("D", "j", "decoder_hidden", w1("decoder"), w2("decoder"), "second layer of the fused MLP", "latent 512, n_out_pad 128 form"),
    *_static_cases("D", ["m2g_edge_embed"], "latent 512 MLP, broadcast segment"),
    # ---- E: the 64-row form of the 4-wave MLP -----------------------------------------------------------------------
    _c("E", "b", "m2g_edge_hidden", w1("m2g_edge"), w2("m2g_edge"), "second layer of the fused MLP",
       "31 968 rows >= kMlpMt2Rows: 4 waves x 64 rows, triple-sum epilogue"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
PAIRS = [c for c in CASES if c.kind == "pair"]
NOFALLBACK = [c for c in CASES if c.kind == "nofallback"]


@functools.lru_cache(maxsize=None)
def setup(shape):
  """(graph, dims, params, x, sigma, graph dict, attention function) of a shape; shared, never modified."""
  cfg = dict(SHAPES[shape])
  gr, dims, params, x, sigma = helpers.tiny_setup(**cfg)
  g = helpers.graph_dict(gr)
  return gr, dims, params, x, sigma, g, O.make_attention_fn(g, "dense")


def scaled_params(case, scale):
  params = dict(setup(case.shape)[2])
  params[case.param] = (params[case.param].astype(np.float64) * scale).astype(np.float32)
  return params


def forward(case, params, x=None, sigma=None, **kw):
  gr, dims, _, x0, sigma0, g, attn = setup(case.shape)
  return O.denoiser_forward(params, g, x0 if x is None else x, sigma0 if sigma is None else sigma,
                            num_layers=dims.num_layers, num_heads=dims.num_heads, attention=attn, **kw)


def operand_sites(rec):
  """The recorder's entries that are operands (the residual stream `...x` is recorded but never split)."""
  return {k: v for k, v in rec.items() if not k.endswith(".x")}


def _measure(case, scale):
  rec = {}
  params = scaled_params(case, scale)
  y = forward(case, params, operand_max=rec)
  return dict(scale=scale, params=params, rec=rec, y=y)


def site_value(case, res):
  """The magnitude a case is about, in an `evaluate` result: a recorder entry, or max |output| for site "y"."""
  return float(np.abs(res["y"]).max()) if case.site == "y" else res["rec"][case.site]


@functools.lru_cache(maxsize=None)
def evaluate(case_id, which):
  """The case `which` ("out", "in" or "nofallback") of a table row, from the recorder alone:

  the recorder is read once at scale PROBE_SCALE, where the scaled parameter dominates its bias and every site downstream
  of it is proportional to the scale (swish and gelu are positively homogeneous out there, LayerNorm ends the
  dependence); then
    out / nofallback  scale = PROBE x OUT_GOAL / site(PROBE), capped at the largest scale that keeps every weight <= 65504
    in                scale = PROBE x IN_GOAL / (largest recorded site at PROBE that moved with the scale)
  and the forward is evaluated again at that scale.  Returns dict(scale, params, rec, y) of that evaluation:
  float32 parameters as the handle gets them, the recorder's dict, the float64 output."""
  case = BY_ID[case_id]
  probe, base = _probe(case_id)
  if which == "in":
    moved = [v for k, v in probe["rec"].items() if v > 2.0 * base["rec"].get(k, 0.0)]
    scale = PROBE_SCALE * IN_GOAL / max(moved)
  else:
    scale = PROBE_SCALE * OUT_GOAL / site_value(case, probe)
    wmax = float(np.abs(setup(case.shape)[2][case.param]).max())
    scale = min(scale, F16_MAX / wmax * (1.0 - 2.0 ** -20))
  return _measure(case, scale)


@functools.lru_cache(maxsize=None)
def _probe(case_id):
  case = BY_ID[case_id]
  return _measure(case, PROBE_SCALE), _unscaled(case.shape)


@functools.lru_cache(maxsize=None)
def _unscaled(shape):
  return _measure(next(c for c in CASES if c.shape == shape), 1.0)


def first_site_above(rec, bound=F16_MAX):
  """The first operand site in forward order above `bound`, or None."""
  return next((k for k, v in operand_sites(rec).items() if v > bound), None)
