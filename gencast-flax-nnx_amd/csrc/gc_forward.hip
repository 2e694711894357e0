// One denoiser forward on the device: its route (which kernel build, which weight image, which kernel form -- decided
// once per forward), one launcher per kernel form, the MLP call, forward() and the static embeddings.
#include "gc_handle.h"

namespace gci {

// gc_a16 = the same kernels compiled a second time (gc_kernels.hip with -DGC_TU_A16): 2 MFMAs per product for
// exact-fp16 activation operands.  Its argument structs are the same declarations in another namespace.
template <class To, class From>
static const To& a16_view(const From& v) {
  static_assert(sizeof(To) == sizeof(From), "argument struct mismatch between the two kernel builds");
  return reinterpret_cast<const To&>(v);
}

// The route of the forward that would be enqueued now.  Precision: f16x3 unless switched off, unsafe for the weights,
// or re-running a poisoned call (in_fallback); the exact-f32 family takes the same launch structure on WF32 images
// where the shapes allow it (f32_ws; precision can be switched after gc_finalize).
// st16, "fp16 node features" with PHYSICAL 2-byte activation storage (BASELINE.json configs[4]): every kernel of the call
// must then be the gc_a16 / H16 form that reads and writes halfs, so it is all or nothing -- when a shape would put
// an LDS-staged kernel on the path (and during the exact-f32 re-run of the f16x3 domain guard, and with
// GC_TUNE_A16=0) the mode runs on float32 containers with the rounding flags instead (same values).
Route make_route(const gc_handle* h) {
  const int D = h->cfg.d_model, F = h->cfg.ffw_hidden;
  Route r;
  r.f16 = h->f16x3 && !h->weights_f16_unsafe && !h->in_fallback;
  r.x32 = !r.f16 && h->f32_ws;
  const bool streams = r.f16 || r.x32;          // the weight-streaming MLP / fused kernels have images to read
  r.ffw_slabs = streams ? h->ffw_fused_slabs : 0;
  r.st16 = h->feat16 && h->a16 && r.f16 && D % 128 == 0 && D <= 512 &&
           (h->ffw_fused_slabs > 0 || (F % 128 == 0 && (F / h->ffw2_splits) % 128 == 0));   // else: both FFW layers as weight-streaming GEMMs
  // f16x3: the projection hands K and V to attention already split into fp16 hi / lo planes
  r.v2 = r.f16 && r.ws(3 * D, D, 1);
  // attention as a work-item list (build_attention_items): needs the out-projection whose loader merges
  r.att_items = (h->att_n_items > 0 && r.ws(3 * D, D, 1) && h->attn_splits == 1 && D <= 512) ? h->att_n_items : 0;
  r.fuse_row = streams && D % 128 == 0 && D <= 512;
  r.node_ws = r.f16;
  r.split_edge = h->split_edge;
  r.try_pair = h->mlp_pair && h->hidden_layers == 1;
  // The sum of every grid node's 3 updated edges inside the edge MLP: the reference's edge set (3 edges per grid node,
  // sorted by receiver: HostGraph::m2g_tri), one launch per MLP, the weight-streaming kernel (build_mlp_args checks)
  r.m2g_fused = h->m2g_fuse_sum && h->hg.m2g_tri && h->hidden_layers == 1 && streams;
  // inside a sample (embed_cache_live): the noisy block on the weight-streaming kernel; fp16 node features round the
  // staged inputs and keep the one-launch form
  r.embed_cache = h->embed_cache_live && h->embed_cache_ready && !h->feat16 && h->hidden_layers == 1 && streams;
  // inside a sample whose noise levels have their terms cached (ensure_edge_terms built them for this very list)
  r.edge_terms = h->embed_cache_live && h->terms.ready && edge_terms_possible(h) && r.f16;
  return r;
}

// What the edge-term route needs of the handle, whatever the noise levels: f16x3 (the exact-f32 family -- precision = f32,
// the re-run of the domain guard -- keeps the products), float32 features, one hidden layer, latent 256 (the forms the
// product-free first layer is built in), batch 1, the reference's mesh2grid edge set (3 edges per grid node; their sum in
// the edge MLP's epilogue or, GC_TUNE_M2G_FUSE_SUM=0, as a launch of its own: the same bits).  GC_TUNE_EDGE_TERMS=0
// switches it off.
bool edge_terms_possible(const gc_handle* h) {
  return h->edge_terms && h->f16x3 && !h->weights_f16_unsafe && !h->in_fallback && !h->feat16 && h->hidden_layers == 1 &&
         h->cfg.latent_size == 256 && h->cfg.batch == 1 && h->hg.m2g_tri;
}

static gc::Segment seg(const float* ptr, const int* index, const float* affine, int width, int ld, int bcast) {
  gc::Segment s;
  s.ptr = ptr; s.index = index; s.affine = affine; s.width = width; s.ld = ld; s.bcast = bcast;
  return s;
}

// One MLP of the GNNs as the caller describes it; what the route and the weights add is build_mlp_args' business.
struct MlpCall {
  gc::Segment seg[3] = {};             // input column blocks, concatenated along K
  gc::AddTerm add[3] = {};             // products added to the first layer (split edge MLP, embed cache, edge terms)
  int nseg = 0, nadd = 0, rows = 0, B = 1, ldo = 0;
  bool ln = true, cond = true;         // LayerNorm; conditioning (where the MLP has one)
  const float* residual = nullptr;
  float* out = nullptr;
  bool round_out = true;               // fp16 features: round the LayerNorm + conditioning output
  bool seg0_f32 = false, out_f32 = false;   // fp16 storage: segment 0 / out stay float32
  bool tri = false;                    // triple-sum epilogue (mesh2grid fused sum)
  MlpCall& segments(std::initializer_list<gc::Segment> l) { for (const auto& s : l) seg[nseg++] = s; return *this; }
  MlpCall& add_terms(std::initializer_list<gc::AddTerm> l) { for (const auto& t : l) add[nadd++] = t; return *this; }
};
static MlpCall mlp_call(std::initializer_list<gc::Segment> segs, int rows, int B, float* out, int ldo,
                        const float* residual = nullptr) {
  MlpCall c;
  c.rows = rows; c.B = B; c.out = out; c.ldo = ldo; c.residual = residual;
  return c.segments(segs);
}

// Arguments of one fused-MLP launch on the route being enqueued (h->route).
static int build_mlp_args(gc_handle* h, const DevMlp& w, const MlpCall& c, gc::MlpArgs* out_args) {
  const Route& r = h->route;
  gc::MlpArgs& a = *out_args;
  a = gc::MlpArgs{};
  a.nseg = c.nseg; a.nadd = c.nadd;
  std::copy(c.seg, c.seg + c.nseg, a.seg);
  std::copy(c.add, c.add + c.nadd, a.add);
  a.rows = c.rows; a.B = c.B; a.hidden = h->cfg.latent_size;
  a.f16 = r.f16 ? 1 : 0;
  // with add terms only one block of W1 multiplies the staged input: the edge block, or the grid embedding's noisy block
  const Weight& w1 = c.nadd ? w.w1e : w.w1;
  a.w1t = pick(w1, r, Form::Staged); a.ldw1 = w1.ld; a.b1 = w.b1;
  a.w2t = pick(w.w2, r, Form::Staged); a.b2 = w.b2;
  if (r.f16 || r.x32) {
    a.w1f = pick(w1, r, Form::Streaming); a.k1f = w1.kf;
    a.w2f = pick(w.w2, r, Form::Streaming); a.ones = h->d_ones; a.zeros = h->d_zeros;
    a.f32w = r.x32 ? 1 : 0;
  }
  a.n_out = w.n_out; a.n_out_pad = w.n_out_pad; a.do_ln = c.ln ? 1 : 0;
  a.cond = (c.cond && w.cond_off >= 0) ? (h->cond_cur ? h->cond_cur : h->d_cond) + w.cond_off : nullptr;
  a.cond_stride = h->cond_total;
  a.residual = c.residual; a.out = c.out; a.ldo = c.ldo;
  a.round16 = h->feat16 ? 1 : 0;
  a.round_out = (h->feat16 && c.round_out) ? 1 : 0;
  a.a16 = r.st16 ? 1 : 0;
  a.seg0_f32 = c.seg0_f32 ? 1 : 0;
  a.out_f32 = c.out_f32 ? 1 : 0;
  a.tri = c.tri ? 1 : 0;
  if (c.tri && !gc::mlp_runs_weight_streaming(a))
    return fail(h, GC_ERR_INTERNAL, "the triple-sum epilogue exists in the weight-streaming MLP kernel only");
  return GC_OK;
}

// ---- one launcher per kernel form: the event bracketing, and the gc_a16 build where the arguments ask for it ----
static int enqueue_mlp(gc_handle* h, const gc::MlpArgs& a) {
  return launch(h, gc::KC_MLP, [&] {
    return a.a16 ? gc_a16::launch_mlp(h->stream, a16_view<gc_a16::MlpArgs>(a)) : gc::launch_mlp(h->stream, a);
  });
}
static int enqueue_mlp_pair(gc_handle* h, const gc::MlpArgs& a, const gc::MlpArgs& b) {
  return launch(h, gc::KC_MLP, [&] {
    return a.a16 ? gc_a16::launch_mlp_pair(h->stream, a16_view<gc_a16::MlpArgs>(a), a16_view<gc_a16::MlpArgs>(b))
                 : gc::launch_mlp_pair(h->stream, a, b);
  });
}
static int enqueue_gemm_ws(gc_handle* h, int cls, const gc::GemmArgs& ga, int mt, int splits, int epi) {
  return launch(h, cls, [&] {
    return ga.a16 ? gc_a16::launch_gemm_ws(h->stream, cls, a16_view<gc_a16::GemmArgs>(ga), mt, splits, epi)
                  : gc::launch_gemm_ws(h->stream, cls, ga, mt, splits, epi);
  });
}
static int enqueue_gemm_rowop(gc_handle* h, int cls, const gc::GemmArgs& ga, const gc::RowFuse& rf) {
  return launch(h, cls, [&] {
    return ga.a16 ? gc_a16::launch_gemm_rowop(h->stream, cls, a16_view<gc_a16::GemmArgs>(ga), a16_view<gc_a16::RowFuse>(rf))
                  : gc::launch_gemm_rowop(h->stream, cls, ga, rf);
  });
}
static int enqueue_ffw_fused(gc_handle* h, const gc::FfwArgs& fa) {
  return launch(h, gc::KC_GEMM_FFW1, [&] {
    return fa.a16 ? gc_a16::launch_ffw_fused(h->stream, a16_view<gc_a16::FfwArgs>(fa)) : gc::launch_ffw_fused(h->stream, fa);
  });
}

static int run_mlp_one(gc_handle* h, const DevMlp& w, const MlpCall& c) {
  gc::MlpArgs a{};
  if (int rc = build_mlp_args(h, w, c, &a)) return rc;
  return enqueue_mlp(h, a);
}

// One MLPWithNormConditioning / MLP of the GNNs.  hidden_layers == 1 (the reference's trained configuration): one
// fused launch.  hidden_layers >= 2: the leading (Linear -> activation) layers run first, one launch each, handing a
// [rows][latent] float32 array over (gathers / concatenation happen in the first launch only).
static int run_mlp(gc_handle* h, const DevMlp& w, const MlpCall& c) {
  if (w.pre.empty()) return run_mlp_one(h, w, c);
  if (c.nadd || c.tri || !h->d_mlp_tmp[0]) return fail(h, GC_ERR_INTERNAL, "hidden_layers >= 2: unsupported MLP form");
  const int L = h->cfg.latent_size;
  auto handed = [&](MlpCall m, size_t buf) {      // the hand-over array in, float32
    m.nseg = 0; m.seg0_f32 = true;
    return m.segments({seg(h->d_mlp_tmp[buf & 1], nullptr, nullptr, L, L, 0)});
  };
  MlpCall lead = c;                              // no LayerNorm, float32 out
  lead.ln = lead.cond = lead.round_out = false; lead.residual = nullptr; lead.ldo = L; lead.out_f32 = true;
  for (size_t i = 0; i < w.pre.size(); ++i) {
    lead.out = h->d_mlp_tmp[i & 1];
    if (int rc = run_mlp_one(h, w.pre[i], i ? handed(lead, i - 1) : lead)) return rc;
  }
  return run_mlp_one(h, w, handed(c, w.pre.size() - 1));
}

// Row-tile height of the weight-streaming GEMM (x 32 rows).  Every workgroup streams its 128 weight columns
// once per row tile, so the L2 -> CU weight traffic per FLOP halves with every doubling: 64-row tiles once
// they still give >= 1.5 workgroups per CU.  128-row tiles were measured at the 1-degree sizes and did not
// help (FFW-1 1.49 vs 1.42 ms per call): these GEMMs are not bound by weight traffic.
int pick_ws_mt(int rows, int n, int splits) {
  const int panels = (n / 128) * splits;
  return ((rows + 63) / 64) * panels >= 400 ? 2 : 1;
}

// Work-item list for an attention launch whose tiles (one workgroup each, one workgroup per CU at heads of 128) would
// run as a full round of 256 plus a partly filled second one that lasts nearly as long (321 tiles at the 1-degree size:
// list scheduling of its 12-14 chunks per tile gives 29.6 chunk-times against a balanced 18.1, tools/attention_tile_schedule.py).
// Every XCD takes a contiguous range of tiles (the L2 locality of the plain launch); 32 of them run whole, one per CU, the
// other n - 32 (evenly spaced inside the range) are cut into 32 key-range pieces of at most kItemPieces per tile that follow
// as a second, short round; the pieces' partial results are merged by the out-projection's loader (GemmArgs::att_tiles).
// items: [8 * per_xcd][4] = (tile, first chunk, end chunk, partial slot or -1), tile -1 = padding; tiles: [n_tiles][2] = (first
// slot, pieces).  Used where the tiles per XCD are ONE full round plus at most 16 (1 degree: 32 + 8 / 9).
bool build_attention_items(const gc::HostGraph& g, std::vector<int>* items, std::vector<int>* tiles) {
  const int n = g.n_tiles;
  tiles->assign((size_t)2 * n, 0);
  // per XCD: full rounds of whole tiles (32 CUs, one workgroup each), then the n_cut < 32 tiles left over as pieces.
  // Worth it while the pieces are shorter than the tiles they replace: at most 16 cut tiles (>= 2 pieces each).
  std::vector<std::vector<int>> lists(8);
  int slot = 0, any_cut = 0;
  for (int x = 0; x < 8; ++x) {
    const int t0 = (int)((long long)n * x / 8), t1 = (int)((long long)n * (x + 1) / 8), ng = t1 - t0;
    if (ng < 32) return false;                               // less than one round: the plain launch (with key splits) is the right one
    if (ng >= 64) return false;   // several rounds balance themselves: at 0.25 degree (5 rounds + 1 tile) the list measured 4.48 -> 4.40 ms of
                                  // attention per call and 2.57 -> 2.66 of out-projection, net nothing
    const int n_cut = ng % 32;
    if (n_cut > 16) return false;
    any_cut += n_cut;
    std::vector<char> cut(ng, 0);
    for (int k = 0; k < n_cut; ++k) cut[(int)(((2LL * k + 1) * ng) / (2LL * n_cut))] = 1;   // evenly spaced: distinct, ng / n_cut >= 2
    std::vector<int>& it = lists[x];
    std::vector<int> order;
    for (int i = 0; i < ng; ++i) {
      const int t = t0 + i;
      if (cut[i]) { order.push_back(t); continue; }
      it.insert(it.end(), {t, g.tile_chunk_start[t], g.tile_chunk_start[t + 1], -1});
    }
    if ((int)order.size() != n_cut) return false;
    if (n_cut == 0) continue;
    // up to 32 pieces (one short round) over the cut tiles, at most kItemPieces each; the longest tiles get the extra ones
    const int pieces = std::min(32, gc::kItemPieces * n_cut), base = pieces / n_cut, rem = pieces % n_cut;
    std::vector<int> by_len = order;
    std::stable_sort(by_len.begin(), by_len.end(), [&](int a, int b) {
      return g.tile_chunk_start[a + 1] - g.tile_chunk_start[a] > g.tile_chunk_start[b + 1] - g.tile_chunk_start[b];
    });
    std::vector<std::array<int, 4>> pieces_x;
    for (int t : order) {
      int np = base;
      for (int k = 0; k < rem; ++k)
        if (by_len[k] == t) ++np;
      const int c0 = g.tile_chunk_start[t], nc = g.tile_chunk_start[t + 1] - c0;
      np = std::min(np, std::max(nc, 1));                    // never more pieces than chunks
      if (np > gc::kItemPieces || np < 1) return false;
      (*tiles)[2 * t] = slot;
      (*tiles)[2 * t + 1] = np;
      for (int k = 0; k < np; ++k) pieces_x.push_back({t, c0 + (nc * k) / np, c0 + (nc * (k + 1)) / np, slot++});
    }
    // the second round is dealt to CUs as they finish their whole tile: longest piece first (list scheduling), so that the
    // last CUs to come free take the shortest pieces
    std::stable_sort(pieces_x.begin(), pieces_x.end(), [](const std::array<int, 4>& a, const std::array<int, 4>& b) {
      return a[2] - a[1] > b[2] - b[1];
    });
    for (const auto& pc : pieces_x) it.insert(it.end(), pc.begin(), pc.end());
  }
  if (any_cut == 0 || slot > n) return false;                // nothing to balance / the partial buffers hold n_tiles slots
  size_t per_xcd = 0;
  for (const auto& l : lists) per_xcd = std::max(per_xcd, l.size() / 4);
  items->assign(8 * per_xcd * 4, -1);                        // tile -1: padding
  for (int x = 0; x < 8; ++x) std::copy(lists[x].begin(), lists[x].end(), items->begin() + (size_t)x * per_xcd * 4);
  return true;
}

// per-node half of a split edge MLP's first layer: out[rows][L] = nodes[rows][L] @ W_block
static int node_gemm(gc_handle* h, const float* nodes, int rows, const Weight& w, float* out) {
  const Route& r = h->route;
  const int L = h->cfg.latent_size;
  gc::GemmArgs ga{};
  ga.a = nodes; ga.lda = L; ga.a_f32 = 1; ga.ldw = L;
  ga.rows = rows; ga.n = L; ga.k_slice = L; ga.bias = nullptr; ga.act = 0; ga.out = out; ga.ldo = L;
  ga.round16 = 0;   // pre-activation terms of the split edge MLP: accumulator values, never rounded
  ga.out_f32 = 1;   // ... and float32 also when the node latents they are made from are stored as halfs
  if (r.node_ws) {  // (nodes are halfs in the gc_a16 build)
    ga.wt = pick(w, r, Form::Streaming); ga.a16 = r.st16 ? 1 : 0;
    return enqueue_gemm_ws(h, gc::KC_GEMM_NODE, ga, pick_ws_mt(rows, L, 1), 1, 0);
  }
  ga.wt = pick(w, r, Form::Staged);
  return launch(h, gc::KC_GEMM_NODE, [&] { return gc::launch_gemm(h->stream, gc::KC_GEMM_NODE, ga, 1, 0, r.f16); });
}
// both of them, in front of the edge MLP that gathers them as add terms
static int edge_node_products(gc_handle* h, const DevMlp& w, const float* senders, int snd_rows, float* snd_out,
                              const float* receivers, int rcv_rows, float* rcv_out) {
  if (int rc = node_gemm(h, senders, snd_rows, w.w1snd, snd_out)) return rc;
  return node_gemm(h, receivers, rcv_rows, w.w1rcv, rcv_out);
}

// An edge update e' = MLPc([e | nodes[senders] | nodes[receivers]]) (typed_graph_net.py:134-159): the gathered node
// latents as segments, or -- split_edge -- their per-node first-layer products (pnd, prcv) as add terms.
static MlpCall edge_call(gc_handle* h, const float* e_hat, const float* e_affine, int E, const int* snd, const int* rcv,
                         const float* nsnd, const float* nrcv, const float* psnd, const float* prcv, float* out) {
  const int B = h->cfg.batch, L = h->cfg.latent_size;
  MlpCall c = mlp_call({seg(e_hat, nullptr, e_affine, L, L, 1)}, E * B, B, out, L);
  c.seg0_f32 = true;
  if (h->route.split_edge) c.add_terms({{psnd, snd}, {prcv, rcv}});
  else c.segments({seg(nsnd, snd, nullptr, L, L, 0), seg(nrcv, rcv, nullptr, L, L, 0)});
  return c;
}
// The same update on the edge-term route: no segment, no product -- the first layer is the noise level's edge term (one
// row per edge), the senders' product and the receivers' product, added in that order, then b1 (MlpArgs::nseg == 0).
static MlpCall edge_terms_call(gc_handle* h, const float* T, int E, const int* snd, const int* rcv, const float* psnd,
                               const float* prcv, float* out) {
  const int B = h->cfg.batch, L = h->cfg.latent_size;
  MlpCall c = mlp_call({}, E * B, B, out, L);
  c.seg0_f32 = true;
  return c.add_terms({{T, nullptr}, {psnd, snd}, {prcv, rcv}});
}

// mesh2grid edge update f1 = MLPc([f0 | m2[senders] | g1[receivers]]) (typed_graph_net.py:295-305; split_edge: the
// per-node products are in d_pm / d_pg by then).  fused: the kernel's epilogue adds each grid node's three results and
// writes agg2 [G, L] instead of f1 [E2, L].  Runs on h->route (gc_debug_fetch re-runs it unfused).
int run_m2g_edge(gc_handle* h, const float* cond, bool fused) {
  const size_t slot_rows = (size_t)std::max(h->term_slot, 0) * h->hg.E2 * h->cfg.latent_size;
  MlpCall c = h->route.edge_terms
                  ? edge_terms_call(h, h->terms.T2 + slot_rows, h->hg.E2, h->d_m2g_snd, h->d_m2g_rcv, h->d_pm, h->d_pg,
                                    fused ? h->d_agg2 : h->d_f1)
                  : edge_call(h, h->d_f0_hat, cond + h->m2g_embed_edge.cond_off, h->hg.E2, h->d_m2g_snd, h->d_m2g_rcv,
                        h->d_m2, h->d_g1, h->d_pm, h->d_pg, fused ? h->d_agg2 : h->d_f1);
  c.tri = fused;
  return run_mlp(h, h->m2g_edge, c);
}

// The fields every transformer GEMM over the mesh rows shares (ws: it takes the weight-streaming form).
static gc::GemmArgs mesh_gemm_args(const gc_handle* h, const float* a, int lda, bool ws) {
  gc::GemmArgs ga{};
  ga.a = a; ga.lda = lda; ga.a_f32 = 1; ga.rows = h->hg.M * h->cfg.batch;
  ga.round16 = h->feat16 ? 1 : 0; ga.a16 = h->route.st16 ? 1 : 0; ga.f32w = (ws && h->route.x32) ? 1 : 0;
  return ga;
}
// A = the attention output merged in the loader: from the key-split partials, or (item list) for the rows of the tiles
// that were cut into pieces.
static void merge_attention_partials(const gc_handle* h, gc::GemmArgs* ga) {
  const int D = h->cfg.d_model, H = h->cfg.num_heads;
  ga->att_po = h->d_apart_o; ga->att_pml = h->d_apart_ml; ga->att_B = h->cfg.batch; ga->att_H = H; ga->att_DH = D / H;
  if (h->attn_splits > 1) ga->att_S = h->attn_splits;
  else ga->att_tiles = h->d_att_tiles;
}
// out = act(a @ W + bias) (epi 0) or raw split-K slabs (epi 1) over the mesh rows: the weight-streaming GEMM where the
// route allows it, else the LDS-staged one.  att_merge: a is the attention output, still in key-split partials.
static int mesh_gemm(gc_handle* h, int cls, const float* a, int lda, const Weight& w, int n, int k, int splits,
                     const float* bias, int act, float* out, int ldo, int epi, bool att_merge = false) {
  const Route& r = h->route;
  const bool ws = r.ws(n, k, splits);
  gc::GemmArgs ga = mesh_gemm_args(h, a, lda, ws);
  ga.wt = pick(w, r, ws ? Form::Streaming : Form::Staged); ga.ldw = k; ga.n = n; ga.k_slice = k / splits;
  ga.bias = bias; ga.act = act; ga.out = out; ga.ldo = ldo;
  if (att_merge) merge_attention_partials(h, &ga);
  // 64-row tiles halve the weight traffic (pick_ws_mt); merged partials come in 32-row tiles only
  if (ws) return enqueue_gemm_ws(h, cls, ga, att_merge ? 1 : pick_ws_mt(ga.rows, n, splits), splits, epi);
  return launch(h, cls, [&] { return gc::launch_gemm(h->stream, cls, ga, splits, epi, r.f16); });
}

// One denoiser forward on device-resident, already packed grid input (h->d_xp).
// sigma comes from h->d_sigma when sigma_scalar < 0, else the scalar is used for every batch element.
int forward(gc_handle* h, float sigma_scalar, const float* cond_ready) {
  const gc_config& c = h->cfg;
  const gc::HostGraph& g = h->hg;
  const int B = c.batch, L = c.latent_size, D = c.d_model, F = c.ffw_hidden;
  hipStream_t s = h->stream;
  int rc;
  // cond_ready: the sampler computed this call's conditioning vectors up front (one launch per sample)
  const float* cond = cond_ready ? cond_ready : h->d_cond;
  h->cond_cur = cond;
  const int cs = h->cond_total;
  const int64_t launches0 = h->launch_count;
  const Route& r = h->route = h->last_route = make_route(h);

  if (!cond_ready && (rc = launch(h, gc::KC_COND, [&] {
         return gc::launch_cond(s, sigma_scalar < 0 ? h->d_sigma : nullptr, sigma_scalar, B, h->d_nw0t,
                                h->d_nb0, h->d_nw1t, h->d_nb1, c.noise_num_frequencies, c.noise_hidden,
                                c.noise_base_period, h->d_wc_all, h->d_bc_all, cs, h->d_condvec,
                                h->d_cond);
       })))
    return rc;

  // ---- grid2mesh (denoiser.py:602-688; deep_typed_graph_net.py:493-581) ----
  {
    // inside a sample: the noisy block of the first layer + the cached static part (embed_cache); else all columns
    MlpCall embed = r.embed_cache ? mlp_call({seg(h->d_xn, nullptr, nullptr, h->nwp, h->nwp, 0)}, g.G * B, B, h->d_g0, L)
                                  : mlp_call({seg(h->d_xp, nullptr, nullptr, h->kp, h->kp, 0)}, g.G * B, B, h->d_g0, L);
    embed.seg0_f32 = true;
    if (r.embed_cache) embed.add_terms({{h->d_pstat, nullptr}});
    if ((rc = run_mlp(h, r.embed_cache ? h->g2m_embed_grid_n : h->g2m_embed_grid, embed))) return rc;
  }
  // m0 = affine(m0_hat; cond): a launch of the call, or (edge terms) the noise level's slot of the cache
  const size_t ML = (size_t)g.M * L;
  if (r.edge_terms && (h->term_slot < 0 || !h->terms.ready))
    return fail(h, GC_ERR_INTERNAL, "edge terms: the forward has no slot of the cache");
  const float* const m0 = r.edge_terms ? h->terms.m0 + h->term_slot * ML : h->d_m0;
  h->m0_cur = m0;
  if (!r.edge_terms && (rc = launch(h, gc::KC_PACK, [&] {
         return gc::launch_affine_rows(s, h->d_m0_hat, cond + h->g2m_embed_mesh.cond_off, cs, g.M, B, L,
                                       h->d_m0, h->feat16, r.st16);
       })))
    return rc;
  // The grid2mesh edge update and the grid-node update g1 = g0 + MLP(g0) read only g0 / m0 and are independent
  // (typed_graph_net.py:134-195): when both take the same kernel form they go out as ONE launch (gc_mlp_ws_pair_kernel) --
  // at nano the edge update's 526 row tiles are a round of 512 workgroups and a round of 14 that lasts as long again, and
  // the node update's 329 tiles fill that second round instead of a launch of their own (GC_TUNE_MLP_PAIR=0: two launches).
  // edge terms: the senders' product g0 @ W1snd is the one per-call product of this update (the receivers' is Pm[slot])
  if (r.edge_terms && (rc = node_gemm(h, h->d_g0, g.G * B, h->g2m_edge.w1snd, h->d_pg))) return rc;
  const MlpCall edge = r.edge_terms
                           ? edge_terms_call(h, h->terms.T1 + (size_t)h->term_slot * g.E1 * L, g.E1, h->d_g2m_snd, h->d_g2m_rcv,
                                             h->d_pg, h->terms.Pm + h->term_slot * ML, h->d_e1)
                           : edge_call(h, h->d_e0_hat, cond + h->g2m_embed_edge.cond_off, g.E1, h->d_g2m_snd, h->d_g2m_rcv,
                                       h->d_g0, h->d_m0, h->d_pg, h->d_pm, h->d_e1);
  const MlpCall node = mlp_call({seg(h->d_g0, nullptr, nullptr, L, L, 0)}, g.G * B, B, h->d_g1, L, h->d_g0);
  gc::MlpArgs ea{}, na{};
  bool paired = false;
  if (r.try_pair) {
    if ((rc = build_mlp_args(h, h->g2m_edge, edge, &ea)) || (rc = build_mlp_args(h, h->g2m_grid, node, &na))) return rc;
    paired = gc::mlp_pair_supported(ea, na);
  }
  if (r.split_edge && (rc = edge_node_products(h, h->g2m_edge, h->d_g0, g.G * B, h->d_pg, h->d_m0, g.M * B, h->d_pm)))
    return rc;
  if ((rc = paired ? enqueue_mlp_pair(h, ea, na) : run_mlp(h, h->g2m_edge, edge))) return rc;
  if ((rc = launch(h, gc::KC_SEGSUM, [&] {
         return gc::launch_segsum(s, h->d_e1, h->d_g2m_ptr, h->d_g2m_eid, g.M, g.E1, B, L, h->d_agg1, h->feat16, r.st16,
                                  h->g2m_agg_norm);
       })))
    return rc;
  if ((rc = run_mlp(h, h->g2m_mesh, mlp_call({seg(m0, nullptr, nullptr, L, L, 0), seg(h->d_agg1, nullptr, nullptr, L, L, 0)},
                                             g.M * B, B, h->d_x, L, m0))))
    return rc;
  if (!paired && (rc = run_mlp(h, h->g2m_grid, node))) return rc;

  // ---- mesh transformer (sparse_transformer.py:486-525, 624-634) ----
  // The residual adds are deferred: a projection writes split-K slabs, and the next row pass
  // (gc_rowop) folds "x += bias + slabs" together with the following LayerNorm + conditioning.
  // The exact-f32 family (precision = f32, and the re-run of the f16x3 domain guard) takes the SAME launch structure:
  // the weight-streaming GEMM, the fused FFW and the out-projection + row pass read WF32 images (Route::x32).
  const int MB = g.M * B;
  const int n_layers = (h->debug_layer_limit >= 0 && h->debug_layer_limit < c.num_layers)
                           ? h->debug_layer_limit : c.num_layers;
  const float* pend_bias = nullptr;
  int pend_slabs = 0;
  auto rowop = [&](const float* bias, int slabs, int cond_off, float* hout) {
    return launch(h, gc::KC_ROWOP, [&] {
      return gc::launch_rowop(s, h->d_x, bias, h->d_part, slabs, MB, D, B, cond + cond_off, cs, hout, 0, h->feat16, r.st16);
    });
  };
  // gc_debug_set_stop (tests): leave the forward inside block i, after phase 0 (pre-attention row pass: x, h),
  // 1 (QKV projection) or 2 (attention + out-projection + row pass: x, h); buffers keep what was computed so far
  auto stop_here = [&](int i, int phase) { return h->debug_stop_layer == i && h->debug_stop_phase == phase; };
  const int* att_items = r.att_items ? h->d_att_items : nullptr;
  for (int i = 0; i < n_layers; ++i) {
    const DevLayer& ly = h->layers[i];
    if ((rc = rowop(pend_bias, pend_slabs, ly.cond_attn, h->d_h))) return rc;
    if (stop_here(i, 0)) return GC_OK;
    if (r.v2) {
      gc::GemmArgs ga = mesh_gemm_args(h, h->d_h, D, true);
      ga.wt = pick(ly.wqkv, r, Form::Streaming); ga.ldw = D; ga.n = 3 * D; ga.k_slice = D;
      ga.out = h->d_qkv; ga.ldo = r.st16 ? D : 3 * D;   // fp16 storage: q alone, as halfs [rows][D]
      ga.kv16 = h->d_kv16; ga.kv_d = D;
      if ((rc = enqueue_gemm_ws(h, gc::KC_GEMM_QKV, ga, pick_ws_mt(MB, 3 * D, 1), 1, 3))) return rc;
      if (stop_here(i, 1)) return GC_OK;
      if ((rc = launch(h, gc::KC_ATTN, [&] {
             return gc::launch_attention_v2(s, h->d_qkv, h->d_kv16, h->d_att, h->d_apart_o, h->d_apart_ml, g.M, B, D,
                                            c.num_heads, h->attn_splits, h->d_tile_start, h->d_union, h->d_mask,
                                            g.n_tiles, h->max_tile_chunks, h->feat16, r.st16, att_items, r.att_items);
           })))
        return rc;
    } else {
      if ((rc = mesh_gemm(h, gc::KC_GEMM_QKV, h->d_h, D, ly.wqkv, 3 * D, D, 1, nullptr, 0, h->d_qkv, 3 * D, 0))) return rc;
      if (stop_here(i, 1)) return GC_OK;
      if ((rc = launch(h, gc::KC_ATTN, [&] {
             return gc::launch_attention(s, h->d_qkv, h->d_att, h->d_apart_o, h->d_apart_ml, g.M, B, D,
                                         c.num_heads, h->attn_splits, false, h->d_tile_start, h->d_union,
                                         h->d_mask, g.n_tiles, h->feat16, att_items, r.att_items);
           })))
        return rc;
    }
    // key-split partials (attn_splits > 1) and the pieces of an item list are merged inside the out-projection's A
    // loader (no combine launch).  Out-projection with the row pass in its epilogue: weight-streaming form, no K split
    if (r.fuse_row) {
      gc::GemmArgs ga = mesh_gemm_args(h, h->d_att, D, true);
      ga.wt = pick(ly.wo, r, Form::Streaming); ga.ldw = D; ga.n = D; ga.k_slice = D;
      if (h->attn_splits > 1 || r.att_items) merge_attention_partials(h, &ga);
      gc::RowFuse rf{h->d_x, ly.bo, cond + ly.cond_ffw, cs, B, h->d_h, h->feat16 ? 1 : 0};
      if ((rc = enqueue_gemm_rowop(h, gc::KC_GEMM_OUT, ga, rf))) return rc;
    } else {
      if ((rc = mesh_gemm(h, gc::KC_GEMM_OUT, h->d_att, D, ly.wo, D, D, h->out_splits, nullptr, 0, h->d_part, D, 1, h->attn_splits > 1)))
        return rc;
      if ((rc = rowop(ly.bo, h->out_splits, ly.cond_ffw, h->d_h))) return rc;
    }
    if (stop_here(i, 2)) return GC_OK;
    if (r.ffw_slabs > 0) {   // both FFW layers in one launch, one slab per 256 hidden columns
      gc::FfwArgs fa{h->d_h, MB, (int)D, (int)F, pick(ly.w1, r, Form::Streaming), ly.b1, pick(ly.w2, r, Form::Streaming),
                     h->d_part, h->feat16 ? 1 : 0, r.st16 ? 1 : 0};
      fa.f32w = r.x32 ? 1 : 0;
      if ((rc = enqueue_ffw_fused(h, fa))) return rc;
    } else {
      if ((rc = mesh_gemm(h, gc::KC_GEMM_FFW1, h->d_h, D, ly.w1, F, D, 1, ly.b1, 1, h->d_u, F, 0))) return rc;
      if ((rc = mesh_gemm(h, gc::KC_GEMM_FFW2, h->d_u, F, ly.w2, D, F, h->ffw2_splits, nullptr, 0, h->d_part, D, 1))) return rc;
    }
    pend_bias = ly.b2;
    pend_slabs = r.ffw_slabs > 0 ? r.ffw_slabs : h->ffw2_splits;
  }
  if ((rc = rowop(pend_bias, pend_slabs, h->cond_final, h->d_m2))) return rc;

  // ---- mesh2grid + decoder (denoiser.py:730-768) ----
  if ((r.split_edge || r.edge_terms) && (rc = edge_node_products(h, h->m2g_edge, h->d_m2, g.M * B, h->d_pm, h->d_g1, g.G * B, h->d_pg)))
    return rc;
  // The edge update, and the sum of every grid node's 3 updated edges (typed_graph_net.py:175-182): ONE launch when the
  // route says so (Route::m2g_fused) -- f1 [E2, L] is neither stored nor read back.  Other in-degrees (injected graphs),
  // hidden_layers >= 2, the LDS-staged MLP kernel: edge update, then the segment-sum launch.
  if ((rc = run_m2g_edge(h, cond, r.m2g_fused))) return rc;
  if (!r.m2g_fused && (rc = launch(h, gc::KC_SEGSUM, [&] {
         return gc::launch_segsum(s, h->d_f1, h->d_m2g_ptr, h->d_m2g_eid, g.G, g.E2, B, L, h->d_agg2, h->feat16, r.st16);
       })))
    return rc;
  if ((rc = run_mlp(h, h->m2g_grid, mlp_call({seg(h->d_g1, nullptr, nullptr, L, L, 0), seg(h->d_agg2, nullptr, nullptr, L, L, 0)},
                                             g.G * B, B, h->d_g2, L, h->d_g1))))
    return rc;
  MlpCall dec = mlp_call({seg(h->d_g2, nullptr, nullptr, L, L, 0)}, g.G * B, B, h->d_y, c.c_out);
  dec.ln = dec.cond = false; dec.out_f32 = true;
  if ((rc = run_mlp(h, h->m2g_dec, dec))) return rc;
  h->launches_last_call = h->launch_count - launches0;
  return GC_OK;
}

// Static embeddings: LayerNorm(MLP(static features)) in the precision currently selected; the
// per-call conditioning is applied where they are consumed.  Re-run when the precision changes.
// f16x3 domain guard: every call reads them, the exact-f32 re-run of a poisoned call included, so a hidden activation
// beyond fp16 range in here (every weight inside it: weights_f16_unsafe does not see that) would leave NaN in them for
// the life of the handle, and the re-run of every call would return NaN too.  They are checked where they are made and
// made again on the exact-f32 kernels when poisoned; nothing is added to a call.
int compute_static_embeddings(gc_handle* h) {
  const gc::HostGraph& hg = h->hg;
  const int L = h->cfg.latent_size;
  const struct { const DevMlp& w; const float* in; int items; float* out; } embeds[] = {
      {h->g2m_embed_mesh, h->d_mesh_struct16, hg.M, h->d_m0_hat},
      {h->g2m_embed_edge, h->d_e1_struct16, hg.E1, h->d_e0_hat},
      {h->m2g_embed_edge, h->d_e2_struct16, hg.E2, h->d_f0_hat}};
  if (int rc = drop_edge_terms(h)) return rc;   // the edge terms are made from these embeddings
  auto run = [&]() -> int {
    h->route = make_route(h);    // same kernel build as the forward will use; float32 in (structural features) and out
    for (const auto& e : embeds) {
      MlpCall c = mlp_call({seg(e.in, nullptr, nullptr, 32, 32, 1)}, e.items, 1, e.out, L);
      c.cond = c.round_out = false; c.seg0_f32 = c.out_f32 = true;
      if (int rc = run_mlp(h, e.w, c)) return rc;
    }
    return GC_OK;
  };
  if (int rc = run()) return rc;
  GC_HIP(h, hipStreamSynchronize(h->stream));
  // (fp16 features: an overflow in there is the mode's own arithmetic, the exact-f32 kernels round to the same Inf)
  if (!h->route.f16 || h->feat16) return GC_OK;
  // The counter is shared with the calls' checks.  Both gc_set_option callers resolve a pending sample's check first and
  // gc_finalize has no sample to keep; should one be unresolved all the same, its count reached the host copy with the
  // synchronisation above (guard_enqueue queued that copy behind the sample), so `before` holds it and only what these
  // three launches add is taken off as theirs.
  const unsigned before = *h->h_nonfinite;
  for (const auto& e : embeds)
    if (int rc = launch(h, gc::KC_PACK, [&] { return gc::launch_finite_check(h->stream, e.out, (size_t)e.items * L, h->d_nonfinite); }))
      return rc;
  GC_HIP(h, hipMemcpyAsync(h->h_nonfinite, h->d_nonfinite, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  const unsigned hits = *h->h_nonfinite - before;
  if (!hits) return GC_OK;
  h->nonfinite_seen += hits;
  ++h->static_embedding_fallbacks;
  h->in_fallback = true;
  const int rc = run();
  h->in_fallback = false;
  if (rc) return rc;
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
}

// ---- edge terms (gc_handle::EdgeTerms) ----
// Forgets the cache: waits for the stream that may still read it, frees it, and drops the captured samples, which bake
// its addresses.  Called wherever something the terms are made from changes (weights, precision, feature mode, the static
// embeddings, the cap) and by ensure_edge_terms for a new noise-level list.
int drop_edge_terms(gc_handle* h) {
  if (h->terms.sigmas.empty() && h->term_allocs.ptrs.empty()) return GC_OK;
  if (!h->term_allocs.ptrs.empty()) {
    GC_HIP(h, hipStreamSynchronize(h->stream));
    drop_sample_graphs(h);
    h->term_allocs.free();
  }
  h->terms = gc_handle::EdgeTerms{};
  h->term_slot = -1;
  return GC_OK;
}

// Makes the cache hold the terms of this sample's noise levels (one per denoiser call, in call order), outside any
// stream capture: a no-op when it already does -- every sample after the first of a sampler configuration.  Otherwise the
// cache of the previous list goes and, if the new one fits the cap, is built on the handle's stream with the kernels
// every call used so far: the conditioning of all levels in one launch, then per distinct level the affine pass over
// each static embedding and the weight-streaming GEMM with the block of W1 it meets.  Over the cap (or more levels than
// one conditioning launch takes) nothing is built and the sample keeps the route with the products.
int ensure_edge_terms(gc_handle* h, const std::vector<float>& call_sigma) {
  if (!edge_terms_possible(h)) return GC_OK;    // (the cache, if any, stays: the exact-f32 re-run of a sample must not cost the next one its terms)
  gc_handle::EdgeTerms& t = h->terms;
  if (t.sigmas.size() == call_sigma.size() &&
      !std::memcmp(t.sigmas.data(), call_sigma.data(), call_sigma.size() * sizeof(float)))
    return GC_OK;                               // built, or found too large, for this very list
  if (int rc = drop_edge_terms(h)) return rc;
  t.sigmas = call_sigma;
  std::vector<float> distinct;
  for (float sg : call_sigma) {
    size_t k = 0;
    while (k < distinct.size() && std::memcmp(&distinct[k], &sg, sizeof(float))) ++k;
    if (k == distinct.size()) distinct.push_back(sg);
    t.call_slot.push_back((int)k);
  }
  const gc::HostGraph& g = h->hg;
  const gc_config& c = h->cfg;
  const size_t L = c.latent_size, n = distinct.size();
  const size_t per_slot = ((size_t)g.E1 + g.E2 + 2 * (size_t)g.M) * L;
  t.bytes = (int64_t)(n * per_slot * sizeof(float));
  if (n == 0 || n > (size_t)gc::kMaxSigmaList || t.bytes > h->edge_term_cap_mb * (int64_t)(1 << 20) ||
      n * (size_t)c.batch * h->cond_total > h->cond_all_cap) {
    t.bytes = 0;
    return GC_OK;
  }
  int rc;
  BufferGroup* own = &h->term_allocs;
  if ((rc = dev_alloc(h, &t.T1, n * g.E1 * L, own)) || (rc = dev_alloc(h, &t.T2, n * g.E2 * L, own)) ||
      (rc = dev_alloc(h, &t.m0, n * g.M * L, own)) || (rc = dev_alloc(h, &t.Pm, n * g.M * L, own)))
    return rc;
  hipStream_t s = h->stream;
  h->route = make_route(h);                     // f16x3 on float32 arrays (edge_terms_possible): the node GEMM's form
  gc::SigmaList sl{};
  for (size_t i = 0; i < n; ++i) sl.v[i] = distinct[i];
  if ((rc = launch(h, gc::KC_COND, [&] {
         return gc::launch_cond_multi(s, sl, (int)n, c.batch, h->d_nw0t, h->d_nb0, h->d_nw1t, h->d_nb1, c.noise_num_frequencies,
                                      c.noise_hidden, c.noise_base_period, h->d_wc_all, h->d_bc_all, h->cond_total, h->d_cond_all);
       })))
    return rc;
  // d_e1 / d_f1 ([E1][L], [E2][L] at batch 1) hold the conditioned edge embeddings of the level in hand: every call
  // overwrites them anyway
  const int cs = h->cond_total;
  for (size_t i = 0; i < n; ++i) {
    const float* cond = h->d_cond_all + i * (size_t)c.batch * cs;
    const struct { const float* hat; int cond_off, items; float* staged; const Weight* w; float* out; } passes[] = {
        {h->d_e0_hat, h->g2m_embed_edge.cond_off, g.E1, h->d_e1, &h->g2m_edge.w1e, t.T1 + i * g.E1 * L},
        {h->d_f0_hat, h->m2g_embed_edge.cond_off, g.E2, h->d_f1, &h->m2g_edge.w1e, t.T2 + i * g.E2 * L},
        {h->d_m0_hat, h->g2m_embed_mesh.cond_off, g.M, t.m0 + i * g.M * L, &h->g2m_edge.w1rcv, t.Pm + i * g.M * L}};
    for (const auto& p : passes) {
      if ((rc = launch(h, gc::KC_PACK, [&] {
             return gc::launch_affine_rows(s, p.hat, cond + p.cond_off, cs, p.items, 1, (int)L, p.staged, false, false);
           })))
        return rc;
      if ((rc = node_gemm(h, p.staged, p.items, *p.w, p.out))) return rc;
    }
  }
  t.ready = true;
  return GC_OK;
}

}  // namespace gci
