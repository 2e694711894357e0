// Weights of libgencast_hip.so: the parameter specs, the host-side encoders of the device images (S16, WF16, WF32),
// and gc_finalize's layout of every matrix on the device.
#include "gc_handle.h"

namespace gci {

const char* const P_NOISE = "denoiser.noise_level_encoder";
const char* const P_G2M = "denoiser.predictor.grid2mesh_gnn";
const char* const P_M2G = "denoiser.predictor.mesh2grid_gnn";
const char* const P_TR = "denoiser.predictor.mesh_gnn.batch_first_transformer";

void add_mlp_specs(gc_handle* h, const std::string& p, int n_in, int n_hid, int n_out, bool cond) {
  // common/mlp.py:166-199: hidden_layers x (Linear, activation), then the output Linear; nnx.Sequential index 2 i = i-th Linear
  const int nh = h->hidden_layers;
  for (int i = 0; i < nh; ++i) {
    const std::string l = p + ".network.network.layers." + std::to_string(2 * i);
    h->specs[l + ".kernel"] = {i == 0 ? n_in : n_hid, n_hid};
    h->specs[l + ".bias"] = {n_hid};
  }
  const std::string l = p + ".network.network.layers." + std::to_string(2 * nh);
  h->specs[l + ".kernel"] = {n_hid, n_out};
  h->specs[l + ".bias"] = {n_out};
  if (cond) {
    h->specs[p + ".norm_conditioning_layer.conditional_linear_layer.kernel"] = {gc::kCondDim, 2 * n_out};
    h->specs[p + ".norm_conditioning_layer.conditional_linear_layer.bias"] = {2 * n_out};
  }
}

void build_specs(gc_handle* h) {
  const gc_config& c = h->cfg;
  const int L = c.latent_size, D = c.d_model, F = c.ffw_hidden;
  const std::string n = P_NOISE, g = P_G2M, m = P_M2G, t = P_TR;
  h->specs[n + ".linear_0.kernel"] = {2 * c.noise_num_frequencies, c.noise_hidden};
  h->specs[n + ".linear_0.bias"] = {c.noise_hidden};
  h->specs[n + ".linear_1.kernel"] = {c.noise_hidden, gc::kCondDim};
  h->specs[n + ".linear_1.bias"] = {gc::kCondDim};
  const int node_in = 3 + c.c_in;
  add_mlp_specs(h, g + ".embedder_network.embed_edge_fns.grid2mesh", 4, L, L, true);
  add_mlp_specs(h, g + ".embedder_network.embed_node_fns.grid_nodes", node_in, L, L, true);
  add_mlp_specs(h, g + ".embedder_network.embed_node_fns.mesh_nodes", node_in, L, L, true);
  const std::string gn = g + ".processor_networks.0.graph_network";
  add_mlp_specs(h, gn + ".update_edge_fns.grid2mesh.edge_fn", 3 * L, L, L, true);
  add_mlp_specs(h, gn + ".update_node_fns.grid_nodes.node_fn", L, L, L, true);
  add_mlp_specs(h, gn + ".update_node_fns.mesh_nodes.node_fn", 2 * L, L, L, true);
  add_mlp_specs(h, m + ".embedder_network.embed_edge_fns.mesh2grid", 4, L, L, true);
  const std::string gn2 = m + ".processor_networks.0.graph_network";
  add_mlp_specs(h, gn2 + ".update_edge_fns.mesh2grid.edge_fn", 3 * L, L, L, true);
  add_mlp_specs(h, gn2 + ".update_node_fns.grid_nodes.node_fn", 2 * L, L, L, true);
  add_mlp_specs(h, m + ".decoder_network.embed_node_fns.grid_nodes", L, L, c.c_out, false);
  for (int i = 0; i < c.num_layers; ++i) {
    const std::string b = t + ".blocks." + std::to_string(i);
    for (const char* q : {"q", "k", "v"})
      h->specs[b + ".attn_module." + q + "_proj.linear.kernel"] = {D, D};
    h->specs[b + ".attn_module.final_linear.kernel"] = {D, D};
    h->specs[b + ".attn_module.final_linear.bias"] = {D};
    h->specs[b + ".ffw_module.mlp.layers.0.kernel"] = {D, F};
    h->specs[b + ".ffw_module.mlp.layers.0.bias"] = {F};
    h->specs[b + ".ffw_module.mlp.layers.2.kernel"] = {F, D};
    h->specs[b + ".ffw_module.mlp.layers.2.bias"] = {D};
    for (const char* nc : {"norm_cond_attn", "norm_cond_ffw"}) {
      h->specs[b + "." + nc + ".conditional_linear_layer.kernel"] = {gc::kCondDim, 2 * D};
      h->specs[b + "." + nc + ".conditional_linear_layer.bias"] = {2 * D};
    }
  }
  h->specs[t + ".final_norm_cond.conditional_linear_layer.kernel"] = {gc::kCondDim, 2 * D};
  h->specs[t + ".final_norm_cond.conditional_linear_layer.bias"] = {2 * D};
}

// kernel (in,out) -> transposed [out_pad][in_pad], using input rows [in_begin, in_begin+in_count)
std::vector<float> transpose_pad(const std::vector<float>& k, int n_in, int n_out, int in_begin,
                                 int in_count, int in_pad, int out_pad) {
  std::vector<float> t((size_t)out_pad * in_pad, 0.f);
  for (int i = 0; i < in_count; ++i)
    for (int o = 0; o < n_out; ++o) t[(size_t)o * in_pad + i] = k[(size_t)(in_begin + i) * n_out + o];
  (void)n_in;
  return t;
}

// IEEE half conversions on the host (round to nearest even), used to pre-split the weights.
uint16_t f32_to_f16_bits(float f) {
  uint32_t x;
  std::memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  const uint32_t mant = x & 0x7FFFFFu;
  const int exp = (int)((x >> 23) & 0xFF) - 127 + 15;
  if (((x >> 23) & 0xFF) == 0xFF) return (uint16_t)(sign | 0x7C00u | (mant ? 0x200u : 0));
  if (exp >= 31) return (uint16_t)(sign | 0x7BFFu);                 // clamp to the largest finite half
  if (exp <= 0) {
    if (exp < -10) return (uint16_t)sign;
    const uint32_t m = mant | 0x800000u;
    const int shift = 14 - exp;
    uint32_t h = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (h & 1))) ++h;
    return (uint16_t)(sign | h);
  }
  uint32_t h = ((uint32_t)exp << 10) | (mant >> 13);
  const uint32_t rem = mant & 0x1FFFu;
  if (rem > 0x1000u || (rem == 0x1000u && (h & 1))) ++h;
  return (uint16_t)(sign | h);
}

float f16_bits_to_f32(uint16_t h) {
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
  const int exp = (h >> 10) & 0x1F;
  const uint32_t mant = h & 0x3FFu;
  float out;
  if (exp == 0) {
    out = std::ldexp((float)mant, -24);
  } else if (exp == 31) {
    out = mant ? NAN : INFINITY;
  } else {
    out = std::ldexp((float)(mant | 0x400u), exp - 25);
  }
  uint32_t bits;
  std::memcpy(&bits, &out, 4);
  bits |= sign;
  std::memcpy(&out, &bits, 4);
  return out;
}

// Row-major f32 [rows][k] (k % 32 == 0) -> S16: per row, k/32 groups of [32 hi halfs | 32 lo halfs];
// same 4 bytes per element, returned as a float-typed buffer.
std::vector<float> encode_s16(const std::vector<float>& m, int rows, int k) {
  std::vector<float> out((size_t)rows * k);
  uint16_t* o = reinterpret_cast<uint16_t*>(out.data());
  for (int r = 0; r < rows; ++r)
    for (int g = 0; g < k / 32; ++g)
      for (int i = 0; i < 32; ++i) {
        float x = m[(size_t)r * k + g * 32 + i];
        x = std::min(std::max(x, -65000.0f), 65000.0f);
        const uint16_t hi = f32_to_f16_bits(x);
        const uint16_t lo = f32_to_f16_bits((x - f16_bits_to_f32(hi)) * 2048.0f);
        o[((size_t)r * k + g * 32) * 2 + i] = hi;
        o[((size_t)r * k + g * 32) * 2 + 32 + i] = lo;
      }
  return out;
}

// Row-major f32 W^T [n][k] (n % 32 == 0, k % 16 == 0) -> WF16, the MFMA fragment order the
// weight-streaming GEMM loads with one coalesced 16-byte read per lane: for column tile ct = n/32
// and k step s = k/16, 1 KB of hi halfs then 1 KB of lo halfs; inside each, lane (k%16/8)*32 + n%32
// holds the 8 consecutive k values it feeds to v_mfma_f32_32x32x16_f16.
std::vector<float> encode_wf16(const std::vector<float>& m, int n, int k) {
  std::vector<float> out((size_t)n * k);
  uint16_t* o = reinterpret_cast<uint16_t*>(out.data());
  const size_t steps = (size_t)k / 16;
  for (int row = 0; row < n; ++row)
    for (int kk = 0; kk < k; ++kk) {
      float x = m[(size_t)row * k + kk];
      x = std::min(std::max(x, -65000.0f), 65000.0f);
      const uint16_t hi = f32_to_f16_bits(x);
      const uint16_t lo = f32_to_f16_bits((x - f16_bits_to_f32(hi)) * 2048.0f);
      const size_t frag = ((size_t)(row / 32) * steps + kk / 16) * 2;
      const int k16 = kk % 16;
      const size_t lane = (size_t)(k16 >> 3) * 32 + row % 32;
      o[(frag * 64 + lane) * 8 + (k16 & 7)] = hi;
      o[((frag + 1) * 64 + lane) * 8 + (k16 & 7)] = lo;
    }
  return out;
}

// Row-major f32 W^T [n][k] -> WF32, the same blocks as WF16 with float32 payload: for column tile n/32 and k step k/16,
// 512 floats; lane (k%16/8)*32 + n%32 holds ITS 8 consecutive k values as 4 floats at [lane*4] (k%8 < 4) and 4 floats at
// [256 + lane*4] -- so the weight-streaming kernels' two 16-byte loads per fragment (the "hi" and "lo" slots of the
// ring) fetch the two halves, and a k16 step is 8 v_mfma_f32_32x32x2_f32 (exact-f32 family, precision = f32).
std::vector<float> encode_wf32(const std::vector<float>& m, int n, int k) {
  std::vector<float> out((size_t)n * k);
  const size_t steps = (size_t)k / 16;
  for (int row = 0; row < n; ++row)
    for (int kk = 0; kk < k; ++kk) {
      const size_t blk = (size_t)(row / 32) * steps + kk / 16;
      const size_t lane = (size_t)((kk % 16) / 8) * 32 + row % 32;
      out[blk * 512 + ((kk % 8) / 4) * 256 + lane * 4 + kk % 4] = m[(size_t)row * k + kk];
    }
  return out;
}

std::vector<float> pad_vec(const std::vector<float>& v, int n_pad) {
  std::vector<float> r(n_pad, 0.f);
  std::copy(v.begin(), v.end(), r.begin());
  return r;
}

struct CondPacker {
  std::vector<const std::vector<float>*> kernels, biases;
  std::vector<int> sizes;
  std::map<std::string, std::pair<int, int>> sites;   // parameter path of the conditioning linear -> (offset, width)
  int total = 0;
  int add(const gc_handle* h, const std::string& name, int c) {   // name: the conditioning linear's parameter path
    kernels.push_back(&h->weights.at(name + ".kernel")); biases.push_back(&h->weights.at(name + ".bias")); sizes.push_back(c);
    const int off = total;
    sites[name] = {off, c};
    total += 2 * c;
    return off;
  }
};

// Every image of one matrix m = W^T [n][k] (k % 32 == 0): float32 and S16 as given, WF16 and -- where the exact-f32
// family runs on the weight-streaming kernels (wf32) -- WF32 with K zero-padded to kf (a multiple of 64: the ring walks
// 4 k16 steps).  The only caller of the encoders besides build_embed_cache.
int upload_weight(gc_handle* h, const std::vector<float>& m, int n, int k, int kf, bool wf32, Weight* w) {
  BufferGroup* own = &h->weight_allocs;
  *w = Weight{};
  w->ld = k; w->kf = kf;
  int rc;
  if ((rc = dev_upload(h, &w->t, m, own)) || (rc = dev_upload(h, &w->s, encode_s16(m, n, k), own))) return rc;
  std::vector<float> padded;
  if (kf != k) {
    padded.assign((size_t)n * kf, 0.f);
    for (int r = 0; r < n; ++r) std::copy(m.begin() + (size_t)r * k, m.begin() + (size_t)(r + 1) * k, padded.begin() + (size_t)r * kf);
  }
  const std::vector<float>& mp = kf != k ? padded : m;
  if ((rc = dev_upload(h, &w->f, encode_wf16(mp, n, kf), own))) return rc;
  if (wf32 && (rc = dev_upload(h, &w->x, encode_wf32(mp, n, kf), own))) return rc;
  return GC_OK;
}

// one fused launch's weights: (k1 [n_in][n_hid], b1) -> activation -> (k2 [n_hid][n_out], b2)
int upload_mlp_pair(gc_handle* h, const std::vector<float>& k1, const std::vector<float>& b1,
                    const std::vector<float>& k2, const std::vector<float>& b2, int n_in, int in_begin, int in_count,
                    int in_pad, int n_hid, int n_out, DevMlp* out) {
  const int n_out_pad = round_up(n_out, 128);
  int rc;
  const auto w1 = transpose_pad(k1, n_in, n_hid, in_begin, in_count, in_pad, n_hid);
  const auto w2 = transpose_pad(k2, n_hid, n_out, 0, n_hid, n_hid, n_out_pad);
  if ((rc = upload_weight(h, w1, n_hid, in_pad, round_up(in_pad, 64), h->f32_ws, &out->w1))) return rc;
  if ((rc = upload_weight(h, w2, n_out_pad, n_hid, n_hid, h->f32_ws, &out->w2))) return rc;
  if ((rc = dev_upload(h, &out->b1, b1, &h->weight_allocs))) return rc;
  if ((rc = dev_upload(h, &out->b2, pad_vec(b2, n_out_pad), &h->weight_allocs))) return rc;
  out->n_out = n_out;
  out->n_out_pad = n_out_pad;
  out->cond_off = -1;
  return GC_OK;
}

int upload_mlp(gc_handle* h, const std::string& p, int n_in, int in_begin, int in_count, int in_pad,
               int n_hid, int n_out, bool cond, CondPacker* cp, DevMlp* out) {
  const int nh = h->hidden_layers;
  auto kern = [&](int i) -> const std::vector<float>& { return h->weights.at(p + ".network.network.layers." + std::to_string(2 * i) + ".kernel"); };
  auto bias = [&](int i) -> const std::vector<float>& { return h->weights.at(p + ".network.network.layers." + std::to_string(2 * i) + ".bias"); };
  int rc;
  out->pre.clear();
  if (nh == 1) {
    if ((rc = upload_mlp_pair(h, kern(0), bias(0), kern(1), bias(1), n_in, in_begin, in_count, in_pad, n_hid, n_out, out))) return rc;
  } else {
    // layers 0 .. nh-2: Linear -> activation, each as a fused launch whose second layer is the identity (no LayerNorm,
    // no conditioning): u = act(x W_i + b_i), u I + 0 = u.  Layer nh-1 and the output Linear are the usual pair.
    std::vector<float> eye((size_t)n_hid * n_hid, 0.f), zero((size_t)n_hid, 0.f);
    for (int i = 0; i < n_hid; ++i) eye[(size_t)i * n_hid + i] = 1.f;
    out->pre.resize(nh - 1);
    for (int i = 0; i + 1 < nh; ++i) {
      if (i == 0) rc = upload_mlp_pair(h, kern(0), bias(0), eye, zero, n_in, in_begin, in_count, in_pad, n_hid, n_hid, &out->pre[0]);
      else rc = upload_mlp_pair(h, kern(i), bias(i), eye, zero, n_hid, 0, n_hid, n_hid, n_hid, n_hid, &out->pre[i]);
      if (rc) return rc;
    }
    if ((rc = upload_mlp_pair(h, kern(nh - 1), bias(nh - 1), kern(nh), bias(nh), n_hid, 0, n_hid, n_hid, n_hid, n_out, out))) return rc;
  }
  if (cond) out->cond_off = cp->add(h, p + ".norm_conditioning_layer.conditional_linear_layer", n_out);
  return GC_OK;
}

// Split first layer of the grid embedding for the current weights and noisy slots (gc_handle::embed_cache).  Its four
// images replace those of the previous build; d_xn / d_pstat are allocated once.
int build_embed_cache(gc_handle* h) {
  h->embed_cache_ready = false;
  if (!h->embed_cache || !h->finalized_weights || !h->has_slots || h->hidden_layers != 1) return GC_OK;
  const gc_config& c = h->cfg;
  const int L = c.latent_size, node_in = 3 + c.c_in, kp = h->kp;
  const std::string p = std::string(P_G2M) + ".embedder_network.embed_node_fns.grid_nodes.network.network.layers.0.kernel";
  const auto& k1 = h->weights.at(p);                          // [node_in][L]
  int rc;
  drop_sample_graphs(h);                                      // captured samples bake these images' addresses
  h->cache_allocs.free();                                     // (callers have synchronised the stream)
  BufferGroup* own = &h->cache_allocs;
  auto wst = transpose_pad(k1, node_in, L, 0, node_in, kp, L);   // [L][kp]
  for (int o = 0; o < L; ++o)
    for (int cc = 0; cc < c.c_out; ++cc) wst[(size_t)o * kp + 3 + h->h_slots[cc]] = 0.f;
  if ((rc = dev_upload(h, &h->w1st_t, wst, own))) return rc;
  if ((rc = dev_upload(h, &h->w1st_s, encode_s16(wst, L, kp), own))) return rc;
  h->nwp = round_up(c.c_out, 32);
  const int k1e = round_up(h->nwp, 64);
  std::vector<float> wn((size_t)L * k1e, 0.f);                // [L][k1e]: column cc = kernel row 3 + slots[cc]
  for (int cc = 0; cc < c.c_out; ++cc)
    for (int o = 0; o < L; ++o) wn[(size_t)o * k1e + cc] = k1[(size_t)(3 + h->h_slots[cc]) * L + o];
  DevMlp& n = h->g2m_embed_grid_n;
  n = h->g2m_embed_grid;                                      // second layer, biases, conditioning: shared
  n.w1e = Weight{};                                           // streaming images only (make_route: embed_cache)
  n.w1e.kf = k1e; n.w1e.ld = h->nwp;
  if ((rc = dev_upload(h, &n.w1e.f, encode_wf16(wn, L, k1e), own))) return rc;
  if (h->f32_ws && (rc = dev_upload(h, &n.w1e.x, encode_wf32(wn, L, k1e), own))) return rc;
  if (!h->d_xn) {
    const size_t GB = (size_t)h->hg.G * c.batch;
    if ((rc = dev_alloc(h, &h->d_xn, GB * h->nwp))) return rc;
    if ((rc = dev_alloc(h, &h->d_pstat, GB * L))) return rc;
    GC_HIP(h, hipMemset(h->d_xn, 0, GB * h->nwp * sizeof(float)));   // the padding columns stay zero for good
  }
  h->embed_cache_ready = true;
  return GC_OK;
}

// Frees what finalize_weights allocated (the stream is idle and no captured sample is left: gc_finalize, destroy).
void free_weights(gc_handle* h) {
  (void)drop_edge_terms(h);                     // made from these weights
  h->weight_allocs.free();
  h->finalized = h->finalized_weights = h->embed_cache_ready = false;
  h->cond_cur = nullptr;                        // (it may point into the d_cond just freed)
}

// The body of gc_finalize: every weight image, the packed conditioning linears, the noise encoder.
int finalize_weights(gc_handle* h) {
  const gc_config& c = h->cfg;
  const int L = c.latent_size, D = c.d_model, F = c.ffw_hidden;
  const std::string g = P_G2M, m = P_M2G, t = P_TR, nz = P_NOISE;
  BufferGroup* own = &h->weight_allocs;
  CondPacker cp;
  int rc;
  const int node_in = 3 + c.c_in;
  const std::string gn = g + ".processor_networks.0.graph_network";
  const std::string gn2 = m + ".processor_networks.0.graph_network";
  if (h->hidden_layers >= 2) {
    // every MLP is a chain of launches (run_mlp): the algebraic edge-MLP split assumes ONE launch
    h->split_edge = false;
    if (!h->d_mlp_tmp[0]) {
      const size_t rows = (size_t)std::max(std::max(h->hg.G, h->hg.M), std::max(h->hg.E1, h->hg.E2)) * (size_t)c.batch;
      for (int i = 0; i < 2; ++i)
        if ((rc = dev_alloc(h, &h->d_mlp_tmp[i], rows * (size_t)L))) return rc;
    }
  }
  if ((rc = upload_mlp(h, g + ".embedder_network.embed_node_fns.grid_nodes", node_in, 0, node_in, h->kp, L, L, true, &cp, &h->g2m_embed_grid))) return rc;
  // mesh nodes see [struct(3) | zeros(c_in)] (denoiser.py:661-668): only the first 3 kernel rows matter.
  if ((rc = upload_mlp(h, g + ".embedder_network.embed_node_fns.mesh_nodes", node_in, 0, 3, 32, L, L, true, &cp, &h->g2m_embed_mesh))) return rc;
  if ((rc = upload_mlp(h, g + ".embedder_network.embed_edge_fns.grid2mesh", 4, 0, 4, 32, L, L, true, &cp, &h->g2m_embed_edge))) return rc;
  if ((rc = upload_mlp(h, gn + ".update_edge_fns.grid2mesh.edge_fn", 3 * L, 0, 3 * L, 3 * L, L, L, true, &cp, &h->g2m_edge))) return rc;
  if ((rc = upload_mlp(h, gn + ".update_node_fns.mesh_nodes.node_fn", 2 * L, 0, 2 * L, 2 * L, L, L, true, &cp, &h->g2m_mesh))) return rc;
  if ((rc = upload_mlp(h, gn + ".update_node_fns.grid_nodes.node_fn", L, 0, L, L, L, L, true, &cp, &h->g2m_grid))) return rc;
  if ((rc = upload_mlp(h, m + ".embedder_network.embed_edge_fns.mesh2grid", 4, 0, 4, 32, L, L, true, &cp, &h->m2g_embed_edge))) return rc;
  if ((rc = upload_mlp(h, gn2 + ".update_edge_fns.mesh2grid.edge_fn", 3 * L, 0, 3 * L, 3 * L, L, L, true, &cp, &h->m2g_edge))) return rc;
  if ((rc = upload_mlp(h, gn2 + ".update_node_fns.grid_nodes.node_fn", 2 * L, 0, 2 * L, 2 * L, L, L, true, &cp, &h->m2g_grid))) return rc;
  if ((rc = upload_mlp(h, m + ".decoder_network.embed_node_fns.grid_nodes", L, 0, L, L, L, c.c_out, false, &cp, &h->m2g_dec))) return rc;

  // the edge MLPs' first layer once more, by input block [e | sender | receiver] (K = L; the per-node blocks run on the
  // f16x3 weight-streaming GEMM or the LDS-staged one: no WF32 image)
  for (DevMlp* em : {&h->g2m_edge, &h->m2g_edge}) {
    const std::string pth = (em == &h->g2m_edge) ? gn + ".update_edge_fns.grid2mesh.edge_fn"
                                                 : gn2 + ".update_edge_fns.mesh2grid.edge_fn";
    const auto& k1 = h->weights.at(pth + ".network.network.layers.0.kernel");   // [3L][L]
    if ((rc = upload_weight(h, transpose_pad(k1, 3 * L, L, 0, L, L, L), L, L, L, h->f32_ws, &em->w1e))) return rc;
    if ((rc = upload_weight(h, transpose_pad(k1, 3 * L, L, L, L, L, L), L, L, L, false, &em->w1snd))) return rc;
    if ((rc = upload_weight(h, transpose_pad(k1, 3 * L, L, 2 * L, L, L, L), L, L, L, false, &em->w1rcv))) return rc;
  }
  h->layers.assign(c.num_layers, DevLayer());
  for (int i = 0; i < c.num_layers; ++i) {
    const std::string b = t + ".blocks." + std::to_string(i);
    DevLayer& ly = h->layers[i];
    auto wt = [&](const char* name, int n_in, int n_out) {   // W^T [n_out][n_in] of a Linear of this block
      return transpose_pad(h->weights.at(b + name), n_in, n_out, 0, n_in, n_in, n_out);
    };
    std::vector<float> qkv((size_t)3 * D * D);
    int part = 0;
    for (const char* q : {"q", "k", "v"}) {
      const auto tt = wt((std::string(".attn_module.") + q + "_proj.linear.kernel").c_str(), D, D);
      std::copy(tt.begin(), tt.end(), qkv.begin() + (size_t)part++ * D * D);
    }
    if ((rc = upload_weight(h, qkv, 3 * D, D, D, h->f32_ws, &ly.wqkv))) return rc;
    if ((rc = upload_weight(h, wt(".attn_module.final_linear.kernel", D, D), D, D, D, h->f32_ws, &ly.wo))) return rc;
    if ((rc = upload_weight(h, wt(".ffw_module.mlp.layers.0.kernel", D, F), F, D, D, h->f32_ws, &ly.w1))) return rc;
    if ((rc = upload_weight(h, wt(".ffw_module.mlp.layers.2.kernel", F, D), D, F, F, h->f32_ws, &ly.w2))) return rc;
    if ((rc = dev_upload(h, &ly.bo, h->weights.at(b + ".attn_module.final_linear.bias"), own))) return rc;
    if ((rc = dev_upload(h, &ly.b1, h->weights.at(b + ".ffw_module.mlp.layers.0.bias"), own))) return rc;
    if ((rc = dev_upload(h, &ly.b2, h->weights.at(b + ".ffw_module.mlp.layers.2.bias"), own))) return rc;
    ly.cond_attn = cp.add(h, b + ".norm_cond_attn.conditional_linear_layer", D);
    ly.cond_ffw = cp.add(h, b + ".norm_cond_ffw.conditional_linear_layer", D);
  }
  h->cond_final = cp.add(h, t + ".final_norm_cond.conditional_linear_layer", D);

  // all conditioning linears side by side: wc_all[16][total], bc_all[total] (+1 folded into scales)
  h->cond_total = cp.total;
  h->cond_sites = cp.sites;
  std::vector<float> wc((size_t)gc::kCondDim * cp.total), bc(cp.total);
  int off = 0;
  for (size_t li = 0; li < cp.kernels.size(); ++li) {
    const int cdim = cp.sizes[li];
    const auto& k = *cp.kernels[li];
    const auto& b = *cp.biases[li];
    for (int i = 0; i < gc::kCondDim; ++i)
      for (int j = 0; j < 2 * cdim; ++j) wc[(size_t)i * cp.total + off + j] = k[(size_t)i * 2 * cdim + j];
    for (int j = 0; j < 2 * cdim; ++j) bc[off + j] = b[j] + (j < cdim ? 1.0f : 0.0f);
    off += 2 * cdim;
  }
  if ((rc = dev_upload(h, &h->d_wc_all, wc, own))) return rc;
  if ((rc = dev_upload(h, &h->d_bc_all, bc, own))) return rc;
  if ((rc = dev_alloc(h, &h->d_cond, (size_t)c.batch * cp.total, own))) return rc;

  const int nf2 = 2 * c.noise_num_frequencies;
  if ((rc = dev_upload(h, &h->d_nw0t, transpose_pad(h->weights.at(nz + ".linear_0.kernel"), nf2, c.noise_hidden, 0, nf2, nf2, c.noise_hidden), own))) return rc;
  if ((rc = dev_upload(h, &h->d_nb0, h->weights.at(nz + ".linear_0.bias"), own))) return rc;
  if ((rc = dev_upload(h, &h->d_nw1t, transpose_pad(h->weights.at(nz + ".linear_1.kernel"), c.noise_hidden, gc::kCondDim, 0, c.noise_hidden, c.noise_hidden, gc::kCondDim), own))) return rc;
  if ((rc = dev_upload(h, &h->d_nb1, h->weights.at(nz + ".linear_1.bias"), own))) return rc;

  // f16x3 domain of the weights: a non-finite or > fp16-max weight cannot be split, so such a model
  // runs on the exact-f32 kernels only (the reference's f32 arithmetic has no such limit)
  h->weights_f16_unsafe = false;
  for (const auto& kv : h->weights)
    for (float w : kv.second)
      if (!(std::fabs(w) <= 65504.0f)) { h->weights_f16_unsafe = true; break; }
  if ((rc = compute_static_embeddings(h))) return rc;
  h->finalized = true;
  h->finalized_weights = true;
  return build_embed_cache(h);
}

}  // namespace gci
