// C ABI of libgencast_hip.so (include/gencast_hip.h): every extern "C" entry point, and the RCCL binding of the
// ensemble exchange.  The work is in gc_weights.hip, gc_forward.hip and gc_sampler.hip.
#include <dlfcn.h>

#include "gc_handle.h"

using namespace gci;

namespace {

// Entry points that overwrite the initial noise while a sample's domain check is pending write the OTHER buffer.
void protect_pending_noise(gc_handle* h) {
  if (h->guard_pending && h->d_noise == h->last_noise) std::swap(h->d_noise, h->d_noise_alt);
}

int check_ready(gc_handle* h) {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!h->finalized) return fail(h, GC_ERR_STATE, "gc_finalize has not been called");
  return GC_OK;
}

// ---- RCCL, bound at run time ----------------------------------------------------------------------
// The denoiser itself never communicates; only the ensemble driver's one exchange per forecast step
// does.  librccl is therefore not a link-time dependency: a single-GPU user (or a CPU-only box that
// only checks the ABI) never loads it.
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string error;
};

Rccl& rccl() {
  static Rccl r = [] {
    Rccl x;
    const char* override_path = std::getenv("GC_RCCL_LIBRARY");
    // ROCm's own library first: by search path the name resolved to the copy inside torch's wheel on a test box
    // (profiles/r03_gpu_tests.log); GC_RCCL_LIBRARY overrides
    for (const char* name : {override_path ? override_path : "/opt/rocm/lib/librccl.so.1", "librccl.so.1", "librccl.so"}) {
      x.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (x.lib) break;
    }
    if (!x.lib) {
      x.error = std::string("cannot load librccl: ") + dlerror();
      return x;
    }
    auto sym = [&](const char* n) {
      void* p = dlsym(x.lib, n);
      if (!p && x.error.empty()) x.error = std::string("librccl lacks ") + n;
      return p;
    };
    x.GetUniqueId = reinterpret_cast<decltype(x.GetUniqueId)>(sym("ncclGetUniqueId"));
    x.CommInitRank = reinterpret_cast<decltype(x.CommInitRank)>(sym("ncclCommInitRank"));
    x.CommDestroy = reinterpret_cast<decltype(x.CommDestroy)>(sym("ncclCommDestroy"));
    x.CommCount = reinterpret_cast<decltype(x.CommCount)>(sym("ncclCommCount"));
    x.CommUserRank = reinterpret_cast<decltype(x.CommUserRank)>(sym("ncclCommUserRank"));
    x.Broadcast = reinterpret_cast<decltype(x.Broadcast)>(sym("ncclBroadcast"));
    x.AllReduce = reinterpret_cast<decltype(x.AllReduce)>(sym("ncclAllReduce"));
    x.GetErrorString = reinterpret_cast<decltype(x.GetErrorString)>(sym("ncclGetErrorString"));
    return x;
  }();
  return r;
}

#define GC_NCCL(h, call)                                                                    \
  do {                                                                                      \
    ncclResult_t r__ = (call);                                                              \
    if (r__ != ncclSuccess) {                                                               \
      (h)->err = std::string(#call) + ": " + rccl().GetErrorString(r__);                    \
      return GC_ERR_COMM;                                                                   \
    }                                                                                       \
  } while (0)

// The counters of the units that keep a Meter.  A unit with a regular name has <prefix>_calls, <prefix>_device_us and
// <prefix>_blocks (Meter, gc_handle.h), and <prefix>_invalid_points where it counts skipped points; the names that do not
// follow are rows of their own.
const int64_t* meter_counter(const gc_handle* h, const std::string& n) {
  struct Unit { const char* prefix; Meter gc_handle::*meter; bool invalid_points; };
  static const Unit units[] = {
      {"ens_event", &gc_handle::evt, true},     {"ens_derive", &gc_handle::drv, false}, {"ens_band", &gc_handle::band, false},
      {"ens_order", &gc_handle::ord, true},     {"ens_clim", &gc_handle::clim, true},   {"ens_energy", &gc_handle::en, true},
      {"ens_variogram", &gc_handle::vg, false}, {"ens_tail", &gc_handle::tail, true},   {"ens_region", &gc_handle::reg, true},
      {"ens_feature", &gc_handle::feat, false}, {"ens_fss", &gc_handle::fss, false},  {"ens_efi", &gc_handle::efi, true},
      {"ens_map", &gc_handle::map, true}};
  struct Row { const char* name; Meter gc_handle::*meter; int64_t Meter::*field; };
  static const Row rows[] = {
      {"ens_scores", &gc_handle::ens, &Meter::calls},
      {"ens_score_device_us", &gc_handle::ens, &Meter::device_us},
      {"ens_invalid_points", &gc_handle::ens, &Meter::invalid},
      {"ens_score_blocks", &gc_handle::ens, &Meter::blocks},
      {"ens_fss_chunks", &gc_handle::fss, &Meter::chunks},
      {"spec_calls", &gc_handle::spec, &Meter::calls},
      {"spec_device_us", &gc_handle::spec, &Meter::device_us},
      {"spec_invalid_columns", &gc_handle::spec, &Meter::invalid},
      {"ens_band_invalid_columns", &gc_handle::band, &Meter::invalid},
      {"ens_window_emits", &gc_handle::win, &Meter::calls},
      {"ens_window_device_us", &gc_handle::win, &Meter::device_us}};
  for (const Row& r : rows)
    if (n == r.name) return &(h->*r.meter.*r.field);
  for (const Unit& u : units) {
    const size_t len = std::strlen(u.prefix);
    if (n.compare(0, len, u.prefix) != 0) continue;
    const Meter& m = h->*u.meter;
    if (n.compare(len, std::string::npos, "_calls") == 0) return &m.calls;
    if (n.compare(len, std::string::npos, "_device_us") == 0) return &m.device_us;
    if (n.compare(len, std::string::npos, "_blocks") == 0) return &m.blocks;
    if (u.invalid_points && n.compare(len, std::string::npos, "_invalid_points") == 0) return &m.invalid;
  }
  return nullptr;
}

}  // namespace

// =================================================================================================
static void destroy_impl(gc_handle* h);

extern "C" {

int gc_abi_version(void) { return GC_ABI_VERSION; }

const char* gc_build_info(void) {
#ifndef GC_SOURCE_HASH
#define GC_SOURCE_HASH "unknown"
#endif
  return "libgencast_hip gfx950 f16x3/f32-mfma " __DATE__ " " __TIME__ " src:" GC_SOURCE_HASH;
}

int gc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int gc_device_pci_bus_id(int32_t device_id, char* out, int64_t cap) {
  if (!out || cap < 16 || device_id < 0 || device_id >= gc_device_count()) return GC_ERR_INVALID_ARGUMENT;
  out[0] = 0;
  return hipDeviceGetPCIBusId(out, (int)cap, device_id) == hipSuccess ? GC_OK : GC_ERR_HIP;
}

const char* gc_last_error(const gc_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

// The environment switches, all read here, once per handle (gc_create).  GC_PRECISION and GC_TUNE_GRAPH set the
// defaults of gc_set_option's "precision" and "graphs"; M2G_FUSE_SUM, EMBED_CACHE, ATTN_ITEMS, MLP_PAIR, EDGE_TERMS and A16 select
// the other form of a fused path (the tests' bit-identity references); GRAPH_SERIALIZE and GRAPH_VERBOSE are the
// graph-replay safety valve and its diagnostics (run_sampler).  GC_DEBUG_POISON=1 makes dev_alloc fill every new buffer
// (gc_handle.h; never timed).
static void read_switches(gc_handle* h) {
  auto is = [](const char* name, const char* value) { const char* v = std::getenv(name); return v && std::string(v) == value; };
  auto off = [](const char* name) { const char* v = std::getenv(name); return v && *v && std::atoi(v) == 0; };
  auto on = [](const char* name) { const char* v = std::getenv(name); return v && *v == '1'; };
  h->f16x3 = !is("GC_PRECISION", "f32");
  h->use_graphs = !is("GC_TUNE_GRAPH", "0");
  h->m2g_fuse_sum = !off("GC_TUNE_M2G_FUSE_SUM");
  h->embed_cache = !off("GC_TUNE_EMBED_CACHE");
  h->attn_items = !off("GC_TUNE_ATTN_ITEMS");
  h->mlp_pair = !off("GC_TUNE_MLP_PAIR");
  h->edge_terms = !off("GC_TUNE_EDGE_TERMS");
  h->a16 = !off("GC_TUNE_A16");
  h->graph_serialize = on("GC_TUNE_GRAPH_SERIALIZE");
  h->graph_verbose = on("GC_TUNE_GRAPH_VERBOSE");
  h->poison = on("GC_DEBUG_POISON");
}

int gc_create(const gc_config* cfg, int device_id, gc_handle** out) {
  return guarded(nullptr, [&]() -> int {
  if (!cfg || !out) { g_create_error = "null argument"; return GC_ERR_INVALID_ARGUMENT; }
  *out = nullptr;
  const gc_config& c = *cfg;
  auto bad = [&](const char* m) { g_create_error = m; return GC_ERR_INVALID_ARGUMENT; };
  if (c.latent_size <= 0 || c.d_model <= 0 || c.num_heads <= 0 || c.ffw_hidden <= 0 ||
      c.num_layers < 0 || c.c_in <= 0 || c.c_out <= 0 || c.batch <= 0)
    return bad("all dimensions must be positive");
  if (c.c_out > c.c_in) return bad("c_out cannot exceed c_in (noisy targets are part of the forcings)");
  if (c.latent_size != c.d_model) return bad("latent_size must equal d_model");
  if (c.d_model % c.num_heads) return bad("num_heads has to divide d_model exactly");
  if (c.noise_num_frequencies <= 0 || c.noise_num_frequencies > 128 || c.noise_hidden <= 0 ||
      c.noise_hidden > 128 || !(c.noise_base_period > 0))
    return bad("noise encoder sizes out of range");
  auto unsup = [&](const char* m) { g_create_error = m; return GC_ERR_UNSUPPORTED; };
  if (c.latent_size != 128 && c.latent_size != 256 && c.latent_size != 512)
    return unsup("latent_size must be 128, 256 or 512 (MFMA column tiling)");
  const int dh = c.d_model / c.num_heads;
  if (dh != 32 && dh != 64 && dh != 128) return unsup("head size must be 32, 64 or 128");
  if (c.num_heads > 8) return unsup("at most 8 heads");
  if (c.ffw_hidden % 128) return unsup("ffw_hidden must be a multiple of 128");
  if (c.c_out > 512) return unsup("c_out must be <= 512");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    g_create_error = "no HIP device visible (this library has no CPU fallback)";
    return GC_ERR_NO_DEVICE;
  }
  if (device_id < 0 || device_id >= ndev) { g_create_error = "device_id out of range"; return GC_ERR_NO_DEVICE; }
  std::unique_ptr<gc_handle> h(new gc_handle());
  h->cfg = c;
  h->device = device_id;
  hipError_t e = hipSetDevice(device_id);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&h->ev0);
  if (e == hipSuccess) e = hipEventCreate(&h->ev1);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_pin, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_nonfinite, sizeof(unsigned));
  if (e == hipSuccess) e = hipMemset(h->d_nonfinite, 0, sizeof(unsigned));
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_nonfinite, sizeof(unsigned), hipHostMallocDefault);
  if (e != hipSuccess) {
    g_create_error = hipGetErrorString(e);
    gc_destroy(h.release());
    return GC_ERR_HIP;
  }
  *h->h_nonfinite = 0;
  h->kp = round_up(3 + c.c_in, 32);
  read_switches(h.get());
  build_specs(h.get());
  *out = h.release();
  return GC_OK;
  });
}

void gc_destroy(gc_handle* h) {
  if (!h) return;
  try {
    destroy_impl(h);
  } catch (...) {
  }
}

static void destroy_impl(gc_handle* h) {
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  drop_sample_graphs(h);
  if (h->comm) (void)rccl().CommDestroy(h->comm);
  for (gc_handle::CtxSlot& c : h->ctx) {            // context copies run on other handles' streams
    if (c.saved) (void)hipEventSynchronize(c.ev_w);
    if (c.read) (void)hipEventSynchronize(c.ev_r);
  }
  for (BufferGroup* g : h->groups) g->free();
  if (h->d_nonfinite) (void)hipFree(h->d_nonfinite);
  for (void* p : {(void*)h->h_nonfinite, (void*)h->pin_cond, (void*)h->pin_noise, (void*)h->pin_forc,
                  (void*)h->pin_lguard})
    if (p) (void)hipHostFree(p);
  if (h->ev_pin) (void)hipEventDestroy(h->ev_pin);
  if (h->ev_stash) (void)hipEventDestroy(h->ev_stash);
  for (Event* e : h->events)
    if (e->e) (void)hipEventDestroy(e->e);
  for (gc_handle::CtxSlot& c : h->ctx)
    for (hipEvent_t e : {c.ev_w, c.ev_r})
      if (e) (void)hipEventDestroy(e);
  if (h->stream2) {
    (void)hipStreamSynchronize(h->stream2);
    (void)hipStreamDestroy(h->stream2);
  }
  for (hipEvent_t e : h->prof_events) (void)hipEventDestroy(e);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int gc_set_option(gc_handle* h, const char* key, const char* value) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!key || !value) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  const std::string k(key), v(value);
  // A pending exact-f32 re-run of the LAST sample (f16x3 domain guard) belongs to the mode that sample was drawn in:
  // it is resolved BEFORE a flag changes (the flags are part of the forward's identity -- fp16 storage, graph signature).
  auto settle = [&]() -> int {
    if (!h->finalized) return GC_OK;
    GC_HIP(h, hipSetDevice(h->device));
    return resolve_guard(h);
  };
  if (k == "precision") {
    if (v != "f16x3" && v != "f32") return fail(h, GC_ERR_INVALID_ARGUMENT, "precision must be f16x3 or f32");
    const bool want = v == "f16x3";
    if (want == h->f16x3) return GC_OK;
    if (int rc = settle()) return rc;
    h->f16x3 = want;
    return h->finalized ? compute_static_embeddings(h) : GC_OK;   // the static embeddings follow the precision
  }
  if (k == "hidden_layers") {
    // DenoiserArchitectureConfig.hidden_layers (gencast/denoiser.py:108,135,374,402 -> common/mlp.py:157-199): hidden
    // layers of every MLP of the two GNNs.  It fixes the parameter names, so it is set before any weight is loaded.
    char* end = nullptr;
    const long n = std::strtol(v.c_str(), &end, 10);
    if (v.empty() || (end && *end) || n < 1 || n > 4) return fail(h, GC_ERR_INVALID_ARGUMENT, "hidden_layers must be in 1..4");
    if ((int)n == h->hidden_layers) return GC_OK;
    if (h->finalized || !h->weights.empty())
      return fail(h, GC_ERR_STATE, "hidden_layers must be set before the first gc_load_weight");
    h->hidden_layers = (int)n;
    h->specs.clear();
    build_specs(h);
    return GC_OK;
  }
  if (k == "features") {
    if (v != "f16" && v != "f32") return fail(h, GC_ERR_INVALID_ARGUMENT, "features must be f32 or f16");
    const bool want = v == "f16";
    if (want == h->feat16) return GC_OK;
    if (int rc = settle()) return rc;
    h->feat16 = want;
    return h->finalized ? compute_static_embeddings(h) : GC_OK;   // their internal roundings follow the mode
  }
  if (k == "grid2mesh_aggregate_normalization") {
    // DenoiserArchitectureConfig.grid2mesh_aggregate_normalization (gencast/denoiser.py:123,138,367): the summed
    // grid2mesh edge messages of every mesh node are divided by this constant (deep_typed_graph_net.py:396-410);
    // "0" or "none": not normalised (the reference default)
    char* end = nullptr;
    const float f = (v == "none" || v.empty()) ? 0.f : std::strtof(v.c_str(), &end);
    if ((end && *end) || !(f >= 0.f) || !std::isfinite(f))
      return fail(h, GC_ERR_INVALID_ARGUMENT, "grid2mesh_aggregate_normalization must be a non-negative number");
    if (f == h->g2m_agg_norm) return GC_OK;
    if (int rc = settle()) return rc;
    h->g2m_agg_norm = f;
    drop_sample_graphs(h);                       // the constant is a kernel argument baked into captured samples
    return GC_OK;
  }
  if (k == "edge_term_cache_mb") {
    // cap of the edge-term cache (gc_handle::EdgeTerms): a noise-level list whose terms need more keeps the products
    char* end = nullptr;
    const long long mb = std::strtoll(v.c_str(), &end, 10);
    if (v.empty() || (end && *end) || mb < 0 || mb > (1ll << 24)) return fail(h, GC_ERR_INVALID_ARGUMENT, "edge_term_cache_mb must be a number of MiB, 0 .. 2^24");
    if (mb == h->edge_term_cap_mb) return GC_OK;
    if (int rc = settle()) return rc;
    h->edge_term_cap_mb = mb;
    drop_sample_graphs(h);                       // captured samples bake the route
    return drop_edge_terms(h);                   // the next sample decides again
  }
  if (k == "graphs") {
    if (v == "on") h->use_graphs = true;
    else if (v == "off") h->use_graphs = false;
    else return fail(h, GC_ERR_INVALID_ARGUMENT, "graphs must be on or off");
    return GC_OK;
  }
  return fail(h, GC_ERR_INVALID_ARGUMENT, "unknown option: " + k);
  });
}

int gc_set_graph(gc_handle* h, int32_t G, int32_t M, int32_t E1, const int32_t* g2m_s,
                 const int32_t* g2m_r, int32_t E2, const int32_t* m2g_s, const int32_t* m2g_r,
                 const int32_t* khop_rowptr, const int32_t* khop_cols, const float* grid_struct,
                 const float* mesh_struct, const float* g2m_edge_struct, const float* m2g_edge_struct,
                 const float* mesh_xyz) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (h->has_graph) return fail(h, GC_ERR_STATE, "graph already set on this handle");
  if (!g2m_s || !g2m_r || !m2g_s || !m2g_r || !khop_rowptr || !khop_cols || !grid_struct ||
      !mesh_struct || !g2m_edge_struct || !m2g_edge_struct)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "null graph array");
  std::string msg = gc::build_host_graph(G, M, E1, g2m_s, g2m_r, E2, m2g_s, m2g_r, khop_rowptr,
                                         khop_cols, mesh_xyz, &h->hg);
  if (!msg.empty()) return fail(h, GC_ERR_INVALID_ARGUMENT, msg);
  GC_HIP(h, hipSetDevice(h->device));
  const gc::HostGraph& g = h->hg;
  int rc;
  const std::pair<int**, const std::vector<int>*> index_arrays[] = {
      {&h->d_g2m_snd, &g.g2m_snd}, {&h->d_g2m_rcv, &g.g2m_rcv}, {&h->d_m2g_snd, &g.m2g_snd}, {&h->d_m2g_rcv, &g.m2g_rcv},
      {&h->d_g2m_ptr, &g.g2m_ptr}, {&h->d_g2m_eid, &g.g2m_eid}, {&h->d_m2g_ptr, &g.m2g_ptr}, {&h->d_m2g_eid, &g.m2g_eid},
      {&h->d_tile_start, &g.tile_chunk_start}};
  for (const auto& a : index_arrays)
    if ((rc = dev_upload(h, a.first, *a.second))) return rc;
  {
    std::vector<int> items, tiles;
    h->att_n_items = 0;
    if (h->attn_items && h->cfg.batch == 1 && h->cfg.num_heads <= 4 &&
        h->cfg.d_model / h->cfg.num_heads == 128 && build_attention_items(g, &items, &tiles)) {
      if ((rc = dev_upload(h, &h->d_att_items, items))) return rc;
      if ((rc = dev_upload(h, &h->d_att_tiles, tiles))) return rc;
      h->att_n_items = (int)(items.size() / 4);
    }
  }
  h->max_tile_chunks = 0;
  for (int t = 0; t < g.n_tiles; ++t)
    h->max_tile_chunks = std::max(h->max_tile_chunks, g.tile_chunk_start[t + 1] - g.tile_chunk_start[t]);
  if ((rc = dev_upload(h, &h->d_union, g.union_idx))) return rc;
  if ((rc = dev_upload(h, &h->d_mask, g.mask_bits))) return rc;
  if ((rc = dev_upload(h, &h->d_grid_struct, std::vector<float>(grid_struct, grid_struct + (size_t)G * 3)))) return rc;
  std::vector<float> ms16((size_t)M * 32, 0.f), e1s((size_t)E1 * 32, 0.f), e2s((size_t)E2 * 32, 0.f);
  for (int i = 0; i < M; ++i)           // internal mesh order
    for (int k = 0; k < 3; ++k) ms16[(size_t)i * 32 + k] = mesh_struct[(size_t)g.perm[i] * 3 + k];
  for (int e = 0; e < E1; ++e)
    for (int k = 0; k < 4; ++k) e1s[(size_t)e * 32 + k] = g2m_edge_struct[(size_t)e * 4 + k];
  for (int e = 0; e < E2; ++e)
    for (int k = 0; k < 4; ++k) e2s[(size_t)e * 32 + k] = m2g_edge_struct[(size_t)g.m2g_order[e] * 4 + k];   // internal edge order
  if ((rc = dev_upload(h, &h->d_mesh_struct16, ms16))) return rc;
  if ((rc = dev_upload(h, &h->d_e1_struct16, e1s))) return rc;
  if ((rc = dev_upload(h, &h->d_e2_struct16, e2s))) return rc;

  // activations
  const gc_config& c = h->cfg;
  const size_t B = c.batch, L = c.latent_size, D = c.d_model, F = c.ffw_hidden;
  const size_t GB = (size_t)G * B, MB = (size_t)M * B;
  auto alloc_all = [&](std::initializer_list<std::pair<float**, size_t>> bufs) {
    for (const auto& b : bufs)
      if (int r = dev_alloc(h, b.first, b.second)) return r;
    return (int)GC_OK;
  };
  if ((rc = alloc_all({{&h->d_sigma, B}, {&h->d_condvec, B * gc::kCondDim}, {&h->d_feats, GB * c.c_in}, {&h->d_xp, GB * h->kp},
                       {&h->d_g0, GB * L}, {&h->d_g1, GB * L}, {&h->d_g2, GB * L}, {&h->d_agg2, GB * L}, {&h->d_m0, MB * L},
                       {&h->d_x, MB * L}, {&h->d_agg1, MB * L}, {&h->d_m2, MB * L}, {&h->d_qkv, MB * 3 * D}, {&h->d_att, MB * D}})))
    return rc;
  {
    uint16_t* kv = nullptr;
    if ((rc = dev_alloc(h, &kv, MB * 4 * D, nullptr, true))) return rc;   // fp16 planes: poisoned as NaN
    h->d_kv16 = kv;
  }
  if ((rc = dev_alloc(h, &h->d_u, MB * F))) return rc;
  {
    auto largest_split = [](int k, int cap) {
      int best = 1;
      for (int sp = 1; sp <= cap; ++sp)
        if (k % (32 * sp) == 0) best = sp;
      return best;
    };
    // enough attention blocks to cover the 256 CUs about once
    int as = (int)std::lround(256.0 / std::max(1, h->hg.n_tiles * (int)B));
    h->attn_splits = std::min(8, std::max(1, as));
    // FFW layer 2 as a GEMM of its own (d_model 512, or the fused FFW switched off): K = ffw_hidden is split only while
    // the unsplit launch would leave CUs idle -- every split is one more float32 slab the next row pass reads.  At the
    // 1-degree size (161 row tiles x 4 column panels = 644 workgroups) 1 split vs 4: FFW-2 1.39 -> 1.33 ms and the row
    // pass 0.44 -> 0.30 ms per call, +3.2 % calls/s (float32 features), +2.5 % (fp16 features).
    const int ffw2_wgs = (int)((MB + 63) / 64) * (int)(D / 128);
    h->ffw2_splits = largest_split((int)F, ffw2_wgs >= 512 ? 1 : 4);
    h->out_splits = largest_split((int)D, 2);
    h->f32_ws = D % 128 == 0 && F % 256 == 0;
    // both FFW layers in one launch (weight-streaming form, d_model 128 / 256: see launch_ffw_fused)
    h->ffw_fused_slabs = (D % 128 == 0 && D <= 256 && F % 256 == 0 && F / 256 <= 16) ? (int)(F / 256) : 0;
    const size_t slabs = (size_t)std::max(std::max(h->ffw2_splits, h->out_splits), std::max(h->ffw_fused_slabs, 1));
    if ((rc = dev_alloc(h, &h->d_h, MB * D))) return rc;
    if ((rc = dev_alloc(h, &h->d_pg, GB * L))) return rc;
    if ((rc = dev_alloc(h, &h->d_pm, MB * L))) return rc;
    if (!h->d_ones) {
      if ((rc = dev_upload(h, &h->d_ones, std::vector<float>(2048, 1.0f)))) return rc;
      if ((rc = dev_upload(h, &h->d_zeros, std::vector<float>(2048, 0.0f)))) return rc;
    }
    // Edge MLPs with the first layer split by input block (e @ Wa + (n_s @ Wb)[senders] + (n_r @ Wc)[receivers]: the two
    // node products are computed once per NODE, 46 % of the first layer's FLOPs at the 1-degree sizes).  On the
    // weight-streaming kernels: 1 degree / latent 512 +7.6 % calls/s (float32 features) / +4.3 % (fp16 features);
    // nano / latent 256: -0.7 % (four more launches buy too little there) -- so on from latent 512.
    h->split_edge = L >= 512;
    if ((rc = dev_alloc(h, &h->d_part, slabs * MB * D))) return rc;
    const size_t aslots = (size_t)h->hg.n_tiles * h->attn_splits * B * c.num_heads;
    if ((rc = dev_alloc(h, &h->d_apart_o, aslots * 32 * (D / c.num_heads)))) return rc;
    if ((rc = dev_alloc(h, &h->d_apart_ml, aslots * 32 * 2))) return rc;
  }
  if ((rc = alloc_all({{&h->d_e1, (size_t)E1 * B * L}, {&h->d_f1, (size_t)E2 * B * L}, {&h->d_y, GB * c.c_out}, {&h->d_sx, GB * c.c_out},
                       {&h->d_sden, GB * c.c_out}, {&h->d_smid, GB * c.c_out}, {&h->d_noise, GB * c.c_out},
                       {&h->d_noise_alt, GB * c.c_out}})))
    return rc;
  if ((rc = dev_alloc(h, &h->d_slots, (size_t)c.c_out))) return rc;
  if ((rc = alloc_all({{&h->d_m0_hat, (size_t)M * L}, {&h->d_e0_hat, (size_t)E1 * L}, {&h->d_f0_hat, (size_t)E2 * L}}))) return rc;
  GC_HIP(h, hipMemset(h->d_xp, 0, GB * h->kp * sizeof(float)));
  GC_HIP(h, pinned_alloc(h, &h->pin_cond, GB * c.c_in));
  GC_HIP(h, pinned_alloc(h, &h->pin_noise, GB * c.c_out));
  h->has_graph = true;
  h->finalized = false;
  return GC_OK;
  });
}

int gc_load_weight(gc_handle* h, const char* name, const float* data, const int64_t* shape,
                   int32_t ndim) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!name || !data || !shape) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  const std::string n(name);
  const std::string dead = std::string(P_M2G) + ".processor_networks.0.graph_network.update_node_fns.mesh_nodes.";
  if (n.compare(0, dead.size(), dead) == 0) return GC_OK;  // never read by the reference either
  auto it = h->specs.find(n);
  if (it == h->specs.end()) return fail(h, GC_ERR_INVALID_ARGUMENT, "unknown parameter name: " + n);
  const auto& want = it->second;
  bool ok = ((int)want.size() == ndim);
  size_t count = 1;
  for (int i = 0; ok && i < ndim; ++i) { ok = (shape[i] == want[i]); count *= (size_t)shape[i]; }
  if (!ok) {
    std::string w = "(";
    for (size_t i = 0; i < want.size(); ++i) w += (i ? "," : "") + std::to_string(want[i]);
    return fail(h, GC_ERR_INVALID_ARGUMENT, "shape mismatch for " + n + ", expected " + w + ")");
  }
  h->weights[n].assign(data, data + count);
  h->finalized = false;
  h->finalized_weights = false;
  h->embed_cache_ready = false;
  return GC_OK;
  });
}

int gc_missing_weights(gc_handle* h, int32_t* count) {
  return guarded(h, [&]() -> int {
  if (!h || !count) return GC_ERR_INVALID_ARGUMENT;
  int miss = 0;
  for (const auto& kv : h->specs)
    if (!h->weights.count(kv.first)) ++miss;
  *count = miss;
  return GC_OK;
  });
}

int gc_finalize(gc_handle* h) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!h->has_graph) return fail(h, GC_ERR_STATE, "gc_set_graph must be called before gc_finalize");
  for (const auto& kv : h->specs)
    if (!h->weights.count(kv.first)) return fail(h, GC_ERR_STATE, "missing parameter: " + kv.first);
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  drop_sample_graphs(h);                        // the weight images are re-made: captured samples bake their addresses
  free_weights(h);
  return finalize_weights(h);
  });
}

int gc_denoise(gc_handle* h, const float* grid_feats, const float* sigma, float* out) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!grid_feats || !sigma || !out) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  const gc_config& c = h->cfg;
  for (int b = 0; b < c.batch; ++b)
    if (!(sigma[b] > 0.f)) return fail(h, GC_ERR_INVALID_ARGUMENT, "noise levels must be > 0");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t GB = (size_t)h->hg.G * c.batch;
  GC_HIP(h, hipMemcpyAsync(h->d_feats, grid_feats, GB * c.c_in * sizeof(float), hipMemcpyHostToDevice, h->stream));
  GC_HIP(h, hipMemcpyAsync(h->d_sigma, sigma, c.batch * sizeof(float), hipMemcpyHostToDevice, h->stream));
  if ((rc = launch(h, gc::KC_PACK, [&] {
         return gc::launch_pack_full(h->stream, h->d_grid_struct, h->d_feats, h->hg.G, c.batch, c.c_in,
                                     h->kp, h->d_xp);
       })))
    return rc;
  h->has_cond = false;  // d_xp no longer holds the sampler's conditioning
  if ((rc = forward(h, -1.0f))) return rc;
  if ((rc = guard_enqueue(h, h->d_y, GB * c.c_out))) return rc;
  GC_HIP(h, hipMemcpyAsync(out, h->d_y, GB * c.c_out * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  if (h->last_route.f16 && guard_tripped(h)) {      // left the f16x3 domain: the same call on the exact-f32 kernels
    ++h->range_fallbacks;
    h->in_fallback = true;
    rc = forward(h, -1.0f);
    h->in_fallback = false;
    if (rc) return rc;
    GC_HIP(h, hipMemcpyAsync(out, h->d_y, GB * c.c_out * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    GC_HIP(h, hipStreamSynchronize(h->stream));
  }
  return GC_OK;
  });
}

int gc_set_noisy_slots(gc_handle* h, const int32_t* slots) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!h->has_graph) return fail(h, GC_ERR_STATE, "gc_set_graph must be called first");
  if (!slots) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  const gc_config& c = h->cfg;
  int rc;
  std::vector<char> seen(c.c_in, 0);
  for (int i = 0; i < c.c_out; ++i) {
    if (slots[i] < 0 || slots[i] >= c.c_in || seen[slots[i]])
      return fail(h, GC_ERR_INVALID_ARGUMENT, "noisy slots must be distinct columns of grid_feats");
    seen[slots[i]] = 1;
  }
  // the callers' samplers set the slots before every sample (gencast-flax-nnx_amd/sampler.py): the same slots again change
  // nothing -- no copy, and above all no rebuild of the split embedding images, which would drop the captured sample graphs
  if (h->has_slots && (int)h->h_slots.size() == c.c_out && std::equal(slots, slots + c.c_out, h->h_slots.begin()) &&
      (h->embed_cache_ready || !(h->embed_cache && h->finalized_weights && h->hidden_layers == 1)))
    return GC_OK;
  GC_HIP(h, hipSetDevice(h->device));
  if (h->guard_pending && (rc = resolve_guard(h))) return rc;   // a pending re-run must still see the old slots
  // on the handle's stream (it is non-blocking: a null-stream copy would not be ordered against a
  // sampler still running), then waited for, so `slots` is free on return
  GC_HIP(h, hipMemcpyAsync(h->d_slots, slots, c.c_out * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  h->has_slots = true;
  h->h_slots.assign(slots, slots + c.c_out);
  return build_embed_cache(h);                  // (no-op until gc_finalize has laid the weights out)
  });
}

int gc_commit_cond(gc_handle* h) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  const gc_config& c = h->cfg;
  GC_HIP(h, hipSetDevice(h->device));
  if (h->guard_pending && (rc = resolve_guard(h))) return rc;
  if ((rc = launch(h, gc::KC_PACK, [&] {
         return gc::launch_pack_full(h->stream, h->d_grid_struct, h->d_feats, h->hg.G, c.batch, c.c_in,
                                     h->kp, h->d_xp);
       })))
    return rc;
  h->has_cond = true;
  return GC_OK;
  });
}

int gc_upload_cond(gc_handle* h, const float* cond_feats) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!cond_feats) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  GC_HIP(h, hipSetDevice(h->device));
  if (h->guard_pending && (rc = resolve_guard(h))) return rc;   // a pending re-run needs the conditioning it sampled with
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_in;
  if ((rc = staged_upload(h, h->pin_cond, h->d_feats, cond_feats, n))) return rc;
  return gc_commit_cond(h);
  });
}

int gc_upload_cond_dev(gc_handle* h, const void* cond_feats_dev) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!cond_feats_dev) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  GC_HIP(h, hipSetDevice(h->device));
  if (h->guard_pending && (rc = resolve_guard(h))) return rc;
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_in;
  GC_HIP(h, hipMemcpyAsync(h->d_feats, cond_feats_dev, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  return gc_commit_cond(h);
  });
}

int gc_cond_device_ptr(gc_handle* h, void** ptr, int64_t* nbytes) {
  return guarded(h, [&]() -> int {
  if (!h || !ptr || !nbytes) return GC_ERR_INVALID_ARGUMENT;
  if (!h->has_graph) return fail(h, GC_ERR_STATE, "gc_set_graph must be called first");
  *ptr = h->d_feats;
  *nbytes = (int64_t)h->hg.G * h->cfg.batch * h->cfg.c_in * (int64_t)sizeof(float);
  return GC_OK;
  });
}

int gc_upload_noise(gc_handle* h, const float* init_noise) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!init_noise) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_out;
  protect_pending_noise(h);
  if ((rc = staged_upload(h, h->pin_noise, h->d_noise, init_noise, n))) return rc;
  h->has_noise = true;
  return GC_OK;
  });
}

int gc_sample_resident(gc_handle* h, const float* sigmas, int32_t n, int32_t skip_dead_call,
                       gc_sample_stats* stats) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!sigmas || n < 1) return fail(h, GC_ERR_INVALID_ARGUMENT, "need at least one noise level");
  if (!h->has_slots) return fail(h, GC_ERR_STATE, "gc_set_noisy_slots has not been called");
  if (!h->has_cond) return fail(h, GC_ERR_STATE, "no conditioning uploaded (gc_upload_cond)");
  if (!h->has_noise) return fail(h, GC_ERR_STATE, "no initial noise uploaded (gc_upload_noise)");
  for (int i = 0; i < n; ++i)
    if (!(sigmas[i] > 0.f) || !(sigmas[i + 1] >= 0.f) || !(sigmas[i + 1] < sigmas[i]))
      return fail(h, GC_ERR_INVALID_ARGUMENT, "sigmas must be positive and strictly descending (a trailing 0 is allowed)");
  GC_HIP(h, hipSetDevice(h->device));
  return run_sampler(h, sigmas, n, skip_dead_call, stats);
  });
}

int gc_download_sample(gc_handle* h, float* out) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!out) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_out;
  if ((rc = resolve_guard(h))) return rc;
  GC_HIP(h, hipMemcpyAsync(out, h->d_sx, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
  });
}

int gc_stash_sample(gc_handle* h) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!h->has_sample) return fail(h, GC_ERR_STATE, "no sample on the device (gc_sample_resident)");
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = resolve_guard(h))) return rc;        // the snapshot is of the CHECKED sample (exact-f32 re-run included)
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_out;
  if (!h->d_stash && (rc = dev_alloc(h, &h->d_stash, n))) return rc;
  if (!h->ev_stash) GC_HIP(h, hipEventCreateWithFlags(&h->ev_stash, hipEventDisableTiming));
  if (h->has_stash) GC_HIP(h, hipStreamSynchronize(h->stream2));   // an earlier snapshot's download has left the buffer
  GC_HIP(h, hipMemcpyAsync(h->d_stash, h->d_sx, n * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  GC_HIP(h, hipEventRecord(h->ev_stash, h->stream));
  h->has_stash = true;
  return GC_OK;
  });
}

int gc_download_stash(gc_handle* h, float* out) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!out) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->has_stash) return fail(h, GC_ERR_STATE, "no snapshot on the device (gc_stash_sample)");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_out;
  // on the side stream, behind the snapshot copy only: whatever the main stream has been given since (the context
  // update, the next sample) keeps running while the host copy is in flight
  GC_HIP(h, hipStreamWaitEvent(h->stream2, h->ev_stash, 0));
  GC_HIP(h, hipMemcpyAsync(out, h->d_stash, n * sizeof(float), hipMemcpyDeviceToHost, h->stream2));
  GC_HIP(h, hipStreamSynchronize(h->stream2));
  return GC_OK;
  });
}

int gc_rollout_plan(gc_handle* h, const int32_t* kind, const int32_t* src, const int32_t* sidx, const float* a,
                    const float* b, int32_t n_forcing) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!kind || !src || !sidx || !a || !b || n_forcing < 0) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  const gc_config& c = h->cfg;
  for (int i = 0; i < c.c_in; ++i) {
    const int k = kind[i];
    if (k < 0 || k > 4) return fail(h, GC_ERR_INVALID_ARGUMENT, "rollout plan: kind must be 0..4");
    if ((k == 1 || k == 2) && (src[i] < 0 || src[i] >= c.c_in))
      return fail(h, GC_ERR_INVALID_ARGUMENT, "rollout plan: src out of range");
    if ((k == 2 || k == 4) && (sidx[i] < 0 || sidx[i] >= c.c_out))
      return fail(h, GC_ERR_INVALID_ARGUMENT, "rollout plan: sample index out of range");
    if (k == 3 && (sidx[i] < 0 || sidx[i] >= n_forcing))
      return fail(h, GC_ERR_INVALID_ARGUMENT, "rollout plan: forcing index out of range");
  }
  GC_HIP(h, hipSetDevice(h->device));
  const size_t GB = (size_t)h->hg.G * c.batch;
  auto upi = [&](int** d, const int32_t* p) -> int {
    int r;
    if (!*d && (r = dev_alloc(h, d, (size_t)c.c_in))) return r;
    GC_HIP(h, hipMemcpyAsync(*d, p, c.c_in * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return GC_OK;
  };
  auto upf = [&](float** d, const float* p) -> int {
    int r;
    if (!*d && (r = dev_alloc(h, d, (size_t)c.c_in))) return r;
    GC_HIP(h, hipMemcpyAsync(*d, p, c.c_in * sizeof(float), hipMemcpyHostToDevice, h->stream));
    return GC_OK;
  };
  if ((rc = upi(&h->d_ro_kind, kind)) || (rc = upi(&h->d_ro_src, src)) || (rc = upi(&h->d_ro_sidx, sidx)) ||
      (rc = upf(&h->d_ro_a, a)) || (rc = upf(&h->d_ro_b, b)))
    return rc;
  GC_HIP(h, hipStreamSynchronize(h->stream));   // the plan arrays are the caller's again
  if (!h->d_feats2 && (rc = dev_alloc(h, &h->d_feats2, GB * c.c_in))) return rc;
  if (n_forcing > h->ro_forc_cap) {            // (an earlier, smaller buffer stays owned by the handle)
    if ((rc = dev_alloc(h, &h->d_ro_forc, GB * n_forcing))) return rc;
    GC_HIP(h, hipEventSynchronize(h->ev_pin));
    if (h->pin_forc) GC_HIP(h, hipHostFree(h->pin_forc));
    h->pin_forc = nullptr;
    GC_HIP(h, pinned_alloc(h, &h->pin_forc, GB * n_forcing));
    h->ro_forc_cap = n_forcing;
  }
  h->ro_nforc = n_forcing;
  return GC_OK;
  });
}

int gc_rollout_advance(gc_handle* h, const float* forcings) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (h->ro_nforc < 0) return fail(h, GC_ERR_STATE, "gc_rollout_plan has not been called");
  if (!h->has_cond) return fail(h, GC_ERR_STATE, "no conditioning uploaded (gc_upload_cond)");
  if (!h->has_sample) return fail(h, GC_ERR_STATE, "no sample on the device (gc_sample_resident)");
  if (h->ro_nforc > 0 && !forcings) return fail(h, GC_ERR_INVALID_ARGUMENT, "the plan needs a forcings array");
  const gc_config& c = h->cfg;
  const size_t GB = (size_t)h->hg.G * c.batch;
  GC_HIP(h, hipSetDevice(h->device));
  if (h->guard_pending && (rc = resolve_guard(h))) return rc;   // the plan reads the sample
  if (h->ro_nforc > 0 && (rc = staged_upload(h, h->pin_forc, h->d_ro_forc, forcings, GB * h->ro_nforc))) return rc;
  if ((rc = launch(h, gc::KC_PACK, [&] {
         return gc::launch_rollout_advance(h->stream, h->d_feats, h->d_sx, h->d_ro_forc, h->d_ro_kind, h->d_ro_src,
                                           h->d_ro_sidx, h->d_ro_a, h->d_ro_b, (int)GB, c.c_in, c.c_out,
                                           h->ro_nforc, h->d_feats2);
       })))
    return rc;
  std::swap(h->d_feats, h->d_feats2);
  return gc_commit_cond(h);
  });
}

int gc_download_cond(gc_handle* h, float* out) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!out) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->has_cond) return fail(h, GC_ERR_STATE, "no conditioning uploaded (gc_upload_cond)");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_in;
  GC_HIP(h, hipMemcpyAsync(out, h->d_feats, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
  });
}

int gc_sync(gc_handle* h) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  GC_HIP(h, hipSetDevice(h->device));
  return resolve_guard(h);
  });
}

int gc_sample(gc_handle* h, const float* cond_feats, const float* init_noise, const float* sigmas,
              int32_t n, int32_t skip_dead_call, float* out, gc_sample_stats* stats) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!cond_feats || !init_noise || !out) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = gc_upload_cond(h, cond_feats))) return rc;
  if ((rc = gc_upload_noise(h, init_noise))) return rc;
  if ((rc = gc_sample_resident(h, sigmas, n, skip_dead_call, stats))) return rc;
  return gc_download_sample(h, out);
  });
}

int gc_num_kernel_classes(void) { return gc::KC_COUNT; }
const char* gc_kernel_class_name(int cls) { return gc::kernel_class_name(cls); }

int gc_profile_enable(gc_handle* h, int cls) {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (cls >= gc::KC_COUNT) return fail(h, GC_ERR_INVALID_ARGUMENT, "unknown kernel class");
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  if (cls >= 0 && h->prof_events.empty()) {
    h->prof_events.resize(2 * 4096);
    for (auto& e : h->prof_events) GC_HIP(h, hipEventCreate(&e));
  }
  h->prof_cls = cls;
  h->prof_used = 0;
  return GC_OK;
}

int gc_profile_set_stride(gc_handle* h, int stride) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (stride < 1) return fail(h, GC_ERR_INVALID_ARGUMENT, "stride must be >= 1");
  h->prof_stride = stride;
  h->prof_seen = 0;
  return GC_OK;
  });
}

int gc_profile_read(gc_handle* h, int32_t* launches, float* total_ms) {
  return guarded(h, [&]() -> int {
  if (!h || !launches || !total_ms) return GC_ERR_INVALID_ARGUMENT;
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  float tot = 0.f;
  for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
    float ms = 0.f;
    GC_HIP(h, hipEventElapsedTime(&ms, h->prof_events[i], h->prof_events[i + 1]));
    tot += ms;
  }
  *launches = (int32_t)(h->prof_used / 2);
  *total_ms = tot;
  h->prof_used = 0;
  return GC_OK;
  });
}

int gc_algorithmic_work(gc_handle* h, double* flops, double* bytes) {
  return guarded(h, [&]() -> int {
  if (!h || !flops || !bytes) return GC_ERR_INVALID_ARGUMENT;
  if (!h->has_graph) return fail(h, GC_ERR_STATE, "gc_set_graph must be called first");
  const gc_config& c = h->cfg;
  const double B = c.batch, G = h->hg.G * B, M = h->hg.M * B, E1 = h->hg.E1 * B, E2 = h->hg.E2 * B;
  const double L = c.latent_size, D = c.d_model, F = c.ffw_hidden, NL = c.num_layers;
  const double nnz = (double)h->hg.khop_nnz * B;
  double f = 0;
  f += 2 * G * (3 + c.c_in) * L + 2 * G * L * L;   // grid embed
  f += 2 * E1 * 3 * L * L + 2 * E1 * L * L;        // g2m edge update
  f += 2 * M * 2 * L * L + 2 * M * L * L;          // g2m mesh update
  f += 2 * G * L * L * 2;                          // g2m grid update
  f += NL * (2 * M * D * 3 * D + 2 * M * D * D + 2 * M * D * F * 2 + 4 * nnz * D);
  f += 2 * E2 * 3 * L * L + 2 * E2 * L * L;        // m2g edge update
  f += 2 * G * 2 * L * L + 2 * G * L * L;          // m2g grid update
  f += 2 * G * L * L + 2 * G * L * c.c_out;        // decoder
  // hidden_layers >= 2: one more L x L Linear per extra hidden layer in each of the 10 MLPs (the three edge / mesh
  // embedders run once per set-up, not per call: not counted, as above)
  f += (h->hidden_layers - 1) * 2.0 * L * L * (G + E1 + M + G + E2 + G + G);
  double params = 0;
  for (const auto& kv : h->specs) {
    double n = 1;
    for (auto d : kv.second) n *= (double)d;
    params += n;
  }
  // weights once + input + output + grid latent w/r + per layer {x r/w x2, QKV w+r}
  *bytes = 4.0 * (params + G * (c.c_in + c.c_out) + 2 * G * L + NL * M * D * 10);
  *flops = f;
  return GC_OK;
  });
}

int gc_get_counter(gc_handle* h, const char* name, int64_t* value) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!name || !value) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  const std::string n(name);
  if (n == "range_fallbacks") *value = h->range_fallbacks;
  else if (n == "static_embedding_fallbacks") *value = h->static_embedding_fallbacks;
  else if (n == "launches_per_call") *value = h->launches_last_call;
  else if (n == "weights_f16_unsafe") *value = h->weights_f16_unsafe ? 1 : 0;
  else if (n == "fp16_storage") *value = h->last_route.st16 ? 1 : 0;
  else if (n == "split_edge") *value = h->split_edge ? 1 : 0;
  else if (n == "attention_items") *value = h->last_route.att_items;
  else if (n == "m2g_fused_sum") *value = h->last_route.m2g_fused ? 1 : 0;
  else if (n == "embed_cache") *value = h->embed_cache_samples;
  else if (n == "edge_term_samples") *value = h->edge_term_samples;
  else if (n == "edge_term_cache_bytes") *value = h->terms.ready ? h->terms.bytes : 0;
  else if (n == "graph_replays") *value = h->graph_replays;
  else if (n == "graph_captures") *value = h->graph_captures;
  else if (n == "loss_evaluations") *value = h->loss_evaluations;
  else if (n == "loss_device_us") *value = h->loss_device_us;
  else if (const int64_t* v = meter_counter(h, n)) *value = *v;
  else if (n == "ens_window_pushes") *value = h->win_pushes;
  else if (n == "ens_window_ring_bytes") {
    const size_t L = h->win_allocs.key[0], M = h->win_allocs.key[1];   // (0, 0): no ring
    *value = (int64_t)(L * (((M + 1) * h->hg.G * h->cfg.batch * h->cfg.c_out + 3) / 4 * 4) * sizeof(float));
  }
  else if (n == "ens_map_bytes") *value = h->map_set ? h->map_bytes : 0;
  else if (n == "poison_allocs") *value = h->poison_allocs;
  else if (n == "poison_bytes") *value = h->poison_bytes;
  else if (n == "noise_stream") *value = (int64_t)h->nz_stream;
  else if (n == "device_allocations") {
    *value = 0;
    for (const BufferGroup* g : h->groups) *value += (int64_t)g->ptrs.size();
  }
  else return fail(h, GC_ERR_INVALID_ARGUMENT, "unknown counter: " + n);
  return GC_OK;
  });
}

// ---- spherical white noise on the device + stochastic churn (include/gencast_hip.h) -----------------
int gc_noise_set_tables(gc_handle* h, int32_t n_lat, int32_t n_lon, int32_t lmax, const float* legendre,
                        const float* cos_table, const float* sin_table) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!h->has_graph) return fail(h, GC_ERR_STATE, "gc_set_graph must be called first");
  if (!legendre || !cos_table || !sin_table) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (n_lat < 2 || n_lon < 2 || lmax < 1 || (int64_t)n_lat * n_lon != h->hg.G)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "n_lat * n_lon must equal the number of grid nodes");
  const int N = h->cfg.batch * h->cfg.c_out;
  // (no size limit: the Legendre step walks the latitudes in blocks of 192, the Fourier step stages wavenumber chunks
  //  of 64 columns through a fixed 64 KB of LDS -- samplers_utils.py:250-346 has none either)
  GC_HIP(h, hipSetDevice(h->device));
  int rc;
  const size_t L = (size_t)lmax;
  if ((rc = dev_upload(h, &h->d_nz_leg, std::vector<float>(legendre, legendre + L * n_lat * L)))) return rc;
  if ((rc = dev_upload(h, &h->d_nz_cos, std::vector<float>(cos_table, cos_table + (size_t)n_lon * L)))) return rc;
  if ((rc = dev_upload(h, &h->d_nz_sin, std::vector<float>(sin_table, sin_table + (size_t)n_lon * L)))) return rc;
  if ((rc = dev_alloc(h, &h->d_nz_coef, 2 * L * L * N + 4))) return rc;
  if ((rc = dev_alloc(h, &h->d_nz_f, 2 * L * n_lat * N))) return rc;
  h->nz_L = lmax; h->nz_lat = n_lat; h->nz_lon = n_lon;
  return GC_OK;
  });
}

int gc_noise_seed(gc_handle* h, uint64_t seed, uint64_t stream) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (h->guard_pending) {                      // a pending re-run draws its churn noise from the old key
    GC_HIP(h, hipSetDevice(h->device));
    int rc = resolve_guard(h);
    if (rc) return rc;
  }
  h->nz_key = seed;
  h->nz_stream = stream;
  return GC_OK;
  });
}

int gc_noise_draw(gc_handle* h) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  protect_pending_noise(h);
  if ((rc = noise_field(h, nullptr, 1.0f, h->d_noise))) return rc;
  h->has_noise = true;
  return GC_OK;
  });
}

int gc_download_noise(gc_handle* h, float* out) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!out) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->has_noise) return fail(h, GC_ERR_STATE, "no initial noise on the device");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_out;
  GC_HIP(h, hipMemcpyAsync(out, h->d_noise, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
  });
}

int gc_set_churn(gc_handle* h, const float* rates, int32_t n, float noise_level_inflation_factor) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (n < 0 || (n > 0 && !rates)) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  bool any = false;
  for (int i = 0; i < n; ++i) {
    if (!(rates[i] >= 0.f)) return fail(h, GC_ERR_INVALID_ARGUMENT, "churn rates must be >= 0");
    any = any || rates[i] > 0.f;
  }
  if (any && h->nz_L == 0) return fail(h, GC_ERR_STATE, "stochastic churn needs the noise tables (gc_noise_set_tables)");
  if (h->guard_pending) {                      // a pending re-run repeats the schedule it sampled with
    GC_HIP(h, hipSetDevice(h->device));
    int rc = resolve_guard(h);
    if (rc) return rc;
  }
  if (any) h->churn_rates.assign(rates, rates + n);
  else h->churn_rates.clear();
  h->churn_inflation = noise_level_inflation_factor;
  return GC_OK;
  });
}

// ---- denoising loss (include/gencast_hip.h) -----------------------------------------------------------
int gc_loss_set_weights(gc_handle* h, const float* node_weight, const float* channel_weight, const int32_t* channel_group,
                        int32_t n_groups, const float* group_weight) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!node_weight || !channel_weight || !channel_group || !group_weight) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (n_groups < 1 || n_groups > gc::kLossMaxGroups) return fail(h, GC_ERR_INVALID_ARGUMENT, "n_groups must be in 1..64");
  if (!h->has_graph) return fail(h, GC_ERR_STATE, "gc_set_graph must be called first");
  const gc_config& c = h->cfg;
  for (int i = 0; i < c.c_out; ++i)
    if (channel_group[i] < 0 || channel_group[i] >= n_groups)
      return fail(h, GC_ERR_INVALID_ARGUMENT, "channel_group holds an index outside [0, n_groups)");
  if ((size_t)(c.batch * c.c_out + c.batch * gc::kLossMaxGroups) * sizeof(double) > gc::kLossMaxLds)
    return fail(h, GC_ERR_UNSUPPORTED, "batch x c_out too large for the loss reduction's finishing kernel");
  GC_HIP(h, hipSetDevice(h->device));
  int rc;
  const int G = h->hg.G;
  if (!h->d_lw_node) {
    if ((rc = dev_alloc(h, &h->d_lw_node, (size_t)G)) || (rc = dev_alloc(h, &h->d_lw_chan, (size_t)c.c_out)) ||
        (rc = dev_alloc(h, &h->d_l_group, (size_t)c.c_out)) || (rc = dev_alloc(h, &h->d_lw_group, (size_t)gc::kLossMaxGroups)) ||
        (rc = dev_alloc(h, &h->d_lpart, (size_t)gc::loss_reduce_blocks(G, c.batch, c.c_out) * c.batch * c.c_out)))
      return rc;
  }
  // on the handle's stream (ordered behind whatever still runs there), then waited for: the arrays are the caller's again
  GC_HIP(h, hipMemcpyAsync(h->d_lw_node, node_weight, (size_t)G * sizeof(float), hipMemcpyHostToDevice, h->stream));
  GC_HIP(h, hipMemcpyAsync(h->d_lw_chan, channel_weight, c.c_out * sizeof(float), hipMemcpyHostToDevice, h->stream));
  GC_HIP(h, hipMemcpyAsync(h->d_l_group, channel_group, c.c_out * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  GC_HIP(h, hipMemcpyAsync(h->d_lw_group, group_weight, n_groups * sizeof(float), hipMemcpyHostToDevice, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  h->loss_groups = n_groups;
  h->has_loss_weights = true;
  return GC_OK;
  });
}

int gc_upload_targets(gc_handle* h, const float* targets) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!targets) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  GC_HIP(h, hipSetDevice(h->device));
  if (h->guard_pending && (rc = resolve_guard(h))) return rc;
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_out;
  if (!h->d_targets) {
    if ((rc = dev_alloc(h, &h->d_targets, n)) || (rc = dev_alloc(h, &h->d_lx, n)) || (rc = dev_alloc(h, &h->d_lden, n))) return rc;
  }
  if ((rc = staged_upload(h, h->pin_noise, h->d_targets, targets, n))) return rc;   // (same size as the noise staging buffer)
  h->has_targets = true;
  h->has_denoised = false;
  return GC_OK;
  });
}

int gc_loss_resident(gc_handle* h, const float* sigmas, int32_t n_eval, int32_t draw_noise, float* loss, float* per_group) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!sigmas || !loss || !per_group) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (n_eval < 1 || n_eval > (1 << 20)) return fail(h, GC_ERR_INVALID_ARGUMENT, "n_eval must be in 1..2^20");
  const gc_config& c = h->cfg;
  const int B = c.batch;
  for (int64_t i = 0; i < (int64_t)n_eval * B; ++i)
    if (!(sigmas[i] > 0.f)) return fail(h, GC_ERR_INVALID_ARGUMENT, "noise levels must be > 0");
  if (!h->has_slots) return fail(h, GC_ERR_STATE, "gc_set_noisy_slots has not been called");
  if (!h->has_loss_weights) return fail(h, GC_ERR_STATE, "no loss weights (gc_loss_set_weights)");
  if (!h->has_targets) return fail(h, GC_ERR_STATE, "no targets uploaded (gc_upload_targets)");
  if (!h->has_cond) return fail(h, GC_ERR_STATE, "no conditioning uploaded (gc_upload_cond)");
  if (draw_noise && h->nz_L == 0) return fail(h, GC_ERR_STATE, "gc_noise_set_tables has not been called");
  if (!draw_noise && !h->has_noise) return fail(h, GC_ERR_STATE, "no noise on the device (gc_upload_noise / gc_noise_draw)");
  GC_HIP(h, hipSetDevice(h->device));
  // a resident sample whose domain check is pending is resolved first: the evaluations share its guard counter, and a
  // re-run of that sample must still find its noise (draw_noise overwrites the initial-noise buffer, like gc_noise_draw)
  if ((rc = resolve_guard(h))) return rc;
  const int ng = h->loss_groups;
  if (n_eval > h->loss_cap) {                    // (earlier, smaller buffers stay owned by the handle)
    const int cap = std::max(n_eval, 2 * h->loss_cap);
    if ((rc = dev_alloc(h, &h->d_lsig, (size_t)cap * B)) || (rc = dev_alloc(h, &h->d_lloss, (size_t)cap * B)) ||
        (rc = dev_alloc(h, &h->d_lpg, (size_t)cap * B * gc::kLossMaxGroups)))
      return rc;
    unsigned* pin = nullptr;                     // the new block first: a failure leaves the old one and loss_cap = 0
    h->loss_cap = 0;
    GC_HIP(h, pinned_alloc(h, &pin, (size_t)cap));
    if (h->pin_lguard) (void)hipHostFree(h->pin_lguard);
    h->pin_lguard = pin;
    h->loss_cap = cap;
  }
  hipStream_t s = h->stream;
  GC_HIP(h, hipMemcpyAsync(h->d_lsig, sigmas, (size_t)n_eval * B * sizeof(float), hipMemcpyHostToDevice, s));
  const bool guard = make_route(h).f16;
  const unsigned long long stream0 = h->nz_stream;
  GC_HIP(h, hipEventRecord(h->ev0, s));
  for (int e = 0; e < n_eval; ++e) {
    if ((rc = loss_eval(h, e, h->d_lsig + (size_t)e * B, draw_noise != 0, e == n_eval - 1))) return rc;
    if (guard) {                                 // NaN / Inf in F: counted on the device, the count kept per evaluation
      if ((rc = launch(h, gc::KC_PACK, [&] {
             return gc::launch_finite_check(s, h->d_y, (size_t)h->hg.G * B * c.c_out, h->d_nonfinite);
           })))
        return rc;
      GC_HIP(h, hipMemcpyAsync(h->pin_lguard + e, h->d_nonfinite, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    }
  }
  GC_HIP(h, hipEventRecord(h->ev1, s));
  GC_HIP(h, hipStreamSynchronize(s));
  {
    float ms = 0.f;
    GC_HIP(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->loss_device_us = (int64_t)(ms * 1000.0f);
  }
  h->loss_evaluations += n_eval;
  h->has_denoised = true;
  if (guard) {
    // An evaluation that left the f16x3 domain runs again on the exact-f32 kernels, from the same noise: the field in
    // the initial-noise buffer, or the same Philox stream drawn again (x = t + sigma n is then the same, bit for bit).
    unsigned seen = h->nonfinite_seen;
    int last_rerun = -1;
    for (int e = 0; e < n_eval; ++e) {
      const bool tripped = h->pin_lguard[e] != seen;
      seen = h->pin_lguard[e];
      if (!tripped) continue;
      ++h->range_fallbacks;
      h->in_fallback = true;
      h->nz_stream = stream0 + (unsigned long long)e;
      rc = loss_eval(h, e, h->d_lsig + (size_t)e * B, draw_noise != 0, e == n_eval - 1);
      h->in_fallback = false;
      if (rc) return rc;
      last_rerun = e;
    }
    if (draw_noise) {
      if (last_rerun >= 0 && last_rerun != n_eval - 1) {   // the buffer holds the LAST evaluation's field again
        h->nz_stream = stream0 + (unsigned long long)(n_eval - 1);
        if ((rc = noise_field(h, nullptr, 1.0f, h->d_noise))) return rc;
      }
      h->nz_stream = stream0 + (unsigned long long)n_eval;
    }
    h->nonfinite_seen = seen;
    *h->h_nonfinite = seen;
  }
  GC_HIP(h, hipMemcpyAsync(loss, h->d_lloss, (size_t)n_eval * B * sizeof(float), hipMemcpyDeviceToHost, s));
  GC_HIP(h, hipMemcpyAsync(per_group, h->d_lpg, (size_t)n_eval * B * ng * sizeof(float), hipMemcpyDeviceToHost, s));
  GC_HIP(h, hipStreamSynchronize(s));
  return GC_OK;
  });
}

int gc_download_denoised(gc_handle* h, float* out) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!out) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->has_denoised) return fail(h, GC_ERR_STATE, "no loss evaluation on the device (gc_loss_resident)");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_out;
  GC_HIP(h, hipMemcpyAsync(out, h->d_lden, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
  });
}

int gc_loss(gc_handle* h, const float* cond_feats, const float* targets, const float* noise, const float* sigma, float* loss,
            float* per_group, float* denoised) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!cond_feats || !targets || !noise || !sigma || !loss || !per_group) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if ((rc = gc_upload_cond(h, cond_feats))) return rc;
  if ((rc = gc_upload_targets(h, targets))) return rc;
  if ((rc = gc_upload_noise(h, noise))) return rc;
  if ((rc = gc_loss_resident(h, sigma, 1, 0, loss, per_group))) return rc;
  return denoised ? gc_download_denoised(h, denoised) : GC_OK;
  });
}

// ---- ensemble exchange over RCCL / xGMI (include/gencast_hip.h) -------------------------------------
int gc_comm_unique_id(void* id_out) {
  return guarded(nullptr, [&]() -> int {
  if (!id_out) { g_create_error = "null argument"; return GC_ERR_INVALID_ARGUMENT; }
  Rccl& r = rccl();
  if (!r.error.empty()) { g_create_error = r.error; return GC_ERR_COMM; }
  ncclUniqueId id;
  const ncclResult_t rc = r.GetUniqueId(&id);
  if (rc != ncclSuccess) { g_create_error = std::string("ncclGetUniqueId: ") + r.GetErrorString(rc); return GC_ERR_COMM; }
  static_assert(sizeof(id) == GC_COMM_ID_BYTES, "ncclUniqueId size");
  std::memcpy(id_out, &id, sizeof(id));
  return GC_OK;
  });
}

int gc_comm_init(gc_handle* h, const void* id, int32_t rank, int32_t world_size) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!id || world_size < 1 || rank < 0 || rank >= world_size) return fail(h, GC_ERR_INVALID_ARGUMENT, "bad rank / world size");
  if (h->comm) return fail(h, GC_ERR_STATE, "communicator already initialised on this handle");
  Rccl& r = rccl();
  if (!r.error.empty()) return fail(h, GC_ERR_COMM, r.error);
  GC_HIP(h, hipSetDevice(h->device));
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  ncclComm_t comm = nullptr;                 // assigned to the handle only once it is valid
  GC_NCCL(h, r.CommInitRank(&comm, world_size, uid, rank));
  h->comm = comm;
  h->comm_rank = rank;
  h->comm_world = world_size;
  if (!h->d_comm_scalar) {
    int rc = dev_alloc(h, &h->d_comm_scalar, 1);
    if (rc) return rc;
  }
  return GC_OK;
  });
}

int gc_comm_info(gc_handle* h, int32_t* num_ranks, int32_t* rank) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!num_ranks || !rank) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  *num_ranks = 0;
  *rank = -1;
  if (!h->comm) return GC_OK;                  // no communicator: 0 ranks
  int n = 0, r = -1;
  GC_NCCL(h, rccl().CommCount(h->comm, &n));
  GC_NCCL(h, rccl().CommUserRank(h->comm, &r));
  *num_ranks = n;
  *rank = r;
  return GC_OK;
  });
}

int gc_comm_broadcast_cond(gc_handle* h, int32_t root) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!h->comm) return fail(h, GC_ERR_STATE, "gc_comm_init has not been called");
  if (root < 0 || root >= h->comm_world) return fail(h, GC_ERR_INVALID_ARGUMENT, "root out of range");
  GC_HIP(h, hipSetDevice(h->device));
  if (h->guard_pending && (rc = resolve_guard(h))) return rc;
  const size_t n = (size_t)h->hg.G * h->cfg.batch * h->cfg.c_in;
  // in place on the resident conditioning, ordered on the handle's stream behind any pending
  // upload (root) and in front of the re-pack below
  GC_NCCL(h, rccl().Broadcast(h->d_feats, h->d_feats, n, ncclFloat32, root, h->comm, h->stream));
  return gc_commit_cond(h);
  });
}

int gc_comm_allreduce_max(gc_handle* h, double* value) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!value) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->comm) return fail(h, GC_ERR_STATE, "gc_comm_init has not been called");
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, hipMemcpyAsync(h->d_comm_scalar, value, sizeof(double), hipMemcpyHostToDevice, h->stream));
  GC_NCCL(h, rccl().AllReduce(h->d_comm_scalar, h->d_comm_scalar, 1, ncclFloat64, ncclMax, h->comm, h->stream));
  GC_HIP(h, hipMemcpyAsync(value, h->d_comm_scalar, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
  });
}

int gc_comm_destroy(gc_handle* h) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!h->comm) return GC_OK;
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  GC_NCCL(h, rccl().CommDestroy(h->comm));
  h->comm = nullptr;
  h->comm_world = 1;
  h->comm_rank = 0;
  return GC_OK;
  });
}

// ---- debug: fetch an intermediate buffer of the last forward (include/gencast_hip_debug.h) ----
int gc_debug_fetch(gc_handle* h, const char* name, float* out, int64_t capacity, int64_t* rows,
                   int64_t* cols) {
  return guarded(h, [&]() -> int {
  int rc = check_ready(h);
  if (rc) return rc;
  if (!name || !rows || !cols) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  const gc_config& c = h->cfg;
  const gc::HostGraph& g = h->hg;
  const int64_t B = c.batch, L = c.latent_size;
  // act: an activation buffer -- a _Float16 array when the last forward ran with physical fp16 storage
  struct Ent { const char* n; const float* p; int64_t items; int64_t w; int mesh; int batched; int act; };
  const Ent table[] = {
      {"cond", h->d_condvec, 1, gc::kCondDim, 0, 1, 0},
      {"g0", h->d_g0, g.G, L, 0, 1, 1},        {"m0", h->m0_cur ? h->m0_cur : h->d_m0, g.M, L, 1, 1, 1},
      {"e1", h->d_e1, g.E1, L, 0, 1, 1},       {"agg1", h->d_agg1, g.M, L, 1, 1, 1},
      {"m1", h->d_x, g.M, L, 1, 1, 1},         {"x", h->d_x, g.M, L, 1, 1, 1},
      {"g1", h->d_g1, g.G, L, 0, 1, 1},        {"qkv", h->d_qkv, g.M, 3 * L, 1, 1, 0},
      {"att", h->d_att, g.M, L, 1, 1, 1},      {"m2", h->d_m2, g.M, L, 1, 1, 1},
      {"h", h->d_h, g.M, L, 1, 1, 1},
      {"f1", h->d_f1, g.E2, L, 0, 1, 1},       {"agg2", h->d_agg2, g.G, L, 0, 1, 1},
      {"g2", h->d_g2, g.G, L, 0, 1, 1},        {"y", h->d_y, g.G, c.c_out, 0, 1, 0},
      {"m0_hat", h->d_m0_hat, g.M, L, 1, 0, 0}, {"e0_hat", h->d_e0_hat, g.E1, L, 0, 0, 0},
      {"f0_hat", h->d_f0_hat, g.E2, L, 0, 0, 0},
  };
  if (!std::strncmp(name, "cond:", 5)) {
    // the [scale | offset] vectors one conditioning linear produced in the last gc_denoise ("+1" folded into the scale)
    auto it = h->cond_sites.find(name + 5);
    if (it == h->cond_sites.end()) return fail(h, GC_ERR_INVALID_ARGUMENT, std::string("unknown conditioning site: ") + (name + 5));
    const int off = it->second.first, w = it->second.second;
    *rows = B;
    *cols = 2 * w;
    if (!out) return GC_OK;
    if (capacity < *rows * *cols) return fail(h, GC_ERR_INVALID_ARGUMENT, "output buffer too small");
    GC_HIP(h, hipSetDevice(h->device));
    GC_HIP(h, hipStreamSynchronize(h->stream));
    for (int64_t b = 0; b < B; ++b)
      GC_HIP(h, hipMemcpy(out + b * 2 * w, h->d_cond + (size_t)b * h->cond_total + off, (size_t)2 * w * sizeof(float), hipMemcpyDeviceToHost));
    return GC_OK;
  }
  for (const Ent& e : table) {
    if (std::strcmp(e.n, name)) continue;
    const int64_t bb = e.batched ? B : 1;
    *rows = e.items * bb;
    *cols = e.w;
    if (!out) return GC_OK;
    if (capacity < *rows * *cols) return fail(h, GC_ERR_INVALID_ARGUMENT, "output buffer too small");
    GC_HIP(h, hipSetDevice(h->device));
    if (!std::strcmp(name, "f1") && h->last_route.m2g_fused) {
      // the last forward summed the updated edges inside the edge MLP and never stored them: run that MLP once more,
      // unfused, on the inputs the forward left behind (m2 / g1 or their per-node products, the call's conditioning)
      if (!h->cond_cur) return fail(h, GC_ERR_STATE, "no forward has run yet");
      if ((rc = run_m2g_edge(h, h->cond_cur, false))) return rc;
    }
    GC_HIP(h, hipStreamSynchronize(h->stream));
    std::vector<float> tmp((size_t)(*rows * *cols));
    if (e.act && h->last_route.st16) {                 // halfs in HBM: widen
      std::vector<uint16_t> hv(tmp.size());
      GC_HIP(h, hipMemcpy(hv.data(), e.p, hv.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
      for (size_t i = 0; i < hv.size(); ++i) tmp[i] = f16_bits_to_f32(hv[i]);
    } else {
      GC_HIP(h, hipMemcpy(tmp.data(), e.p, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (!std::strcmp(name, "qkv") && h->last_route.v2 && h->last_route.st16) {
      // physical fp16 storage: q is a _Float16 array [rows][D] at d_qkv; k, v are the hi planes of kv16 (lo unwritten)
      const size_t D = (size_t)c.d_model, nrows = (size_t)*rows;
      std::vector<uint16_t> q16(nrows * D), pl(nrows * 4 * D);
      GC_HIP(h, hipMemcpy(q16.data(), h->d_qkv, q16.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
      GC_HIP(h, hipMemcpy(pl.data(), h->d_kv16, pl.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
      for (size_t r0 = 0; r0 < nrows; ++r0)
        for (size_t d0 = 0; d0 < D; ++d0) {
          tmp[r0 * 3 * D + d0] = f16_bits_to_f32(q16[r0 * D + d0]);
          tmp[r0 * 3 * D + D + d0] = f16_bits_to_f32(pl[r0 * 4 * D + d0]);
          tmp[r0 * 3 * D + 2 * D + d0] = f16_bits_to_f32(pl[r0 * 4 * D + 2 * D + d0]);
        }
    } else if (!std::strcmp(name, "qkv") && h->last_route.v2) {
      // the projection wrote k and v as fp16 hi / lo planes only: value = hi + lo / 2048
      const size_t D = (size_t)c.d_model, nrows = (size_t)*rows;
      std::vector<uint16_t> pl(nrows * 4 * D);
      GC_HIP(h, hipMemcpy(pl.data(), h->d_kv16, pl.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
      for (size_t r0 = 0; r0 < nrows; ++r0)
        for (int w = 0; w < 2; ++w)
          for (size_t d0 = 0; d0 < D; ++d0)
            tmp[r0 * 3 * D + (w + 1) * D + d0] = f16_bits_to_f32(pl[r0 * 4 * D + w * 2 * D + d0]) +
                                                 f16_bits_to_f32(pl[r0 * 4 * D + w * 2 * D + D + d0]) / 2048.0f;
    }
    if (e.mesh) {  // back to the caller's mesh numbering
      for (int64_t ni = 0; ni < e.items; ++ni)
        std::memcpy(out + (size_t)g.perm[ni] * bb * e.w, tmp.data() + (size_t)ni * bb * e.w,
                    (size_t)(bb * e.w) * sizeof(float));
    } else if (!std::strcmp(name, "f1") || !std::strcmp(name, "f0_hat")) {  // back to the caller's mesh2grid edge order
      for (int64_t ei = 0; ei < e.items; ++ei)
        std::memcpy(out + (size_t)g.m2g_order[ei] * bb * e.w, tmp.data() + (size_t)ei * bb * e.w,
                    (size_t)(bb * e.w) * sizeof(float));
    } else {
      std::memcpy(out, tmp.data(), tmp.size() * sizeof(float));
    }
    return GC_OK;
  }
  return fail(h, GC_ERR_INVALID_ARGUMENT, std::string("unknown debug buffer: ") + name);
  });
}

#ifdef GC_STAMPS
// Diagnostic build only (csrc/build.sh stamps): per-wave stamps of the LAST attention launch.
int gc_debug_attention_stamps(gc_handle* h, unsigned long long* out, int64_t words) {
  if (!h || (!out && words >= 0)) return GC_ERR_INVALID_ARGUMENT;
  static unsigned long long* dbuf = nullptr;
  static int64_t cap = 0;
  if (words < 0) {                               // arm: allocate -words and install
    if (cap < -words) { (void)hipFree(dbuf); if (hipMalloc((void**)&dbuf, (size_t)(-words) * 8) != hipSuccess) return GC_ERR_HIP; cap = -words; }
    (void)hipMemset(dbuf, 0, (size_t)cap * 8);
    return gc::set_attention_stamp_buffer(dbuf) == hipSuccess ? GC_OK : GC_ERR_HIP;
  }
  (void)hipStreamSynchronize(h->stream);
  return hipMemcpy(out, dbuf, (size_t)std::min(words, cap) * 8, hipMemcpyDeviceToHost) == hipSuccess ? GC_OK : GC_ERR_HIP;
}
#endif

int gc_debug_set_layer_limit(gc_handle* h, int32_t num_layers) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  h->debug_layer_limit = num_layers;
  return GC_OK;
  });
}

int gc_debug_set_stop(gc_handle* h, int32_t layer, int32_t phase) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (layer >= 0 && (phase < 0 || phase > 2)) return fail(h, GC_ERR_INVALID_ARGUMENT, "phase must be 0, 1 or 2");
  h->debug_stop_layer = layer;
  h->debug_stop_phase = layer >= 0 ? phase : -1;
  return GC_OK;
  });
}

int gc_debug_mesh_permutation(gc_handle* h, int32_t* perm_out) {
  return guarded(h, [&]() -> int {
  if (!h || !perm_out) return GC_ERR_INVALID_ARGUMENT;
  if (!h->has_graph) return fail(h, GC_ERR_STATE, "gc_set_graph must be called first");
  for (int i = 0; i < h->hg.M; ++i) perm_out[i] = h->hg.perm[i];
  return GC_OK;
  });
}

int gc_debug_attention_stats(gc_handle* h, int64_t* n_tiles, int64_t* n_chunks, int64_t* khop_nnz) {
  return guarded(h, [&]() -> int {
  if (!h || !n_tiles || !n_chunks || !khop_nnz) return GC_ERR_INVALID_ARGUMENT;
  if (!h->has_graph) return fail(h, GC_ERR_STATE, "gc_set_graph must be called first");
  *n_tiles = h->hg.n_tiles;
  *n_chunks = h->hg.tile_chunk_start.back();
  *khop_nnz = h->hg.khop_nnz;
  return GC_OK;
  });
}

}  // extern "C"
