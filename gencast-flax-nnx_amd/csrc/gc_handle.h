// Internals shared by the host translation units of libgencast_hip.so: the handle, the device-side weight layout,
// the route of a forward, and the allocation / launch helpers.
//   gc_weights.hip   lays the weights out
//   gc_forward.hip   enqueues one denoiser forward
//   gc_sampler.hip   the sampler and the loss around it
//   gc_api.hip       the C ABI, but for the entries of the four units below
//   gc_ensemble.hip  gc_ens_* (the member store and its scores) and gc_ctx_*
//   gc_spectrum.hip  gc_spec_*, gc_ens_spectrum and gc_ens_band_*
//   gc_events.hip    gc_ens_event_*
//   gc_derive.hip    gc_ens_derive_*
//   gc_order.hip     gc_ens_order_*
//   gc_clim.hip      gc_ens_clim_score
//   gc_efi.hip       gc_ens_efi_*
//   gc_map.hip       gc_ens_map_*
//   gc_window.hip    gc_ens_window_*
//   gc_multivar.hip  gc_ens_energy_*, gc_ens_variogram_*
//   gc_tail.hip      gc_ens_tail_*
//   gc_region.hip    gc_ens_region_*
//   gc_feature.hip   gc_ens_feature_*
//   gc_fss.hip       gc_ens_fss_*
// The last fifteen are scorers over the member store of gc_ens_reserve (gc_window.hip fills one from a ring of the last
// lead times of another, gc_feature.hip with the strike fields of the centres it finds in another).  Their host side is two
// protocols, "score a store" and "fill a store from a source handle", written once in gc_store.h.  What a unit keeps on the
// handle is declared with the types below: its device buffers are a BufferGroup (a KeyedGroup where a call makes them
// again for other sizes), its events an Event, and the bookkeeping of its timed calls a Meter; declaring one as a member of
// the handle is all it takes for gc_destroy to release it and for gc_get_counter to see it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include <rccl/rccl.h>   // types and enums only: librccl.so.1 is dlopen'ed on first use (gc_comm_*)

#include "../../include/gencast_hip.h"
#include "../../include/gencast_hip_debug.h"
#include "gc_graph.h"
#include "gc_kernels.h"

namespace gci {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Every decision of one denoiser forward, taken once from the handle's state (make_route, gc_forward.hip); the
// launches read nothing else.
struct Route {
  bool f16 = false;         // GEMM-shaped kernels run f16x3 (3 fp16 MFMAs per product); else exact f32
  bool x32 = false;         // exact f32 on the weight-streaming / fused kernels (WF32 images, v_mfma_f32_32x32x2_f32)
  bool st16 = false;        // PHYSICAL fp16 activation storage: every kernel is the gc_a16 build (halfs in HBM)
  int ffw_slabs = 0;        // > 0: both FFW layers in one launch with this many hidden slices
  bool v2 = false;          // the QKV projection writes K / V as fp16 planes (they live in d_kv16 only) for attention v2
  int att_items = 0;        // work items of the attention launch (0: the plain (tile, split) launch)
  bool fuse_row = false;    // out-projection with the row pass in its epilogue
  bool node_ws = false;     // the per-node GEMMs of a split edge MLP stream their weights (WF16 only: no WF32 image)
  bool m2g_fused = false;   // the mesh2grid edge MLP sums each grid node's three edges: f1 is not stored
  bool split_edge = false;  // edge MLPs with the first layer split by input block
  bool try_pair = false;    // the grid2mesh edge and grid-node updates may go out as one launch
  bool embed_cache = false; // inside a sample that runs the grid embedding on the cache (d_xn / d_pstat)
  bool edge_terms = false;  // inside a sample whose noise levels have their edge terms cached (gc_handle::EdgeTerms): the
                            // two edge MLPs' first layer is T(sigma)[e] + P_snd[snd] + P_rcv[rcv] + b1, no product
  // the weight-streaming GEMM (WF16 / WF32 weights) whenever the K slice is a multiple of 128
  bool ws(int n, int k, int splits) const { return (f16 || x32) && n % 128 == 0 && (k / splits) % 128 == 0; }
};

// One matrix W^T [n][k] on the device, in every image a kernel form reads it from.
struct Weight {
  float* t = nullptr;   // float32, row-major, row stride ld   (LDS-staged kernels, exact f32)
  float* s = nullptr;   // S16 (split-fp16) encoding of t      (LDS-staged kernels, f16x3)
  float* f = nullptr;   // WF16 (MFMA fragment order), K = kf  (weight-streaming kernels, f16x3)
  float* x = nullptr;   // WF32, K = kf                        (weight-streaming kernels, exact f32; only with f32_ws)
  int ld = 0, kf = 0;   // kf: K of the streaming images, zero-padded to a multiple of 64
};
enum class Form { Staged, Streaming };
inline const float* pick(const Weight& w, const Route& r, Form form) {
  if (form == Form::Streaming) return r.x32 ? w.x : w.f;
  return r.f16 ? w.s : w.t;
}

struct DevMlp {        // device-side layout of one MLPWithNormConditioning
  Weight w1, w2;       // [hidden][K padded], [n_out_pad][hidden]
  // edge MLPs only: first layer split by input block [e | sender | receiver] (each L rows of W1; the per-node blocks
  // have no WF32 image).  w1e is also the noisy-columns block of the grid embedding (build_embed_cache: streaming
  // images only, ld = the compact array's row stride)
  Weight w1e, w1snd, w1rcv;
  float *b1 = nullptr, *b2 = nullptr;
  int n_out = 0, n_out_pad = 0;
  int cond_off = -1;   // offset of [scale | offset] in the conditioning buffer
  // hidden_layers >= 2 (common/mlp.py:166-183): the leading (Linear -> activation) layers, each run as a launch of
  // the same fused kernel with an identity second layer and no LayerNorm; this struct then holds the LAST hidden
  // Linear as its first layer and the output Linear as its second
  std::vector<DevMlp> pre;
};

struct DevLayer {      // one transformer block
  Weight wqkv, wo, w1, w2;   // [3D][D], [D][D], [F][D], [D][F]
  float *bo = nullptr, *b1 = nullptr, *b2 = nullptr;
  int cond_attn = -1, cond_ffw = -1;
};

// Device buffers that are freed and replaced together.  A member of the handle enters the handle's list: gc_destroy
// and the "device_allocations" counter walk that list.
struct BufferGroup {
  std::vector<void*> ptrs;
  explicit BufferGroup(std::vector<BufferGroup*>& of_handle) { of_handle.push_back(this); }
  BufferGroup(const BufferGroup&) = delete;
  void free() {                          // (the caller knows that nothing on the device uses the buffers any more)
    for (void* p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
  hipError_t drop(hipStream_t s) {       // synchronise the stream that used them, free, forget
    const hipError_t e = hipStreamSynchronize(s);
    if (e == hipSuccess) free();
    return e;
  }
};

// An event the handle owns: created on first use, destroyed by gc_destroy through the handle's list.
struct Event {
  hipEvent_t e = nullptr;
  explicit Event(std::vector<Event*>& of_handle) { of_handle.push_back(this); }
  Event(const Event&) = delete;
  hipError_t ensure(bool timing = false) {
    return e ? hipSuccess : timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming);
  }
};

// The two timing events around the device work of a feature's last call.
struct Bracket {
  Event e0, e1;
  explicit Bracket(std::vector<Event*>& of_handle) : e0(of_handle), e1(of_handle) {}
  hipError_t ensure() {
    const hipError_t e = e0.ensure(true);
    return e != hipSuccess ? e : e1.ensure(true);
  }
  hipError_t begin(hipStream_t s) {                // (the events are made by the first call)
    const hipError_t e = ensure();
    return e != hipSuccess ? e : hipEventRecord(e0.e, s);
  }
  hipError_t end(hipStream_t s) { return hipEventRecord(e1.e, s); }
  hipError_t microseconds(int64_t* us) {           // (after the stream has been synchronised)
    float ms = 0.f;
    const hipError_t e = hipEventElapsedTime(&ms, e0.e, e1.e);
    *us = (int64_t)(ms * 1000.0f);
    return e;
  }
};

// What a unit keeps of its timed calls (gci::timed, gc_store.h): the events of the last one, and the numbers
// gc_get_counter reports -- calls made, device time of the last, what the last skipped (points or columns; 0 in a
// unit that counts none), and the launch geometry of the last: `blocks` is grid.x of its main pass, the node-range
// workgroups (the regime a call ran in: below a unit's block cap every workgroup has nodes, above it `per` grows and the
// trailing ones may have none); `chunks` the column chunks it went through (gc_ens_fss_score alone; 0 elsewhere).  A
// call with two passes of different geometry reports the pass that has a cap of its own:
//   gc_ens_efi_score    the table pass (kEfiMaxWorkgroups / (T tiles)) where T > 0, else the index pass;
//   gc_ens_efi_fields   the index pass (loss_reduce_blocks), the only one it has;
//   gc_ens_order_score  the sorting pass (ord_blocks);   gc_ens_order_fields  its field pass (loss_reduce_blocks of one tile);
//   gc_ens_derive       the point pass (launch_ens_derive / launch_ens_derive_expr), not the pooling passes;
//   gc_ens_fss_score    the column pass (fss_blocks);
//   gc_ens_feature, gc_ens_band  their gather (grid-stride by gridDim.x * 256; one thread per gathered value): neither
//                       has a node-range pass or a cap that bites below 262 144 nodes.
struct Meter {
  Bracket time;
  int64_t calls = 0, device_us = 0, invalid = 0, blocks = 0, chunks = 0;
  explicit Meter(std::vector<Event*>& of_handle) : time(of_handle) {}
};

// A BufferGroup whose buffers are sized by N numbers: `key` is what they were made for, all zero where there are none (no
// unit has an all-zero key).  A call that finds `differs(its sizes)` makes them again (gci::sized_for below).  free and
// drop forget the key; gc_destroy frees through the BufferGroup, where no key matters any more.
template <size_t N>
struct KeyedGroup : BufferGroup {
  std::array<size_t, N> key{};
  using BufferGroup::BufferGroup;
  bool differs(const std::array<size_t, N>& k) const { return key != k; }
  void free() {
    key.fill(0);
    BufferGroup::free();
  }
  hipError_t drop(hipStream_t s) {
    key.fill(0);
    return BufferGroup::drop(s);
  }
};

}  // namespace gci

struct gc_handle {
  std::vector<gci::BufferGroup*> groups;     // every BufferGroup / Event member below, in declaration order
  std::vector<gci::Event*> events;
  gc_config cfg{};
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;             // side stream of the stash download (gc_stash_sample)
  std::string err;
  bool has_graph = false, finalized = false, has_slots = false, has_cond = false, has_noise = false;
  bool finalized_weights = false;            // gc_finalize ran on the weights now loaded (gc_load_weight clears it)
  gc::HostGraph hg;

  std::map<std::string, std::vector<int64_t>> specs;  // expected shapes
  std::map<std::string, std::vector<float>> weights;  // host copies as loaded
  // device buffers by owner (all freed in destroy): made once per handle; by gc_finalize, freed by the next one
  // (free_weights); by build_embed_cache, freed by the next one
  gci::BufferGroup allocs{groups}, weight_allocs{groups}, cache_allocs{groups};

  // graph (device)
  int *d_g2m_snd = nullptr, *d_g2m_rcv = nullptr, *d_m2g_snd = nullptr, *d_m2g_rcv = nullptr;
  int *d_g2m_ptr = nullptr, *d_g2m_eid = nullptr, *d_m2g_ptr = nullptr, *d_m2g_eid = nullptr;
  int *d_tile_start = nullptr, *d_union = nullptr;
  // work-item list of the attention launch (1.25 rounds of tiles -> one round of whole tiles + one round of pieces):
  // build_attention_items
  int *d_att_items = nullptr, *d_att_tiles = nullptr;
  int att_n_items = 0;
  unsigned* d_mask = nullptr;
  float *d_grid_struct = nullptr, *d_mesh_struct16 = nullptr, *d_e1_struct16 = nullptr,
        *d_e2_struct16 = nullptr;

  // weights (device)
  gci::DevMlp g2m_embed_grid, g2m_embed_mesh, g2m_embed_edge, g2m_edge, g2m_mesh, g2m_grid;
  gci::DevMlp m2g_embed_edge, m2g_edge, m2g_grid, m2g_dec;
  std::vector<gci::DevLayer> layers;
  int cond_final = -1;
  int cond_total = 0;
  std::map<std::string, std::pair<int, int>> cond_sites;   // conditioning linear (parameter path) -> (offset, width) in d_cond
  float *d_nw0t = nullptr, *d_nb0 = nullptr, *d_nw1t = nullptr, *d_nb1 = nullptr;
  float *d_wc_all = nullptr, *d_bc_all = nullptr;

  // static embeddings (LayerNorm output, before conditioning)
  float *d_m0_hat = nullptr, *d_e0_hat = nullptr, *d_f0_hat = nullptr;

  // activations
  int kp = 0;
  float *d_sigma = nullptr, *d_condvec = nullptr, *d_cond = nullptr;
  float* d_cond_all = nullptr;               // sampler: conditioning of every call of the sample [calls][B][total]
  size_t cond_all_cap = 0;
  const float* cond_cur = nullptr;           // conditioning vectors the current forward() reads
  float *d_feats = nullptr, *d_xp = nullptr, *d_g0 = nullptr, *d_g1 = nullptr, *d_m0 = nullptr,
        *d_x = nullptr, *d_e1 = nullptr, *d_agg1 = nullptr, *d_qkv = nullptr, *d_att = nullptr,
        *d_u = nullptr, *d_m2 = nullptr, *d_f1 = nullptr, *d_agg2 = nullptr, *d_g2 = nullptr,
        *d_y = nullptr, *d_h = nullptr, *d_part = nullptr, *d_apart_o = nullptr, *d_apart_ml = nullptr,
        *d_pg = nullptr, *d_pm = nullptr;     // per-node first-layer products of the edge MLPs
  // Grid embedding with its per-sample-constant part cached (dpm_solver_plus_plus_2s.py:107-112,
  // denoiser.py:654-659): inside one sample only the c_out noisy-target channels of the packed grid input change from
  // call to call.  At the start of a sample P = W1[static rows]^T [struct | inputs | forcings] is computed once
  // ([G B, L] float32, the noisy columns' weights zeroed); each call's embedding MLP then multiplies only the compact
  // noisy array xn [G B, c_out padded to 32] and adds P next to the bias (the add-term path of the split edge MLPs).
  bool mlp_pair = true;                      // GC_TUNE_MLP_PAIR=0: the grid2mesh edge update and the grid-node update as two launches
  bool embed_cache = true;                   // GC_TUNE_EMBED_CACHE=0: every call multiplies all 3 + c_in columns
  bool embed_cache_ready = false;            // the split weight images below match the current weights and slots
  bool embed_cache_live = false;             // inside a sample: the forwards may run on the cache (Route::embed_cache)
  int nwp = 0;                               // noisy columns padded to a multiple of 32
  float *d_xn = nullptr, *d_pstat = nullptr;
  float *w1st_t = nullptr, *w1st_s = nullptr;   // static first layer [L][kp]: float32 and S16, noisy columns zero
  gci::DevMlp g2m_embed_grid_n;                   // g2m_embed_grid with the noisy-columns block as its first layer (+ P as add term)
  std::vector<int> h_slots;
  int64_t embed_cache_samples = 0;           // samples that ran on the cache (gc_get_counter "embed_cache")
  bool m2g_fuse_sum = true;                  // GC_TUNE_M2G_FUSE_SUM=0: mesh2grid edge update + a segment-sum launch (the form every
                                             // graph with other in-degrees than 3 takes anyway)
  // Edge terms ("edge terms").  The first layer of an edge MLP is [e | n_snd | n_rcv] @ W1 =
  // e @ W1e + (n_snd @ W1snd)[snd] + (n_rcv @ W1rcv)[rcv].  Inside a sample e = affine(e_hat; cond(sigma)) depends on
  // the noise level alone (static embedding under a conditioning affine), and so do m0 = affine(m0_hat; sigma) and its
  // product with the grid2mesh receiver block.  A sampler runs ONE sigma list for every sample of every member, so
  // these are made once per list, one slot per distinct noise level:
  //   T1 [slots][E1][L] = affine(e0_hat) @ W1e(g2m)      T2 [slots][E2][L] = affine(f0_hat) @ W1e(m2g)
  //   m0 [slots][M][L]                                   Pm [slots][M][L]  = m0 @ W1rcv(g2m)
  // Call i of a sample reads slot call_slot[i].  Key: the sigma list of the calls; weights, precision, feature mode
  // and the static embeddings are covered by dropping the cache where they change (free_weights,
  // compute_static_embeddings).  Batch 1 only (the sampler's conditioning is the same for every batch element, but m0
  // is also a residual with a batch axis): batch > 1 keeps the route with the products.
  struct EdgeTerms {
    bool ready = false;                          // built for `sigmas`, within the cap
    std::vector<float> sigmas;                   // noise level of every denoiser call of the sample it was built for
    std::vector<int> call_slot;                  // call -> slot (equal noise levels share one)
    float *T1 = nullptr, *T2 = nullptr, *m0 = nullptr, *Pm = nullptr;
    int64_t bytes = 0;
  };
  bool edge_terms = true;                        // GC_TUNE_EDGE_TERMS=0: every call multiplies the whole first layer
  int64_t edge_term_cap_mb = 4096;               // gc_set_option("edge_term_cache_mb"): a list that needs more keeps the products
  EdgeTerms terms;
  gci::BufferGroup term_allocs{groups};
  int term_slot = -1;                            // slot of the forward being enqueued / of the last one (gc_debug_fetch)
  const float* m0_cur = nullptr;                 // the conditioned mesh embedding the last forward read (d_m0 or a slot)
  int64_t edge_term_samples = 0;                 // samples that ran on the cache (gc_get_counter)
  float *d_ones = nullptr, *d_zeros = nullptr;   // identity affine for gc_mlp_ws
  int hidden_layers = 1;                         // gc_set_option("hidden_layers"): hidden layers of every GNN MLP (denoiser.py:135)
  float* d_mlp_tmp[2] = {nullptr, nullptr};      // hidden_layers >= 2: [max rows][latent] hand-over between the launches of one MLP
  // autoregressive context update (gc_rollout_plan / gc_rollout_advance)
  float *d_feats2 = nullptr, *d_ro_a = nullptr, *d_ro_b = nullptr, *d_ro_forc = nullptr;
  int *d_ro_kind = nullptr, *d_ro_src = nullptr, *d_ro_sidx = nullptr;
  int ro_nforc = -1, ro_forc_cap = 0;
  bool has_sample = false;
  int max_tile_chunks = 0;                   // largest number of 32-key chunks of any attention tile
  int ffw_fused_slabs = 0;                   // > 0: gc_ffw_fused with this many hidden slices (= slabs)
  void* d_kv16 = nullptr;                    // K / V as fp16 hi / lo planes, written by the QKV projection
  bool f32_ws = true;                        // exact-f32 family on the weight-streaming / fused kernels (WF32 images): the shapes allow it
  bool split_edge = false;                   // the split edge MLPs (latent >= 512, hidden_layers == 1)
  // launch geometry (chosen in gc_set_graph)
  int attn_splits = 1, out_splits = 1, ffw2_splits = 1;
  gci::Route route;                          // of the launches being enqueued (forward, compute_static_embeddings)
  gci::Route last_route;                     // of the last forward (gc_debug_fetch, gc_get_counter)
  bool a16 = true;                           // GC_TUNE_A16=0: fp16-feature mode on float32 containers with 3 MFMAs per product (A/B, bit-identical)
  bool attn_items = true;                    // GC_TUNE_ATTN_ITEMS=0: the plain (tile, split) attention launch
  bool graph_serialize = false;              // GC_TUNE_GRAPH_SERIALIZE=1: every hipGraphLaunch also takes the capture mutex (run_sampler)
  bool graph_verbose = false;                // GC_TUNE_GRAPH_VERBOSE=1: graph capture progress on stderr
  bool poison = false;                       // GC_DEBUG_POISON=1: dev_alloc fills every new buffer (NaN / 0x01 bytes), the pinned staging buffers get 0xFF
  int64_t poison_allocs = 0, poison_bytes = 0;   // device buffers filled so far, and their bytes (gc_get_counter)
  // sampler state
  int* d_slots = nullptr;
  float *d_sx = nullptr, *d_sden = nullptr, *d_smid = nullptr, *d_noise = nullptr;
  // The initial noise is double-buffered: a resident sample whose f16x3 domain check is still pending may have to be
  // re-run from ITS noise, so an upload / draw for the next member that arrives before the check is resolved goes to
  // the other buffer (d_noise always = the buffer the next sample will read; last_noise = the pending sample's).
  float *d_noise_alt = nullptr, *last_noise = nullptr;
  float* d_stash = nullptr;            // gc_stash_sample: snapshot of a sample, downloaded on the side stream
  hipEvent_t ev_stash = nullptr;
  bool has_stash = false;

  // spherical white noise on the device + stochastic churn (gc_noise_*, gc_set_churn)
  int nz_L = 0, nz_lat = 0, nz_lon = 0;
  float *d_nz_leg = nullptr, *d_nz_cos = nullptr, *d_nz_sin = nullptr, *d_nz_coef = nullptr, *d_nz_f = nullptr;
  unsigned long long nz_key = 0, nz_stream = 0;
  std::vector<float> churn_rates;      // per solver step; empty = no churn
  float churn_inflation = 1.0f;

  // denoising loss (gc_loss_*): forward-only evaluation of the training objective on resident conditioning + targets
  bool has_loss_weights = false, has_targets = false, has_denoised = false;
  int loss_groups = 0;
  float *d_lw_node = nullptr, *d_lw_chan = nullptr, *d_lw_group = nullptr;   // [G], [c_out], [kLossMaxGroups]
  int* d_l_group = nullptr;                                                   // channel -> group [c_out]
  float *d_targets = nullptr, *d_lx = nullptr, *d_lden = nullptr;            // targets, noisy targets x, denoised D: [G, B, c_out]
  double* d_lpart = nullptr;                                                  // [loss_reduce_blocks][B][c_out] per-block column sums
  float *d_lsig = nullptr, *d_lloss = nullptr, *d_lpg = nullptr;             // per evaluation: sigma [B], loss [B], per_group [B][n_groups]
  int loss_cap = 0;                                                           // evaluations those three (and pin_lguard) hold
  unsigned* pin_lguard = nullptr;                                             // domain-guard counter as it stood after each evaluation
  int64_t loss_evaluations = 0, loss_device_us = 0;

  // ensemble verification (gc_ens_*, gc_ensemble.hip): a store of M member fields and the sums scored from it
  gci::BufferGroup ens_allocs{groups};               // everything sized by M: freed and replaced by gc_ens_reserve
  int ens_members = 0;                           // M (0: nothing reserved)
  std::vector<char> ens_filled;                  // per slot: pushed since the last gc_ens_reserve
  float* d_ens = nullptr;                        // [M][G, B, c_out] member fields
  double* d_ens_part = nullptr;                  // [blocks][6][B c_out] per-block column sums
  unsigned* d_ens_hpart = nullptr;               // [blocks][B c_out][M + 1] per-block rank counts, then [blocks][tiles] skipped points
  double* d_ens_sums = nullptr;                  // [6][B][c_out]
  unsigned long long* d_ens_hist = nullptr;      // [B][c_out][M + 1], then the skipped points of the call
  float *d_ens_w = nullptr, *d_ens_truth = nullptr;            // [G], [G, B, c_out]: made once, kept across reserves
  float *d_ens_mean = nullptr, *d_ens_var = nullptr;           // [G, B, c_out] each: made by the first call that asks for fields
  bool has_ens_w = false, has_ens_truth = false, has_ens_fields = false;
  gci::Event ev_ens_free{events}, ev_ens_done{events};         // stream order of a push from another handle
  gci::Meter ens{events};                                      // of gc_ens_score
  // member STATES (gc_ens_push_state): output channel j of a member comes from conditioning channel ens_state_src[j]
  // (-1: from the sample); the device copy is uploaded again only when the table changes
  std::vector<int32_t> ens_state_src;
  int* d_ens_state_src = nullptr;                // [c_out], made once

  // context store (gc_ctx_*, gc_ensemble.hip): n conditioning arrays beside the member store, one per ensemble member
  gci::BufferGroup ctx_allocs{groups};               // the store: freed and replaced by gc_ctx_reserve
  int ctx_slots = 0;                             // n (0: nothing reserved)
  float* d_ctx = nullptr;                        // [n][G, B, c_in]
  struct CtxSlot {
    bool saved = false;                          // written since the last gc_ctx_reserve
    bool read = false;                           // ev_r has been recorded since then
    hipEvent_t ev_w = nullptr, ev_r = nullptr;   // behind the last write / the last read, on whichever stream made it
  };
  std::vector<CtxSlot> ctx;                      // (events are kept across reserves and destroyed with the handle)

  // spherical-harmonic power spectra (gc_spec_*, gc_ens_spectrum, gc_spectrum.hip)
  gci::BufferGroup spec_allocs{groups};           // sized by the tables: freed and replaced by gc_spec_set_tables
  gci::BufferGroup spec_work_allocs{groups};      // sized by the coefficient sets a call keeps: replaced when a call needs more
  int sp_L = 0, sp_lat = 0, sp_lon = 0;          // lmax (0: no tables), n_lat, n_lon
  int sp_sets = 0;                               // coefficient sets d_sp_coef holds
  float *d_sp_q = nullptr, *d_sp_tab = nullptr;  // [L m][L l][n_lat] Legendre analysis, [2 L][n_lon] cosine rows then sine rows
  float* d_sp_field = nullptr;                   // [G, B, c_out]: a field handed over from the host
  double* d_sp_F = nullptr;                      // [2][L][n_lat][B c_out]: Fourier step of the field in flight
  double* d_sp_coef = nullptr;                   // [sp_sets][2][L m][L l][B c_out]
  double* d_sp_out = nullptr;                    // [6 + sp_sets][B c_out][L]: the sums, then the member powers
  unsigned* d_sp_flags = nullptr;                // [B c_out]: a value of the column was not finite
  gci::Meter spec{events};                       // of gc_spec_field and gc_ens_spectrum; invalid: columns

  // spectral band views (gc_ens_band_*, gc_spectrum.hip): the plan, and the scratch of the one field in flight
  gci::BufferGroup band_allocs{groups};           // the plan's tables, one buffer: freed and replaced by gc_ens_band_set, dropped by gc_spec_set_tables
  gci::KeyedGroup<2> band_work_allocs{groups};    // the scratch and the flags, sized by (B nu, M + 1): made again by the call that finds either changed
  bool band_set = false;                         // a plan has been set
  int band_c_src = 0, band_K = 0, band_nu = 0;   // source channels, bands, DISTINCT source channels the plan reads
  double* d_band_resp = nullptr;                 // [K][L] responses
  float *d_band_leg = nullptr, *d_band_tab = nullptr;   // [L m][n_lat][L l] Legendre synthesis; [n_lon][L m][2] (cos_s, sin_s)
  int *d_band_comp = nullptr, *d_band_chan = nullptr, *d_band_of = nullptr;   // [K] complement; [c_out] source channel, band
  int *d_band_ucol = nullptr, *d_band_ulist = nullptr;   // [c_out] place of the source channel in the list; [nu] the list, ascending
  float* d_band_gather = nullptr;                // [G][B nu]: the source columns of the field in flight, side by side
  double *d_band_F = nullptr, *d_band_coef = nullptr;    // [2][L][n_lat][B nu], [2][L m][L l][B nu]: its analysis
  double* d_band_G = nullptr;                    // [2][L m][n_lat][B c_out]: the Legendre synthesis of every derived column
  unsigned* d_band_flags = nullptr;              // [M + 1][B nu]: a value of the column of that field was not finite
  gci::Meter band{events};                       // of gc_ens_band; invalid: columns
  gci::Event ev_band_src{events};                // stream order behind the source handle

  // ensemble event verification (gc_ens_event_*, gc_events.hip): threshold fields and the tables scored from the member store
  gci::BufferGroup evt_allocs{groups};            // sized by T: thresholds, codes, weights; kept across gc_ens_reserve
  gci::KeyedGroup<2> evt_table_allocs{groups};    // sized by (T, M): made again by the scoring call that finds either changed
  int evt_T = 0;                                 // thresholds set (0: none)
  unsigned evt_dir_up = 0;                       // bit t: the event of threshold t is `value > thr`
  float* d_evt_thr = nullptr;                    // [T][G, B, c_out]
  unsigned char* d_evt_code = nullptr;           // [T][G, B, c_out]: k | o << 7, 255 = not counted
  unsigned* d_evt_wq = nullptr;                  // [G] integer node weights
  unsigned long long* d_evt_table = nullptr;     // weighted [T][B c_out][2][M + 1], counts (same), invalid [T]
  bool evt_scored = false;                       // a scoring call ran since gc_ens_event_set / gc_ens_reserve
  gci::Meter evt{events};                        // of gc_ens_event_score

  // derived and pooled ensemble fields (gc_ens_derive_*, gc_derive.hip): the plan, and the intermediate of the pooling passes
  gci::BufferGroup drv_allocs{groups};            // the plan's tables, one buffer: freed and replaced by gc_ens_derive_set
  gci::KeyedGroup<1> drv_work_allocs{groups};     // the intermediate, sized by its bytes: made again by the call that finds them changed
  bool drv_set = false;                          // a plan has been set
  int drv_c_src = 0, drv_pool = 0, drv_n_lat = 0, drv_n_lon = 0, drv_r_lat = 0;
  double *d_drv_affine = nullptr, *d_drv_roww = nullptr;       // [c_out][4] (sa, la, sb, lb), [n_lat]
  int *d_drv_op = nullptr, *d_drv_a = nullptr, *d_drv_b = nullptr, *d_drv_rlon = nullptr;   // [c_out] x 3, [n_lat]
  // a plan of gc_ens_derive_set_expr: its further tables lie in the same buffer of drv_allocs and go with it
  bool drv_expr = false;                         // the plan in force came through gc_ens_derive_set_expr
  bool drv_poles = false;                        // ... and has a vorticity / divergence channel on a grid with a pole row
  int drv_n_terms = 0;
  double drv_inv_2dlam = 0.0;
  double *d_drv_tq = nullptr, *d_drv_rows = nullptr;           // [5][n_terms] (coef, sa, la, sb, lb), [3][n_lat] (cos, 1 / (R cos), 1 / dphi)
  int *d_drv_tstart = nullptr, *d_drv_ta = nullptr, *d_drv_tb = nullptr, *d_drv_pole = nullptr;   // [c_out][3], [n_terms] x 2, [n_lat]
  unsigned char* d_drv_work = nullptr;           // 8 fields of row-pooled values: a float (max, min), or a double and an int32 (mean), per point
  gci::Meter drv{events};                                      // of gc_ens_derive
  gci::Event ev_drv_src{events};                               // stream order behind the source handle

  // ensemble order statistics (gc_ens_order_*, gc_order.hip): quantile fields and the bin sums of the CRPS decomposition
  gci::BufferGroup ord_allocs{groups};            // sized by Q: the quantile fields; kept across gc_ens_reserve
  gci::KeyedGroup<2> ord_work_allocs{groups};     // the partial and result buffers, sized by (M, Q): made again by the scoring call that finds either changed
  bool ord_set = false;                          // probabilities have been set (Q = 0 is a setting)
  int ord_Q = 0;
  double ord_p[8] = {};                          // the probabilities: lo, hi and f are formed per call from the current M
  float* d_ord_q = nullptr;                      // [Q][G, B, c_out] quantile fields
  double* d_ord_part = nullptr;                  // [blocks][2 (M + 1) + 3 + Q][B c_out] per-block column sums
  unsigned* d_ord_cpart = nullptr;               // [blocks][Q + 1][B c_out] per-block counts, then [blocks][tiles] skipped points
  double* d_ord_out = nullptr;                   // bins [B c_out][M + 1][2], extra [B c_out][3], pinball [B c_out][Q]
  unsigned long long* d_ord_outc = nullptr;      // counts [B c_out][Q + 1], then the skipped points of the call
  bool ord_ready = false;                        // an order call ran since gc_ens_order_set / gc_ens_reserve / gc_ens_derive
  gci::Meter ord{events};                        // of gc_ens_order_score and gc_ens_order_fields

  // an ensemble against a climatology (gc_ens_clim_score, gc_clim.hip): the sums of a pass over this handle's store and another's
  gci::BufferGroup clim_allocs{groups};           // sized by G, B and c_out alone: made by the first call, kept
  double* d_clim_part = nullptr;                 // [blocks][12][B c_out] per-block column sums
  unsigned* d_clim_cpart = nullptr;              // [blocks][B c_out] per-block counted points, then [blocks][tiles] skipped points
  double* d_clim_out = nullptr;                  // [B c_out][12]
  unsigned long long* d_clim_outc = nullptr;     // [B c_out] counted points, then the skipped points of the call
  gci::Meter clim{events};                       // of gc_ens_clim_score
  gci::Event ev_clim_src{events};                // stream order behind the climatology handle

  // extreme forecast index (gc_ens_efi_*, gc_efi.hip): the members of this handle's store ranked in the samples of another's
  gci::BufferGroup efi_allocs{groups};            // sized by G, B and c_out alone: made by the first call, kept across gc_ens_reserve
  gci::KeyedGroup<2> efi_table_allocs{groups};    // the integer tables, sized by (T + 1, E): made again by the scoring call that finds either changed
  bool efi_set = false;                          // events and bins have been set (T = 0 is a setting)
  int efi_T = 0, efi_E = 0;                      // events, EFI bins
  int efi_rank[4] = {}, efi_dir[4] = {};         // per event: the rank n, and +1 (lt_y >= n) or -1 (le_y <= n)
  int efi_fields = 0;                            // of this store: 0 no fields on the device, 1 the EFI alone, 2 the observed index too
  float* d_efi_field = nullptr;                  // [2][G, B, c_out]: the EFI, the observed index
  unsigned short* d_efi_code = nullptr;          // [G, B, c_out]: bin | event bits << 8, 0xFFFF = not counted
  unsigned* d_efi_wq = nullptr;                  // [G] integer node weights
  double* d_efi_tab = nullptr;                   // [65] the table a[0 .. K] of the call in flight
  double* d_efi_part = nullptr;                  // [blocks][6][B c_out] per-block column sums
  unsigned* d_efi_ipart = nullptr;               // [blocks][tiles] skipped points
  double* d_efi_out = nullptr;                   // [B c_out][6]
  unsigned long long* d_efi_outc = nullptr;      // the skipped points of the call
  unsigned long long* d_efi_table = nullptr;     // weighted [T][B c_out][2][E], then counts (same)
  gci::Meter efi{events};                        // of gc_ens_efi_score and gc_ens_efi_fields
  gci::Event ev_efi_src{events};                 // stream order behind the climatology handle

  // score maps (gc_ens_map_*, gc_map.hip): per-point accumulators of the marginal scores, one set of planes per slot
  gci::BufferGroup map_allocs{groups};            // everything sized by the plan: freed and replaced by gc_ens_map_set; not sized by M, kept across gc_ens_reserve
  bool map_set = false;                          // a plan has been set
  bool map_all = false;                          // ... that selects every channel (the kernels read no channel list)
  int map_C = 0, map_L = 0, map_T = 0;           // selected channels C', slots, event thresholds (0: no event planes)
  std::vector<int> map_M;                        // [L] the M of the dates a slot holds (0: none)
  std::vector<int64_t> map_dates;                // [L][2] field / event calls added into a slot
  int* d_map_chan = nullptr;                     // [C'] the selected channels, ascending
  double* d_map_sums = nullptr;                  // [L][6][G, B, C']
  unsigned* d_map_counts = nullptr;              // [L][3][G, B, C']
  unsigned* d_map_events = nullptr;              // [L][T][5][G, B, C']
  unsigned* d_map_ipart = nullptr;               // [kMapMaxBlocks][tiles] selected points a workgroup skipped
  int64_t map_bytes = 0;                         // bytes of the three accumulator arrays ("ens_map_bytes")
  gci::Meter map{events};                        // of gc_ens_map_accumulate and gc_ens_map_accumulate_events

  // time-window ensemble fields (gc_ens_window_*, gc_window.hip): the plan, and the ring of the last L pushed lead times
  gci::KeyedGroup<2> win_allocs{groups};          // the ring, one buffer sized by (L, M): made again by the push that finds either changed
  bool win_set = false;                          // a plan has been set
  int win_kind = 0, win_L = 0;                   // 0 linear, 1 max, 2 min; the window length
  float* d_win_ring = nullptr;                   // [L][(M + 1) [G, B, c_out] padded to whole float4s]: M members, then the truth
  double* d_win_coef = nullptr;                  // [64] coefficients of a linear window, oldest first: made once
  int64_t win_pushes = 0;                        // pushes since the last gc_ens_window_set / _reset: the next goes to slot win_pushes % L
  gci::Meter win{events};                        // of gc_ens_window_emit
  gci::Event ev_win_src{events};                 // stream order behind the source handle

  // multivariate ensemble scores (gc_ens_energy_*, gc_ens_variogram_*, gc_multivar.hip): the two plans and their sums
  gci::BufferGroup en_allocs{groups};             // the energy plan's tables: freed and replaced by gc_ens_energy_set
  gci::KeyedGroup<3> en_work_allocs{groups};      // the partial and result buffers, sized by (M, K, blocks): made again by the scoring call that finds one changed
  bool en_set = false;                           // an energy plan has been set
  int en_K = 0, en_nc_max = 0;                   // groups; channels of the largest
  int *d_en_gchan = nullptr, *d_en_goff = nullptr;   // the channels of the groups, group after group; [K + 1] where each starts
  double* d_en_scale = nullptr;                  // [c_out] a[c]
  double* d_en_part = nullptr;                   // [blocks][B K][P] per-block pair sums, then [blocks][B K] per-block S0
  unsigned* d_en_ipart = nullptr;                // [blocks][B K] skipped points
  double* d_en_out = nullptr;                    // D2 [B][K][P], then S0 [B][K]
  unsigned long long* d_en_outc = nullptr;       // the skipped points of the call
  gci::Meter en{events};                         // of gc_ens_energy_score
  gci::BufferGroup vg_allocs{groups};             // the variogram plan and the buffers sized by it: replaced by gc_ens_variogram_set
  bool vg_set = false;                           // a variogram plan has been set
  int vg_O = 0, vg_pk = 0, vg_n_lat = 0, vg_n_lon = 0;   // offsets; order 0 (p = 0.5), 1, 2; the grid
  int* d_vg_offs = nullptr;                      // [O][2] (di, dj)
  double* d_vg_part = nullptr;                   // [blocks][O][4][B c_out] per-block column sums
  unsigned* d_vg_cpart = nullptr;                // [blocks][O][B c_out] per-block valid pairs
  double* d_vg_out = nullptr;                    // [4][B c_out][O]
  unsigned long long* d_vg_outc = nullptr;       // [B c_out][O]
  gci::Meter vg{events};                         // of gc_ens_variogram_score

  // threshold-weighted CRPS (gc_ens_tail_*, gc_tail.hip): threshold fields of its own and the sums of one sort per point
  gci::BufferGroup tail_allocs{groups};           // sized by T: the thresholds; kept across gc_ens_reserve
  gci::KeyedGroup<1> tail_work_allocs{groups};    // the partial and result buffers, sized by T: made again by the scoring call that finds it changed
  int tail_T = 0;                                // thresholds set (0: none)
  unsigned tail_dir_up = 0;                      // bit t: threshold t is the upper tail, weight 1{z >= thr}
  float* d_tail_thr = nullptr;                   // [T][G, B, c_out]
  double* d_tail_part = nullptr;                 // [blocks][T][4][B c_out] per-block column sums
  unsigned* d_tail_cpart = nullptr;              // [blocks][T][B c_out] per-block counted points
  double* d_tail_out = nullptr;                  // [T][B c_out][4]
  unsigned long long* d_tail_outc = nullptr;     // [T][B c_out] counted points
  gci::Meter tail{events};                       // of gc_ens_tail_score

  // regional ensemble scores (gc_ens_region_*, gc_region.hip): the plan on the host, its device copy and the sums of one pass
  gci::KeyedGroup<1> reg_allocs{groups};          // the plan's device copy and everything sized by it and by M (the key): replaced as a whole
  int reg_R = 0;                                 // regions set (0: no plan)
  int reg_listed = 0, reg_blocks = 0;            // nodes that belong to a region; entries of the block table
  std::vector<int> reg_plan;                     // order [listed], {begin, end} [blocks], atom bits [blocks]: kept across gc_ens_reserve
  int* d_reg_plan = nullptr;                     // reg_plan as it lies
  double* d_reg_part = nullptr;                  // [blocks][6][B c_out] per-block column sums
  unsigned* d_reg_hpart = nullptr;               // [blocks][B c_out][M + 1] per-block rank counts, then [blocks][tiles] skipped points
  double* d_reg_sums = nullptr;                  // [R][6][B][c_out]
  unsigned long long* d_reg_hist = nullptr;      // [R][B][c_out][M + 1], then [R] skipped points
  gci::Meter reg{events};                        // of gc_ens_region_score

  // ensemble feature detection (gc_ens_feature_*, gc_feature.hip): the plan, the work of a chunk of fields, the centre lists
  gci::BufferGroup feat_allocs{groups};           // the plan's tables, one buffer: freed and replaced by gc_ens_feature_set
  gci::KeyedGroup<1> feat_work_allocs{groups};    // the work buffers and the lists, one buffer sized by its bytes: made again by the call that finds them changed
  bool feat_set = false;                         // a plan has been set
  bool feat_listed = false;                      // the lists are those of a call under the current plan
  int feat_c_src = 0, feat_n_lat = 0, feat_n_lon = 0, feat_max = 0, feat_list_M = 0;
  double* d_feat_depth = nullptr;                // [c_out]
  int* d_feat_tab = nullptr;                     // [7][c_out] per-detector tables, then r_lon, ring_lon, strike_lon [c_out][n_lat]
  unsigned char* d_feat_work = nullptr;          // 8 fields of keys, row minima, flags and block counts; then the lists
  int *d_feat_count = nullptr, *d_feat_node = nullptr;   // [M + 1][B][c_out], [M + 1][B][c_out][max_centres]: inside d_feat_work
  float* d_feat_value = nullptr;                 // [M + 1][B][c_out][max_centres]
  gci::Meter feat{events};                       // of gc_ens_feature
  gci::Event ev_feat_src{events};                // stream order behind the source handle

  // fractions skill score (gc_ens_fss_*, gc_fss.hip): the plan of the scales, and the row sums of a chunk of columns
  gci::BufferGroup fss_allocs{groups};            // the plan's tables, one buffer: freed and replaced by gc_ens_fss_set; kept across gc_ens_reserve
  gci::KeyedGroup<3> fss_work_allocs{groups};     // the work buffer, the partials and the sums, sized by their three lengths: made again by the call that finds one changed
  int fss_S = 0;                                 // scales set (0: no plan)
  int fss_n_lat = 0, fss_n_lon = 0;
  std::vector<int32_t> fss_rlat;                 // [S], as on the device (gc_ens_fss_fields passes one by value)
  int *d_fss_rlat = nullptr, *d_fss_rlon = nullptr;   // [S], [S][n_lat]
  unsigned* d_fss_roww = nullptr;                // [n_lat] integer row weights
  uint2* d_fss_work = nullptr;                   // [S + 1][G][chunk columns]: (k sum, o | counts << 16) of the row windows; last slab: two float fields
  double* d_fss_part = nullptr;                  // [blocks][S][4][chunk columns] per-block column sums
  double* d_fss_out = nullptr;                   // [T][S][B c_out][4]
  gci::Meter fss{events};                        // of gc_ens_fss_score

  // HIP-graph replay of the sampler (gc_set_option "graphs"): one captured graph per sample signature
  struct SampleGraph {
    std::vector<float> sigmas;
    int skip_dead = 1;
    const float* noise = nullptr;      // the initial-noise buffer baked into the graph (it is double-buffered)
    bool feat16 = false;
    gci::Route route;                  // signature: f16, st16; whole once captured (a replay restores last_route)
    hipGraph_t graph = nullptr;
    // null until the signature has been seen twice; TWO executables of the one captured graph, launched alternately,
    // each with an event recorded behind its last launch: an executable is never launched while its previous
    // instance may still be running (the host waits for that event first, outside any lock)
    hipGraphExec_t exec = nullptr, exec2 = nullptr;
    hipEvent_t done[2] = {nullptr, nullptr};
    int next = 0;
    int calls = 0;
    int64_t launches_per_call = 0, launches = 0;
    uint64_t last_use = 0;
  };
  bool use_graphs = true;              // GC_TUNE_GRAPH=0 / gc_set_option(h, "graphs", "off"): always enqueue eagerly
  std::vector<SampleGraph> sample_graphs;
  uint64_t graph_clock = 0;
  int64_t graph_replays = 0, graph_captures = 0;
  int debug_layer_limit = -1;  // gc_debug_set_layer_limit
  int debug_stop_layer = -1, debug_stop_phase = -1;   // gc_debug_set_stop: forward() returns inside this block
  bool f16x3 = true;           // GEMM-shaped kernels run as 3 fp16 MFMAs per product (gc_set_option)
  float g2m_agg_norm = 0.f;    // "grid2mesh_aggregate_normalization": the grid2mesh edge sums are divided by it (0: not)
  bool feat16 = false;         // "features" = "f16": activations rounded to fp16 where stored (BASELINE configs[4])
  // f16x3 domain guard: operands outside fp16 range poison the output with
  // NaN / Inf (no clamp anywhere); the output is checked on the device once per call and a poisoned
  // call is re-run on the exact-f32 kernels, which treat NaN / Inf / huge inputs like the reference.
  bool weights_f16_unsafe = false;   // a weight is non-finite or beyond fp16 range: f32 kernels only
  bool in_fallback = false;          // forward() is running the f32 re-run of a poisoned call
  unsigned* d_nonfinite = nullptr;   // device counter bumped by gc_finite_check
  unsigned* h_nonfinite = nullptr;   // pinned host copy
  unsigned nonfinite_seen = 0;
  int64_t range_fallbacks = 0;       // calls re-run in f32 (gc_get_counter "range_fallbacks")
  int64_t static_embedding_fallbacks = 0;   // times the static embeddings were made again in f32 (compute_static_embeddings)
  bool guard_pending = false;        // a resident sample has not been checked yet
  std::vector<float> last_sigmas;    // arguments of that sample, for the re-run
  int last_skip_dead = 1;
  unsigned long long last_stream0 = 0;
  int64_t launches_last_call = 0, launch_count = 0;   // kernel launches of the last denoiser forward
  // pinned staging buffers of the asynchronous uploads (caller buffers are free on return)
  float *pin_cond = nullptr, *pin_noise = nullptr, *pin_forc = nullptr;
  size_t pin_forc_cap = 0;
  hipEvent_t ev_pin = nullptr;       // last H2D copy out of a staging buffer
  // ensemble exchange (gc_comm_*): one RCCL communicator per handle, collectives on h->stream
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  double* d_comm_scalar = nullptr;

  // profiling
  int prof_cls = -1;
  int prof_stride = 1;
  unsigned prof_seen = 0;
  std::vector<hipEvent_t> prof_events;
  size_t prof_used = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

namespace gci {

#define GC_HIP(h, call)                                                                     \
  do {                                                                                      \
    hipError_t e__ = (call);                                                                \
    if (e__ != hipSuccess) {                                                                \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e__);                        \
      return GC_ERR_HIP;                                                                    \
    }                                                                                       \
  } while (0)

inline int fail(gc_handle* h, int code, const std::string& msg) {
  h->err = msg;
  return code;
}

// Poison mode (GC_DEBUG_POISON=1, DESIGN.md "Poisoned allocations"): the bytes a fresh buffer is filled with.  0xFF makes
// every float, double and fp16 word a NaN.  0x01 makes a stray count 16 843 009 and a stray event code (k = 1, o = 0), both
// of which the `==` assertions see, and keeps a stray index or loop bound bounded (0xFF would read as "not counted" in the
// event codes and as 4 294 967 295 in a bound).
constexpr int kPoisonFloat = 0xFF, kPoisonInt = 0x01;

// owner: the list that frees the buffer (default h->allocs: freed in destroy).  as_float: the buffer holds floating-point
// values (what its poison pattern follows): by default what T says; an fp16 plane behind an integer container passes true.
template <typename T>
int dev_alloc(gc_handle* h, T** p, size_t count, BufferGroup* owner = nullptr, bool as_float = std::is_floating_point<T>::value) {
  void* q = nullptr;
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  GC_HIP(h, hipMalloc(&q, bytes));
  (owner ? owner : &h->allocs)->ptrs.push_back(q);
  if (h->poison) {
    // a synchronous fill, complete before anything on the handle's non-blocking streams (which the null stream does not
    // order) or a `from` copy of the caller can touch the buffer; this mode is never timed
    GC_HIP(h, hipMemset(q, as_float ? kPoisonFloat : kPoisonInt, bytes));
    GC_HIP(h, hipDeviceSynchronize());
    ++h->poison_allocs;
    h->poison_bytes += (int64_t)bytes;
  }
  *p = reinterpret_cast<T*>(q);
  return GC_OK;
}

// A pinned staging buffer of the handle; poison mode fills it with 0xFF on the host.
template <typename T>
hipError_t pinned_alloc(gc_handle* h, T** p, size_t count) {
  const hipError_t e = hipHostMalloc((void**)p, count * sizeof(T), hipHostMallocDefault);
  if (e == hipSuccess && h->poison) std::memset(*p, kPoisonFloat, count * sizeof(T));
  return e;
}

template <typename T>
int dev_upload(gc_handle* h, T** p, const std::vector<T>& v, BufferGroup* owner = nullptr) {
  int rc = dev_alloc(h, p, v.size(), owner);
  if (rc) return rc;
  if (!v.empty()) GC_HIP(h, hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return GC_OK;
}

// `count` elements at *p, to be allocated into a group (alloc_all, sized_for); `from`: host values copied into them
template <typename T>
struct Buf {
  T** p;
  size_t count;
  const T* from;
};
template <typename T>
Buf<T> buf(T** p, size_t count, const T* from = nullptr) { return {p, count, from}; }
template <typename T>
Buf<T> buf(T** p, const std::vector<T>& v) { return {p, v.size(), v.data()}; }

template <typename T>
int alloc_one(gc_handle* h, BufferGroup& g, const Buf<T>& b) {
  if (int rc = dev_alloc(h, b.p, b.count, &g)) return rc;
  if (b.from && b.count) GC_HIP(h, hipMemcpy(*b.p, b.from, b.count * sizeof(T), hipMemcpyHostToDevice));
  return GC_OK;
}

// These buffers into `g`, in order; the first failure frees the whole group and is returned.
template <typename... T>
int alloc_all(gc_handle* h, BufferGroup& g, Buf<T>... b) {
  int rc = GC_OK;
  ((rc = rc ? rc : alloc_one(h, g, b)), ...);
  if (rc) g.free();
  return rc;
}

// The buffers of `g` are those made for `key`, or the old ones are dropped (behind everything on the handle's stream) and
// these made in their place.
template <size_t N, typename... T>
int sized_for(gc_handle* h, KeyedGroup<N>& g, const std::array<size_t, N>& key, Buf<T>... b) {
  if (!g.differs(key)) return GC_OK;
  GC_HIP(h, g.drop(h->stream));
  if (int rc = alloc_all(h, g, b...)) return rc;
  g.key = key;
  return GC_OK;
}

// ---- launch wrapper with optional per-class event bracketing --------------------------------
template <typename F>
int launch(gc_handle* h, int cls, F&& f) {
  ++h->launch_count;
  bool prof = (h->prof_cls == cls) && (h->prof_used + 2 <= h->prof_events.size());
  if (prof && h->prof_stride > 1) prof = ((h->prof_seen++ % (unsigned)h->prof_stride) == 0);
  if (prof) GC_HIP(h, hipEventRecord(h->prof_events[h->prof_used], h->stream));
  hipError_t e = f();
  if (e != hipSuccess) {
    h->err = std::string("launch ") + gc::kernel_class_name(cls) + ": " + hipGetErrorString(e);
    return GC_ERR_HIP;
  }
  if (prof) {
    GC_HIP(h, hipEventRecord(h->prof_events[h->prof_used + 1], h->stream));
    h->prof_used += 2;
  }
  return GC_OK;
}

// what gc_last_error(nullptr) returns: the failure of an entry point that has no handle yet (gc_create)
inline thread_local std::string g_create_error;

// Asynchronous H2D through a handle-owned pinned buffer of `cap` bytes, in pieces where the payload is longer: the
// caller's buffer is free on return.
inline int staged_upload_bytes(gc_handle* h, void* pinned, size_t cap, void* dev, const void* src, size_t bytes) {
  size_t off = 0;
  do {
    const size_t n = std::min(cap, bytes - off);
    GC_HIP(h, hipEventSynchronize(h->ev_pin));     // the previous copy out of a staging buffer is done
    std::memcpy(pinned, static_cast<const char*>(src) + off, n);
    GC_HIP(h, hipMemcpyAsync(static_cast<char*>(dev) + off, pinned, n, hipMemcpyHostToDevice, h->stream));
    GC_HIP(h, hipEventRecord(h->ev_pin, h->stream));
    off += n;
  } while (off < bytes);
  return GC_OK;
}
// `count` floats that fit the buffer
inline int staged_upload(gc_handle* h, float* pinned, float* dev, const float* src, size_t count) {
  return staged_upload_bytes(h, pinned, count * sizeof(float), dev, src, count * sizeof(float));
}

// No C++ exception crosses the C ABI: every entry point runs inside this wrapper.
template <typename F>
int guarded(gc_handle* h, F&& f) noexcept {
  const char* what = "unknown C++ exception";
  try {
    return f();
  } catch (const std::bad_alloc&) {
    what = "out of host memory (std::bad_alloc)";
  } catch (const std::exception& e) {
    try {
      (h ? h->err : g_create_error) = std::string("C++ exception: ") + e.what();
      return GC_ERR_INTERNAL;
    } catch (...) {
    }
  } catch (...) {
  }
  try {
    (h ? h->err : g_create_error) = what;
  } catch (...) {
  }
  return GC_ERR_INTERNAL;
}

// gc_weights.hip
extern const char* const P_M2G;
void build_specs(gc_handle* h);
float f16_bits_to_f32(uint16_t h);
void free_weights(gc_handle* h);
int finalize_weights(gc_handle* h);
int build_embed_cache(gc_handle* h);
// gc_forward.hip
Route make_route(const gc_handle* h);
bool build_attention_items(const gc::HostGraph& g, std::vector<int>* items, std::vector<int>* tiles);
int run_m2g_edge(gc_handle* h, const float* cond, bool fused);
bool edge_terms_possible(const gc_handle* h);
int drop_edge_terms(gc_handle* h);
int ensure_edge_terms(gc_handle* h, const std::vector<float>& call_sigma);
int forward(gc_handle* h, float sigma_scalar, const float* cond_ready = nullptr);
int compute_static_embeddings(gc_handle* h);
// gc_sampler.hip
int guard_enqueue(gc_handle* h, const float* p, size_t n);
bool guard_tripped(gc_handle* h);
int noise_field(gc_handle* h, const float* base, float scale, float* out);
int run_sampler(gc_handle* h, const float* sigmas, int n, int skip_dead, gc_sample_stats* stats);
int resolve_guard(gc_handle* h);
void destroy_sample_graph(gc_handle::SampleGraph& g);
void drop_sample_graphs(gc_handle* h);
int loss_eval(gc_handle* h, int e, const float* sig, bool draw_noise, bool want_den);

}  // namespace gci
