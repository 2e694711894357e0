// Ensemble verification on the device (include/gencast_hip.h, gc_ens_*): a store of M member fields on the handle and
// one scoring pass over it -- CRPS terms, error and spread of the ensemble mean, the rank histogram, and on request
// the mean and variance fields.  Kernels and their host code live together here; DESIGN.md section 8c has the
// definitions and the error bound the tests assert.  Below them: the member STATE gather (gc_ens_push_state) and the
// context store (gc_ctx_*) that let a multi-step ensemble forecast stay on the device.
//
// Per point (g, b, c), from the float32 members x_0 .. x_{M-1} and the truth y, in double:
//   m  = (sum_i x_i) / M                       ascending slot order
//   s2 = sum_i (x_i - m)^2 / (M - 1)           two passes, ascending slot order
//   ae = (sum_i |x_i - y|) / M
//   d  = sum_{i<j} |x_i - x_j| / (M (M-1) / 2)
//   r  = #{i : x_i < y}                        ties are not randomised: a member equal to y is not below it
// A point counts when y and all M members are finite.  Per column (b, c), over the counted nodes, w = node weight:
//   S0 = sum w, S1 = sum w (m - y), S2 = sum w (m - y)^2, S3 = sum w s2, S4 = sum w ae, S5 = sum w d,  H[r] += 1
// No atomics on floats: every partial has one writer and every sum a fixed order, so the result does not depend on how
// the launch was scheduled.  The rank counts are integers; their LDS atomics commute.
#include "gc_colsum.h"
#include "gc_store.h"

// the per-point arithmetic is the definition above, operation for operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace gc {

constexpr int kEnsMinMembers = 2, kEnsMaxMembers = 64;

// (This kernel and its finish keep their own text: on the shared pieces of gc_colsum.h the pass timed slower.)
// Thread layout of gc_loss_reduce_kernel: a grid node's B rows are W = B c_out consecutive floats; grid.y cuts W into
// column tiles of at most 256; inside a tile of wt columns thread t owns column t % wt (ONE accumulator set) of node
// lane t / wt, q = 256 / wt lanes; block x walks the contiguous node range [x per, (x + 1) per) in steps of q.
// The M values of a point are read once from HBM (M loads of stride `field`, each coalesced across the wave) into the
// thread's own column of an LDS tile [M][256]; the second pass and the O(M^2) pair loop read them from there.
// Dynamic LDS: float[M][256], then unsigned[wt][M + 1] rank counts of the block.
// Out, as plain stores: part[block x][6][W] (double), hpart[block x][W][M + 1], ipart[block x][tile] (points skipped).
__global__ __launch_bounds__(256) void gc_ens_score_kernel(const float* __restrict__ mem, size_t field, int M,
                                                            const float* __restrict__ truth,
                                                            const float* __restrict__ node_w, int G, int W, int per,
                                                            double* __restrict__ part, unsigned* __restrict__ hpart,
                                                            unsigned* __restrict__ ipart, float* __restrict__ mean,
                                                            float* __restrict__ var) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ens_lds[];
  __shared__ double lane_sum[256];
  __shared__ unsigned skipped;
  float* const tile = reinterpret_cast<float*>(ens_lds);
  unsigned* const hist = reinterpret_cast<unsigned*>(tile + (size_t)M * 256);
  const int col0 = blockIdx.y * 256;
  const int wt = min(256, W - col0);
  const int q = 256 / wt;
  const int tid = threadIdx.x;
  const int lane = tid / wt;
  const int cl = tid - lane * wt;
  const int col = col0 + cl;
  const int bins = M + 1;
  for (int i = tid; i < wt * bins; i += 256) hist[i] = 0u;
  if (tid == 0) skipped = 0u;
  __syncthreads();
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned inv = 0;
  if (lane < q) {
    float* const my = tile + tid;                  // x_k at my[k * 256]: a bank of its own for every lane
    const double dM = (double)M, pairs = 0.5 * dM * (dM - 1.0);
    const int n_end = min(G, (int)(blockIdx.x + 1) * per);
    for (int n = blockIdx.x * per + lane; n < n_end; n += q) {
      const size_t i = (size_t)n * W + col;
      const float y = truth[i];
      bool xfin = true;
      double sum = 0.0;
#pragma unroll 4
      for (int k = 0; k < M; ++k) {
        const float x = mem[(size_t)k * field + i];
        my[k * 256] = x;
        xfin = xfin && isfinite(x);
        sum += (double)x;
      }
      const double m = sum / dM;
      const bool ok = xfin && isfinite(y);
      double s2 = 0.0, ae = 0.0;
      int r = 0;
      if (xfin) {
        const double yd = (double)y;
#pragma unroll 4
        for (int k = 0; k < M; ++k) {
          const float x = my[k * 256];
          const double dx = (double)x - m;
          s2 += dx * dx;
          ae += fabs((double)x - yd);
          r += x < y ? 1 : 0;
        }
        s2 /= dM - 1.0;
      }
      if (mean) {
        mean[i] = xfin ? (float)m : __builtin_nanf("");
        var[i] = xfin ? (float)s2 : __builtin_nanf("");
      }
      if (!ok) {
        ++inv;
        continue;
      }
      double d0 = 0.0, d1 = 0.0;                    // two chains: the pair sum has no prescribed order
      for (int a = 0; a + 1 < M; ++a) {
        const double xa = (double)my[a * 256];
        int b = a + 1;
        for (; b + 1 < M; b += 2) {
          d0 += fabs(xa - (double)my[b * 256]);
          d1 += fabs(xa - (double)my[(b + 1) * 256]);
        }
        if (b < M) d0 += fabs(xa - (double)my[b * 256]);
      }
      const double w = (double)node_w[n], e = m - (double)y;
      s[0] += w;
      s[1] += w * e;
      s[2] += w * (e * e);
      s[3] += w * s2;
      s[4] += w * (ae / dM);
      s[5] += w * ((d0 + d1) / pairs);
      atomicAdd(&hist[cl * bins + r], 1u);
    }
  }
  if (inv) atomicAdd(&skipped, inv);
  // the q lanes of a column, added in lane order
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    lane_sum[tid] = s[k];
    __syncthreads();
    if (tid < wt) {
      double t = lane_sum[tid];
      for (int l = 1; l < q; ++l) t += lane_sum[l * wt + tid];
      part[((size_t)blockIdx.x * 6 + k) * W + col] = t;
    }
    __syncthreads();
  }
  unsigned* const hp = hpart + ((size_t)blockIdx.x * W + col0) * bins;
  for (int i = tid; i < wt * bins; i += 256) hp[i] = hist[i];
  if (tid == 0) ipart[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = skipped;
}

// One workgroup per column tile.  The blocks of a column are added the way gc_loss_finish_kernel adds them: thread t
// owns column t % wt and the contiguous block range of lane t / wt, the lanes are combined in lane order -- a fixed
// order, ascending in the block index.  sums [6][W]; hist [W][M + 1] then one word: the points the call skipped.
__global__ __launch_bounds__(256) void gc_ens_finish_kernel(const double* __restrict__ part,
                                                             const unsigned* __restrict__ hpart,
                                                             const unsigned* __restrict__ ipart, int blocks, int W, int M,
                                                             double* __restrict__ sums,
                                                             unsigned long long* __restrict__ hist) {
  __shared__ double lane_sum[256];
  __shared__ unsigned long long skipped;
  const int col0 = blockIdx.x * 256;
  const int wt = min(256, W - col0);
  const int q = 256 / wt;
  const int tid = threadIdx.x;
  const int lane = tid / wt;
  const int col = col0 + (tid - lane * wt);
  const int bper = (blocks + q - 1) / q;
  const int bins = M + 1;
  if (tid == 0) skipped = 0ull;
  for (int k = 0; k < 6; ++k) {
    double t = 0.0;
    if (lane < q) {
      const int b_end = min(blocks, (lane + 1) * bper);
#pragma unroll 8
      for (int b = lane * bper; b < b_end; ++b) t += part[((size_t)b * 6 + k) * W + col];
    }
    lane_sum[tid] = t;
    __syncthreads();
    if (tid < wt) {
      double tot = lane_sum[tid];
      for (int l = 1; l < q; ++l) tot += lane_sum[l * wt + tid];
      sums[(size_t)k * W + col] = tot;
    }
    __syncthreads();
  }
  for (int e = tid; e < wt * bins; e += 256) {
    unsigned long long t = 0ull;
    for (int b = 0; b < blocks; ++b) t += hpart[((size_t)b * W + col0) * bins + e];
    hist[(size_t)col0 * bins + e] = t;
  }
  if (blockIdx.x == 0) {
    unsigned long long t = 0ull;
    for (int i = tid; i < blocks * (int)gridDim.x; i += 256) t += ipart[i];
    if (t) atomicAdd(&skipped, t);
    __syncthreads();
    if (tid == 0) hist[(size_t)W * bins] = skipped;
  }
}

static hipError_t launch_ens_score(hipStream_t s, const float* mem, size_t field, int M, const float* truth, const float* node_w,
                                   int G, int B, int c_out, double* part, unsigned* hpart, unsigned* ipart, float* mean, float* var) {
  const int W = B * c_out;
  const int blocks = loss_reduce_blocks(G, B, c_out);
  const int per = (G + blocks - 1) / blocks;
  const size_t lds = ens_score_lds(M, W);
  if (lds > 64 * 1024) {                           // (a per-device property of the kernel; setting it again is harmless)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gc_ens_score_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(gc_ens_score_kernel, dim3(blocks, (W + 255) / 256), dim3(256), lds, s, mem, field, M, truth, node_w, G, W,
                     per, part, hpart, ipart, mean, var);
  return hipGetLastError();
}

static hipError_t launch_ens_finish(hipStream_t s, const double* part, const unsigned* hpart, const unsigned* ipart, int blocks,
                                    int W, int M, double* sums, unsigned long long* hist) {
  hipLaunchKernelGGL(gc_ens_finish_kernel, dim3((W + 255) / 256), dim3(256), 0, s, part, hpart, ipart, blocks, W, M, sums, hist);
  return hipGetLastError();
}

// Member state (gc_ens_push_state): output channel j of a member is conditioning channel state_src[j] of the ADVANCED
// context, or sample channel j where the target has no input channel (state_src[j] < 0).  A gather, no arithmetic: the
// stored value is bit for bit the value the next forecast step is conditioned on.  Thread layout of the kernels above:
// thread t owns column t % wt = (b, j) of node lane t / wt, so the active threads of a block store q whole consecutive
// member rows; the reads are a fixed permutation inside the node's B c_in conditioning floats.
__global__ __launch_bounds__(256) void gc_ens_state_kernel(const float* __restrict__ cond, const float* __restrict__ sample,
                                                            const int* __restrict__ state_src, int G, int B, int c_in,
                                                            int c_out, float* __restrict__ member) {
  const int W = B * c_out;
  const int col0 = blockIdx.y * 256;
  const int wt = min(256, W - col0);
  const int q = 256 / wt;
  const int lane = threadIdx.x / wt;
  if (lane >= q) return;
  const int col = col0 + ((int)threadIdx.x - lane * wt);
  const int b = col / c_out;
  const int sc = state_src[col - b * c_out];
  const float* const from = sc >= 0 ? cond + (size_t)b * c_in + sc : sample + col;
  const size_t stride = sc >= 0 ? (size_t)B * c_in : (size_t)W;
  for (size_t n = (size_t)blockIdx.x * q + lane; n < (size_t)G; n += (size_t)gridDim.x * q)
    member[n * W + col] = from[n * stride];
}

static hipError_t launch_ens_state(hipStream_t s, const float* cond, const float* sample, const int* state_src, int G, int B,
                                   int c_in, int c_out, float* member) {
  const int W = B * c_out;
  const int q = 256 / std::min(256, W);
  const int blocks = std::max(1, std::min(1024, (G + q - 1) / q));
  hipLaunchKernelGGL(gc_ens_state_kernel, dim3(blocks, (W + 255) / 256), dim3(256), 0, s, cond, sample, state_src, G, B, c_in,
                     c_out, member);
  return hipGetLastError();
}

}  // namespace gc

using namespace gci;

namespace {

// the entries that need G only: no weights, no gc_finalize
int ens_ready(gc_handle* h, bool store) {
  const int rc = need_graph(h);
  return rc || !store ? rc : need_store(h);
}

int ens_slot(gc_handle* h, int32_t slot) {
  if (slot < 0 || slot >= h->ens_members) return fail(h, GC_ERR_INVALID_ARGUMENT, "slot outside [0, n_members)");
  return GC_OK;
}

int ctx_ready(gc_handle* h, int32_t slot) {
  if (int rc = need_graph(h)) return rc;
  if (h->ctx_slots == 0) return fail(h, GC_ERR_STATE, "no context store (gc_ctx_reserve)");
  if (slot < 0 || slot >= h->ctx_slots) return fail(h, GC_ERR_INVALID_ARGUMENT, "slot outside [0, n)");
  return GC_OK;
}

// the handle on the other side of a context copy: same device, same [G, B, c_in], finalized
int ctx_peer(gc_handle* h, const gc_handle* o) {
  if (int rc = check_peer(h, o, "other", true)) return rc;
  if (!o->finalized) return fail(h, GC_ERR_STATE, "gc_finalize has not been called on the other handle");
  return GC_OK;
}

// the handle a member is pushed from: same device, same [G, B, c_out] (and c_in for a state), a checked sample on it
int push_source(gc_handle* h, gc_handle* src, bool c_in) {
  if (int rc = check_peer(h, src, "source", c_in, h->cfg.c_out)) return rc;
  if (!src->finalized || !src->has_sample) return fail(h, GC_ERR_STATE, "no sample on the source handle (gc_sample_resident)");
  return GC_OK;
}

}  // namespace

extern "C" {

int gc_ens_reserve(gc_handle* h, int32_t n_members) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ens_ready(h, false);
  if (rc) return rc;
  if (n_members < gc::kEnsMinMembers || n_members > gc::kEnsMaxMembers)
    return fail(h, GC_ERR_UNSUPPORTED, "n_members must be in 2..64");
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, h->ens_allocs.drop(h->stream));         // every push into the old store has landed (pushes from other handles are ordered into this stream)
  h->ens_members = 0;
  h->ens_filled.clear();
  h->has_ens_fields = false;
  h->evt_scored = false;                           // (gc_events.hip: the codes were of the old store)
  h->ord_ready = false;                            // (gc_order.hip: so were the quantile fields)
  h->efi_fields = 0;                               // (gc_efi.hip: and the index fields)
  h->d_ens = nullptr;
  h->d_ens_state_src = nullptr;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, W = c.batch * c.c_out, M = n_members;
  const size_t blocks = (size_t)gc::loss_reduce_blocks(G, c.batch, c.c_out), tiles = (size_t)(W + 255) / 256;
  if ((rc = alloc_all(h, h->ens_allocs, buf(&h->d_ens, (size_t)M * field_len(h)), buf(&h->d_ens_part, blocks * 6 * W),
                      buf(&h->d_ens_hpart, blocks * W * (M + 1) + blocks * tiles), buf(&h->d_ens_sums, (size_t)6 * W),
                      buf(&h->d_ens_hist, (size_t)W * (M + 1) + 1), buf(&h->d_ens_state_src, (size_t)c.c_out))))
    return rc;
  h->ens_state_src.clear();
  GC_HIP(h, h->ev_ens_free.ensure());
  GC_HIP(h, h->ev_ens_done.ensure());
  h->ens_filled.assign((size_t)M, 0);
  h->ens_members = M;
  return GC_OK;
  });
}

int gc_ens_set_node_weight(gc_handle* h, const float* w) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ens_ready(h, false);
  if (rc) return rc;
  if (!w) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  GC_HIP(h, hipSetDevice(h->device));
  if (!h->d_ens_w && (rc = dev_alloc(h, &h->d_ens_w, (size_t)h->hg.G))) return rc;
  // on the handle's stream (ordered behind whatever still runs there), then waited for: the array is the caller's again
  GC_HIP(h, hipMemcpyAsync(h->d_ens_w, w, (size_t)h->hg.G * sizeof(float), hipMemcpyHostToDevice, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  h->has_ens_w = true;
  return GC_OK;
  });
}

int gc_ens_push(gc_handle* h, int32_t slot, gc_handle* src) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ens_ready(h, true);
  if (rc || (rc = ens_slot(h, slot))) return rc;
  if (!src) src = h;
  if ((rc = push_source(h, src, false))) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = relay(h, src, resolve_guard(src), "source"))) return rc;   // the member is the CHECKED sample (exact-f32 re-run included)
  float* const dst = h->d_ens + (size_t)slot * field_len(h);
  const size_t bytes = field_len(h) * sizeof(float);
  // on the SOURCE's stream, in front of that handle's next sample
  auto copy = [&]() -> int {
    GC_HIP(h, hipMemcpyAsync(dst, src->d_sx, bytes, hipMemcpyDeviceToDevice, src->stream));
    return GC_OK;
  };
  if ((rc = src == h ? copy() : on_peer_stream(h, src, copy))) return rc;
  h->ens_filled[(size_t)slot] = 1;
  return GC_OK;
  });
}

int gc_ens_push_host(gc_handle* h, int32_t slot, const float* field) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ens_ready(h, true);
  if (rc || (rc = ens_slot(h, slot))) return rc;
  if (!field) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = staged_upload(h, h->pin_noise, h->d_ens + (size_t)slot * field_len(h), field, field_len(h)))) return rc;
  h->ens_filled[(size_t)slot] = 1;
  return GC_OK;
  });
}

int gc_ens_score(gc_handle* h, const float* truth, int32_t want_fields, double* sums, uint64_t* rank_hist) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_graph(h)) || (rc = need_store(h)) || (rc = need_out(h, sums)) || (rc = store_complete(h, h)) || (rc = need_weights(h)))
    return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_score"))) return rc;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, B = c.batch, W = B * c.c_out, M = h->ens_members;
  const size_t field = field_len(h);
  if (want_fields && !h->d_ens_mean) {
    if ((rc = dev_alloc(h, &h->d_ens_mean, field)) || (rc = dev_alloc(h, &h->d_ens_var, field))) return rc;
  }
  hipStream_t s = h->stream;
  const int blocks = gc::loss_reduce_blocks(G, B, c.c_out);
  unsigned* const ipart = h->d_ens_hpart + (size_t)blocks * W * (M + 1);
  std::vector<uint64_t> hist((size_t)W * (M + 1) + 1);
  rc = timed(h, h->ens,
             [&] {
               return launch_each(h,
                   [&] {
                     return gc::launch_ens_score(s, h->d_ens, field, M, h->d_ens_truth, h->d_ens_w, G, B, c.c_out, h->d_ens_part,
                                                 h->d_ens_hpart, ipart, want_fields ? h->d_ens_mean : nullptr,
                                                 want_fields ? h->d_ens_var : nullptr);
                   },
                   [&] { return gc::launch_ens_finish(s, h->d_ens_part, h->d_ens_hpart, ipart, blocks, W, M, h->d_ens_sums, h->d_ens_hist); });
             },
             [&]() -> int {
               if (want_fields) h->has_ens_fields = true;      // (enqueued: a download on this stream finds them)
               if ((rc = read_back(h, sums, h->d_ens_sums, (size_t)6 * W)) || (rc = read_back(h, hist.data(), h->d_ens_hist, hist.size())))
                 return rc;
               return GC_OK;
             });
  if (rc) return rc;
  h->ens.invalid = (int64_t)hist.back();
  h->ens.blocks = blocks;
  if (rank_hist)
    for (size_t i = 0; i + 1 < hist.size(); ++i) rank_hist[i] = hist[i];
  return GC_OK;
  });
}

int gc_ens_download_fields(gc_handle* h, float* mean, float* variance) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ens_ready(h, true);
  if (rc) return rc;
  if (!h->has_ens_fields) return fail(h, GC_ERR_STATE, "no mean / variance fields on the device (gc_ens_score with want_fields)");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t bytes = field_len(h) * sizeof(float);
  if (mean) GC_HIP(h, hipMemcpyAsync(mean, h->d_ens_mean, bytes, hipMemcpyDeviceToHost, h->stream));
  if (variance) GC_HIP(h, hipMemcpyAsync(variance, h->d_ens_var, bytes, hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
  });
}

int gc_ens_push_state(gc_handle* h, int32_t slot, gc_handle* src, const int32_t* state_src) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ens_ready(h, true);
  if (rc || (rc = ens_slot(h, slot))) return rc;
  if (!state_src) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (!src) src = h;
  const gc_config& c = h->cfg;
  if ((rc = push_source(h, src, true))) return rc;
  if (!src->has_cond) return fail(h, GC_ERR_STATE, "no conditioning on the source handle (gc_upload_cond)");
  for (int j = 0; j < c.c_out; ++j) {
    if (state_src[j] >= c.c_in) return fail(h, GC_ERR_INVALID_ARGUMENT, "state_src: conditioning channel out of range");
    if (state_src[j] >= 0 && std::find(src->h_slots.begin(), src->h_slots.end(), state_src[j]) != src->h_slots.end())
      return fail(h, GC_ERR_INVALID_ARGUMENT, "state_src: a noisy slot holds no state");
  }
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = relay(h, src, resolve_guard(src), "source"))) return rc;   // the state comes from the CHECKED sample
  if (h->ens_state_src.size() != (size_t)c.c_out || !std::equal(state_src, state_src + c.c_out, h->ens_state_src.begin())) {
    // every earlier gather is ordered into this stream (ev_ens_done): after the wait none reads the old table
    GC_HIP(h, hipStreamSynchronize(h->stream));
    GC_HIP(h, hipMemcpyAsync(h->d_ens_state_src, state_src, c.c_out * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    GC_HIP(h, hipStreamSynchronize(h->stream));      // `state_src` is the caller's again, and every stream sees the table
    h->ens_state_src.assign(state_src, state_src + c.c_out);
  }
  float* const dst = h->d_ens + (size_t)slot * field_len(h);
  // on the SOURCE's stream, as the copy of gc_ens_push
  auto gather = [&] {
    return relay(h, src, launch(src, gc::KC_PACK, [&] {
      return gc::launch_ens_state(src->stream, src->d_feats, src->d_sx, h->d_ens_state_src, h->hg.G, c.batch, c.c_in, c.c_out, dst);
    }), "source");
  };
  if ((rc = src == h ? gather() : on_peer_stream(h, src, gather))) return rc;
  h->ens_filled[(size_t)slot] = 1;
  return GC_OK;
  });
}

int gc_ens_download_member(gc_handle* h, int32_t slot, float* out) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ens_ready(h, true);
  if (rc || (rc = ens_slot(h, slot))) return rc;
  if (!out) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->ens_filled[(size_t)slot]) return fail(h, GC_ERR_STATE, "member slot " + std::to_string(slot) + " has not been pushed");
  GC_HIP(h, hipSetDevice(h->device));
  // (every push, whichever stream made it, is ordered into this one)
  GC_HIP(h, hipMemcpyAsync(out, h->d_ens + (size_t)slot * field_len(h), field_len(h) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
  });
}

// ---- context store (include/gencast_hip.h, gc_ctx_*) ------------------------------------------------------------------
// A slot is written and read on the stream of whichever handle's conditioning is copied, so a copy lies in stream order
// with that handle's samples and context updates and waits for nothing else.  Order between streams is per slot: ev_w
// is recorded behind the last write, ev_r behind the last read; a write waits for both, a read for the write and (so
// that ev_r stands for ALL earlier reads) for the read before it.  The host never waits for a copy.

int gc_ctx_reserve(gc_handle* h, int32_t n) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (n < 1 || n > 64) return fail(h, GC_ERR_UNSUPPORTED, "n must be in 1..64");
  GC_HIP(h, hipSetDevice(h->device));
  for (gc_handle::CtxSlot& c : h->ctx) {             // no copy into or out of the old store is still running
    if (c.saved) GC_HIP(h, hipEventSynchronize(c.ev_w));
    if (c.read) GC_HIP(h, hipEventSynchronize(c.ev_r));
    c.saved = c.read = false;
  }
  h->ctx_allocs.free();
  h->ctx_slots = 0;
  h->d_ctx = nullptr;
  int rc;
  if ((rc = dev_alloc(h, &h->d_ctx, (size_t)n * cond_len(h), &h->ctx_allocs))) return rc;
  if (h->ctx.size() < (size_t)n) h->ctx.resize((size_t)n);
  for (int i = 0; i < n; ++i)
    for (hipEvent_t* e : {&h->ctx[(size_t)i].ev_w, &h->ctx[(size_t)i].ev_r})
      if (!*e) GC_HIP(h, hipEventCreateWithFlags(e, hipEventDisableTiming));
  h->ctx_slots = n;
  return GC_OK;
  });
}

int gc_ctx_save(gc_handle* h, int32_t slot, gc_handle* src) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ctx_ready(h, slot);
  if (rc) return rc;
  if (!src) src = h;
  if ((rc = ctx_peer(h, src))) return rc;
  if (!src->has_cond) return fail(h, GC_ERR_STATE, "no conditioning on the source handle (gc_upload_cond)");
  GC_HIP(h, hipSetDevice(h->device));
  if (src->guard_pending && (rc = relay(h, src, resolve_guard(src), "source"))) return rc;
  gc_handle::CtxSlot& c = h->ctx[(size_t)slot];
  if (c.saved) GC_HIP(h, hipStreamWaitEvent(src->stream, c.ev_w, 0));
  if (c.read) GC_HIP(h, hipStreamWaitEvent(src->stream, c.ev_r, 0));
  GC_HIP(h, hipMemcpyAsync(h->d_ctx + (size_t)slot * cond_len(h), src->d_feats, cond_len(h) * sizeof(float),
                           hipMemcpyDeviceToDevice, src->stream));
  GC_HIP(h, hipEventRecord(c.ev_w, src->stream));
  c.saved = true;
  c.read = false;                                    // (this write waited for the reads: ev_w now stands for them too)
  return GC_OK;
  });
}

int gc_ctx_load(gc_handle* h, int32_t slot, gc_handle* dst) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ctx_ready(h, slot);
  if (rc) return rc;
  if (!dst) dst = h;
  if ((rc = ctx_peer(h, dst))) return rc;
  gc_handle::CtxSlot& c = h->ctx[(size_t)slot];
  if (!c.saved) return fail(h, GC_ERR_STATE, "context slot " + std::to_string(slot) + " has not been saved");
  GC_HIP(h, hipSetDevice(h->device));
  // a pending re-run needs the conditioning it sampled with (gc_upload_cond_dev)
  if (dst->guard_pending && (rc = relay(h, dst, resolve_guard(dst), "destination"))) return rc;
  GC_HIP(h, hipStreamWaitEvent(dst->stream, c.ev_w, 0));
  if (c.read) GC_HIP(h, hipStreamWaitEvent(dst->stream, c.ev_r, 0));
  GC_HIP(h, hipMemcpyAsync(dst->d_feats, h->d_ctx + (size_t)slot * cond_len(h), cond_len(h) * sizeof(float),
                           hipMemcpyDeviceToDevice, dst->stream));
  GC_HIP(h, hipEventRecord(c.ev_r, dst->stream));
  c.read = true;
  return relay(h, dst, gc_commit_cond(dst), "destination");
  });
}

int gc_ctx_download(gc_handle* h, int32_t slot, float* out) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ctx_ready(h, slot);
  if (rc) return rc;
  if (!out) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  gc_handle::CtxSlot& c = h->ctx[(size_t)slot];
  if (!c.saved) return fail(h, GC_ERR_STATE, "context slot " + std::to_string(slot) + " has not been saved");
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, hipStreamWaitEvent(h->stream, c.ev_w, 0));
  GC_HIP(h, hipMemcpyAsync(out, h->d_ctx + (size_t)slot * cond_len(h), cond_len(h) * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));        // (complete on return: no read event to leave behind)
  return GC_OK;
  });
}

}  // extern "C"
