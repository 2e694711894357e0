// Ensemble order statistics on the device (include/gencast_hip.h, gc_ens_order_*): the M members of every point of the
// gc_ens_* store in ascending order, and what follows from that order -- quantile fields (the median, a p10 / p90 band)
// and the bin sums of Hersbach's (2000) decomposition of the ensemble CRPS into a reliability and a potential part.
// Kernels and their host code live together here; DESIGN.md section 8h has the definitions and the error bound.
//
// Per point (g, b, c), x_(1) <= .. <= x_(M) the float32 members in ascending order, y the truth, in double:
//   Q_q     = (float)(x_(lo+1) + f (x_(hi+1) - x_(lo+1)))      lo, hi, f formed on the HOST from p_q and M (NumPy "linear")
//   alpha_k = c - x_(k),  beta_k = x_(k+1) - c,  c = min(max(y, x_(k)), x_(k+1))        0 < k < M
//   alpha_0 = 0, beta_0 = max(x_(1) - y, 0);    alpha_M = max(y - x_(M), 0), beta_M = 0
// Q_q exists where all M members are finite (else NaN); a point counts when they and y are finite.  Per column (b, c),
// over the counted nodes, w = node weight:
//   bins[k] = (sum w alpha_k, sum w beta_k)    extra = (sum w, sum w [y < x_(1)], sum w [y > x_(M)])
//   pinball[q] = sum w u (p_q - [u < 0]), u = y - Q_q          counts[q] = #{y < Q_q}, counts[Q] = counted points
// No atomics on floats: every accumulator has one writer and every sum a fixed order (a thread's nodes ascending, the
// node lanes of a column in lane order, the blocks in index order), so the same call twice returns identical bytes.
#include "gc_colsum.h"
#include "gc_sort.h"
#include "gc_store.h"

// the per-point arithmetic is the definition above, operation for operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace gc {

constexpr int kOrdMaxQuantiles = 8;
constexpr size_t kOrdLds = 144 * 1024;           // accumulators of a workgroup (a CU has 160 KB)
constexpr int kOrdCuCount = 256;

// what the host made of the probabilities for the current M (by value in the kernel arguments: wave-uniform)
struct OrdPlan {
  int Q;
  int lo[kOrdMaxQuantiles], hi[kOrdMaxQuantiles];
  double f[kOrdMaxQuantiles], p[kOrdMaxQuantiles];
};

// accumulators of one thread: 2 (M + 1) bin sums, 3 extra, Q pinball (double), then Q + 1 counts (unsigned)
static int ord_nacc(int M, int Q) { return 2 * (M + 1) + 3 + Q; }
static size_t ord_thread_bytes(int M, int Q) { return (size_t)ord_nacc(M, Q) * sizeof(double) + (size_t)(Q + 1) * sizeof(unsigned); }
// threads of a workgroup that get an accumulator set (the others idle), column tiles of equal width within them
static int ord_cap(int M, int Q) { return (int)std::min<size_t>(256, kOrdLds / ord_thread_bytes(M, Q)); }
static int ord_tiles(int W, int cap) { return (W + cap - 1) / cap; }
static int ord_tile_width(int W, int cap) { const int t = ord_tiles(W, cap); return (W + t - 1) / t; }
// node-range blocks: at most 1024 and two rounds of the workgroups the LDS lets a CU hold
static int ord_blocks(int G, int W, int M, int Q) {
  const int cap = ord_cap(M, Q), q = cap / ord_tile_width(W, cap);
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / ((size_t)cap * ord_thread_bytes(M, Q))));
  return node_blocks(G, q, std::min(1024, 2 * kOrdCuCount * per_cu));
}
// ... of the field pass, which holds no accumulators: those of a pass over one 256-wide column tile
static int ord_field_blocks(int G, int W) { return loss_reduce_blocks(G, 1, std::min(256, W)); }

// v[idx] for a wave-uniform idx in [0, P): a tree of selects on the bits of idx, lowest first, over compile-time
// indices -- P - 1 selects on log2 P conditions, and the array stays in registers
template <int P>
__device__ inline float ord_pick(const float (&v)[P], int idx) {
  float t[P];
#pragma unroll
  for (int i = 0; i < P; ++i) t[i] = v[i];
#pragma unroll
  for (int lvl = 0; lvl < OrdLog<P>::value; ++lvl) {
    const bool odd = ((idx >> lvl) & 1) != 0;
#pragma unroll
    for (int i = 0; i < (P >> (lvl + 1)); ++i) {
      const float a = t[2 * i], b = t[2 * i + 1];
      t[i] = odd ? b : a;
    }
  }
  return t[0];
}

// The pass, on equal-width column tiles of tile_w <= cap columns (gc_colsum.h; cap < 256 where the LDS holds fewer
// accumulator sets).  The M values of a point are read once from HBM into P padded registers (load_padded) and sorted
// there.  SCORE = false: the quantile fields only -- no truth, no weights, no LDS.
// Dynamic LDS (SCORE): double acc[nacc][cap], then unsigned cnt[Q + 1][cap]; accumulator j of thread t at [j][t], so the
// threads of a wave touch consecutive words.
// Out, as plain stores: qf [Q][field]; part[block x][nacc][W] (double), cpart[block x][Q + 1][W], ipart[block x][tile].
template <int P, bool SCORE>
__global__ __launch_bounds__(256) void gc_ens_order_kernel(const float* __restrict__ mem, size_t field, int M,
                                                            const float* __restrict__ truth,
                                                            const float* __restrict__ node_w, int G, int W, int per,
                                                            int cap, int tile_w, const OrdPlan plan,
                                                            float* __restrict__ qf, double* __restrict__ part,
                                                            unsigned* __restrict__ cpart, unsigned* __restrict__ ipart) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ord_lds[];
  __shared__ unsigned skipped;
  const int Q = plan.Q;
  const int nacc = 2 * (M + 1) + 3 + Q;
  double* const acc = reinterpret_cast<double*>(ord_lds);
  unsigned* const cnt = reinterpret_cast<unsigned*>(acc + (size_t)nacc * cap);
  const ColTile ct(tile_w, cap, W, blockIdx.y);
  const int col0 = ct.col0, wt = ct.wt, q = ct.q;
  const int tid = threadIdx.x;
  if constexpr (SCORE) {
    for (int i = tid; i < nacc * cap; i += 256) acc[i] = 0.0;
    for (int i = tid; i < (Q + 1) * cap; i += 256) cnt[i] = 0u;
    if (tid == 0) skipped = 0u;
    __syncthreads();
  }
  unsigned inv = 0;
  if (ct.active()) {
    double* const my = acc + tid;                  // accumulator j at my[j * cap]
    unsigned* const myc = cnt + tid;
    const int n_end = ct.n_end(G, per);
    for (int n = ct.n_begin(per); n < n_end; n += q) {
      const size_t i = (size_t)n * W + ct.col;
      float v[P];
      const bool xfin = load_padded<P>(v, mem, field, i, M);
      float qv[kOrdMaxQuantiles];
      if (xfin) {                                  // the network never sees a NaN
        ord_sort<P>(v);
#pragma unroll
        for (int j = 0; j < kOrdMaxQuantiles; ++j) {
          qv[j] = 0.f;
          if (j < Q) {
            const double a = (double)ord_pick<P>(v, plan.lo[j]), b = (double)ord_pick<P>(v, plan.hi[j]);
            qv[j] = (float)(a + plan.f[j] * (b - a));
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kOrdMaxQuantiles; ++j)
        if (j < Q) qf[(size_t)j * field + i] = xfin ? qv[j] : __builtin_nanf("");
      if constexpr (SCORE) {
        const float y = truth[i];
        if (!(xfin && isfinite(y))) {
          ++inv;
          continue;
        }
        const double w = (double)node_w[n], yd = (double)y;
        // bins: k = 0 and k = M are the unbounded ends, the others differences of finite values (guarded on M, not on P)
        my[(size_t)1 * cap] += w * fmax((double)v[0] - yd, 0.0);
#pragma unroll
        for (int k = 1; k <= P; ++k) {
          if (k <= M) {
            const bool last = k == M;
            const float xl = v[k - 1], xr = v[k < P ? k : P - 1];
            const float c = last ? fmaxf(y, xl) : fminf(fmaxf(y, xl), xr);
            my[(size_t)(2 * k) * cap] += w * ((double)c - (double)xl);
            if (!last) my[(size_t)(2 * k + 1) * cap] += w * ((double)xr - (double)c);
          }
        }
        const float top = ord_pick<P>(v, M - 1);
        double* const ex = my + (size_t)(2 * (M + 1)) * cap;
        ex[0] += w;
        ex[(size_t)cap] += w * (y < v[0] ? 1.0 : 0.0);
        ex[(size_t)2 * cap] += w * (y > top ? 1.0 : 0.0);
        double* const pin = ex + (size_t)3 * cap;
#pragma unroll
        for (int j = 0; j < kOrdMaxQuantiles; ++j) {
          if (j < Q) {
            const double u = yd - (double)qv[j];
            pin[(size_t)j * cap] += w * (u * (plan.p[j] - (u < 0.0 ? 1.0 : 0.0)));
            myc[(size_t)j * cap] += y < qv[j] ? 1u : 0u;
          }
        }
        myc[(size_t)Q * cap] += 1u;
      }
    }
  }
  if constexpr (SCORE) {
    if (inv) atomicAdd(&skipped, inv);
    __syncthreads();
    // the lane fold, in place on the accumulator rows
    for (int e = tid; e < nacc * wt; e += 256) {
      const int j = e / wt, c = e - j * wt;
      part[((size_t)blockIdx.x * nacc + j) * W + col0 + c] = lane_fold(acc + (size_t)j * cap, c, wt, q);
    }
    for (int e = tid; e < (Q + 1) * wt; e += 256) {
      const int j = e / wt, c = e - j * wt;
      cpart[((size_t)blockIdx.x * (Q + 1) + j) * W + col0 + c] = lane_fold(cnt + (size_t)j * cap, c, wt, q);
    }
    if (tid == 0) ipart[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = skipped;
  }
}

// The ascending block finish: e < nacc W: double sum j = e / W of column e % W, as the partials lie, stored where the
// result arrays want it -- out = bins [W][M + 1][2], extra [W][3], pinball [W][Q]; then (Q + 1) W counts -> outc
// [W][Q + 1]; the skipped points -> outc[W (Q + 1)].
struct OrdFinishMap {
  const double* part;
  const unsigned* cpart;
  int W, M, Q;
  SkippedSum skipped;
  __host__ __device__ int sums() const { return (2 * (M + 1) + 3 + Q) * W; }
  __host__ __device__ int counts() const { return (Q + 1) * W; }
  __device__ BlockSum<double> sum(int e) const {
    const int j = e / W, col = e - j * W;
    const int nb = 2 * (M + 1);
    size_t at;
    if (j < nb) at = (size_t)col * nb + j;
    else if (j < nb + 3) at = (size_t)W * nb + (size_t)col * 3 + (j - nb);
    else at = (size_t)W * (nb + 3) + (size_t)col * Q + (j - nb - 3);
    return {part + e, (size_t)sums(), at};
  }
  __device__ BlockSum<unsigned> count(int e) const {
    const int j = e / W, col = e - j * W;
    return {cpart + e, (size_t)counts(), (size_t)col * (Q + 1) + j};
  }
};

template <int P, bool SCORE>
static hipError_t ord_launch(hipStream_t s, dim3 grid, size_t lds, const float* mem, size_t field, int M, const float* truth,
                             const float* node_w, int G, int W, int per, int cap, int tile_w, const OrdPlan& plan, float* qf,
                             double* part, unsigned* cpart, unsigned* ipart) {
  if (lds > 64 * 1024) {                           // (a per-device property of the kernel; setting it again is harmless)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gc_ens_order_kernel<P, SCORE>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((gc_ens_order_kernel<P, SCORE>), grid, dim3(256), lds, s, mem, field, M, truth, node_w, G, W, per, cap,
                     tile_w, plan, qf, part, cpart, ipart);
  return hipGetLastError();
}

// score: truth, node_w and the partial buffers; else the quantile fields only
static hipError_t launch_ens_order(hipStream_t s, bool score, const float* mem, size_t field, int M, const float* truth,
                                   const float* node_w, int G, int W, const OrdPlan& plan, float* qf, double* part,
                                   unsigned* cpart, unsigned* ipart) {
  const int Q = plan.Q;
  const int cap = score ? ord_cap(M, Q) : 256;
  const int tiles = ord_tiles(W, cap), tile_w = ord_tile_width(W, cap);
  const int blocks = score ? ord_blocks(G, W, M, Q) : ord_field_blocks(G, W);
  const int per = (G + blocks - 1) / blocks;
  const size_t lds = score ? (size_t)cap * ord_thread_bytes(M, Q) : 0;
  const dim3 grid(blocks, tiles);
  return pad_dispatch(M, [&](auto p) {
    constexpr int P = decltype(p)::value;
    return score ? ord_launch<P, true>(s, grid, lds, mem, field, M, truth, node_w, G, W, per, cap, tile_w, plan, qf, part, cpart,
                                       ipart)
                 : ord_launch<P, false>(s, grid, lds, mem, field, M, truth, node_w, G, W, per, cap, tile_w, plan, qf, part, cpart,
                                        ipart);
  });
}

static hipError_t launch_ens_order_finish(hipStream_t s, const double* part, const unsigned* cpart, const unsigned* ipart,
                                          int blocks, int tiles, int W, int M, int Q, double* out, unsigned long long* outc) {
  return launch_block_finish(s, OrdFinishMap{part, cpart, W, M, Q, {ipart, tiles, (size_t)W * (Q + 1)}}, blocks, out, outc);
}

}  // namespace gc

using namespace gci;

namespace {

// validation shared by the two passes: a graph, a setting, a complete store
int ord_ready(gc_handle* h) {
  int rc;
  if ((rc = need_graph(h)) || (rc = need(h, h->ord_set, "no probabilities (gc_ens_order_set)")) || (rc = need_store(h))) return rc;
  return store_complete(h, h);
}

// lo, hi and f of every probability for the current M, all in double (NumPy's "linear" rule)
gc::OrdPlan ord_plan(const gc_handle* h) {
  gc::OrdPlan p{};
  const int M = h->ens_members;
  p.Q = h->ord_Q;
  for (int q = 0; q < p.Q; ++q) {
    const double pos = h->ord_p[q] * (double)(M - 1);
    const int lo = std::min((int)std::floor(pos), M - 1);
    p.lo[q] = lo;
    p.hi[q] = std::min(lo + 1, M - 1);
    p.f[q] = pos - (double)lo;
    p.p[q] = h->ord_p[q];
  }
  return p;
}

}  // namespace

extern "C" {

int gc_ens_order_set(gc_handle* h, int32_t n_quantiles, const double* probs) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (n_quantiles < 0 || n_quantiles > gc::kOrdMaxQuantiles) return fail(h, GC_ERR_UNSUPPORTED, "n_quantiles must be in 0..8");
  if (n_quantiles > 0 && !probs) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  for (int q = 0; q < n_quantiles; ++q)
    if (!(probs[q] >= 0.0 && probs[q] <= 1.0))
      return fail(h, GC_ERR_INVALID_ARGUMENT, "probability " + std::to_string(q) + " is not in [0, 1]");
  GC_HIP(h, hipSetDevice(h->device));
  const int Q = n_quantiles;
  h->ord_ready = false;
  if (!h->ord_set || Q != h->ord_Q) {
    GC_HIP(h, h->ord_allocs.drop(h->stream));        // nothing reads the old fields any more
    h->ord_set = false;
    h->d_ord_q = nullptr;
    int rc;
    if ((rc = dev_alloc(h, &h->d_ord_q, (size_t)Q * field_len(h), &h->ord_allocs))) return rc;
  }
  for (int q = 0; q < Q; ++q) h->ord_p[q] = probs[q];
  h->ord_Q = Q;
  h->ord_set = true;
  return GC_OK;
  });
}

int gc_ens_order_fields(gc_handle* h) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ord_ready(h);
  if (rc) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  const gc_config& c = h->cfg;
  const int G = h->hg.G, W = c.batch * c.c_out, M = h->ens_members;
  const gc::OrdPlan plan = ord_plan(h);
  hipStream_t s = h->stream;
  rc = timed(h, h->ord,
             [&] {
               return launch_each(h, [&] {
                 return gc::launch_ens_order(s, false, h->d_ens, field_len(h), M, nullptr, nullptr, G, W, plan, h->d_ord_q, nullptr,
                                             nullptr, nullptr);
               });
             },
             no_readbacks);
  if (rc) return rc;
  h->ord.blocks = gc::ord_field_blocks(G, W);
  h->ord_ready = true;
  return GC_OK;
  });
}

int gc_ens_order_score(gc_handle* h, const float* truth, double* bins, double* extra, double* pinball, uint64_t* counts,
                       uint64_t* invalid) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = ord_ready(h);
  if (rc) return rc;
  if ((rc = need_out(h, bins && extra)) || (rc = need_weights(h))) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_order_score"))) return rc;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, W = c.batch * c.c_out, M = h->ens_members, Q = h->ord_Q;
  const int nacc = gc::ord_nacc(M, Q);
  const int blocks = gc::ord_blocks(G, W, M, Q), tiles = gc::ord_tiles(W, gc::ord_cap(M, Q));
  const size_t n_out = (size_t)nacc * W, n_outc = (size_t)(Q + 1) * W + 1;
  if ((rc = sized_for(h, h->ord_work_allocs, {(size_t)M, (size_t)Q}, buf(&h->d_ord_part, (size_t)blocks * n_out),
                      buf(&h->d_ord_cpart, (size_t)blocks * (Q + 1) * W + (size_t)blocks * tiles), buf(&h->d_ord_out, n_out),
                      buf(&h->d_ord_outc, n_outc))))
    return rc;
  const gc::OrdPlan plan = ord_plan(h);
  hipStream_t s = h->stream;
  unsigned* const ipart = h->d_ord_cpart + (size_t)blocks * (Q + 1) * W;
  const size_t n_bins = (size_t)W * 2 * (M + 1), n_extra = (size_t)W * 3;
  std::vector<uint64_t> cnt(n_outc);
  rc = timed(h, h->ord,
             [&] {
               return launch_each(h,
                   [&] {
                     return gc::launch_ens_order(s, true, h->d_ens, field_len(h), M, h->d_ens_truth, h->d_ens_w, G, W, plan,
                                                 h->d_ord_q, h->d_ord_part, h->d_ord_cpart, ipart);
                   },
                   [&] {
                     return gc::launch_ens_order_finish(s, h->d_ord_part, h->d_ord_cpart, ipart, blocks, tiles, W, M, Q, h->d_ord_out,
                                                        h->d_ord_outc);
                   });
             },
             [&]() -> int {
               const double* const out = h->d_ord_out;
               if ((rc = read_back(h, bins, out, n_bins)) || (rc = read_back(h, extra, out + n_bins, n_extra)) ||
                   (pinball && Q > 0 && (rc = read_back(h, pinball, out + n_bins + n_extra, (size_t)W * Q))) ||
                   (rc = read_back(h, cnt.data(), h->d_ord_outc, n_outc)))
                 return rc;
               return GC_OK;
             });
  if (rc) return rc;
  h->ord.invalid = (int64_t)cnt.back();
  h->ord.blocks = blocks;
  h->ord_ready = true;
  if (counts)
    for (size_t i = 0; i + 1 < cnt.size(); ++i) counts[i] = cnt[i];
  if (invalid) invalid[0] = cnt.back();
  return GC_OK;
  });
}

int gc_ens_order_download(gc_handle* h, int32_t q, float* field) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (!h->ord_set) return fail(h, GC_ERR_STATE, "no probabilities (gc_ens_order_set)");
  if (!field) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (q < 0 || q >= h->ord_Q) return fail(h, GC_ERR_INVALID_ARGUMENT, "q outside [0, n_quantiles)");
  if (!h->ord_ready) return fail(h, GC_ERR_STATE, "no quantile fields on the device (gc_ens_order_score / gc_ens_order_fields)");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t n = field_len(h);
  GC_HIP(h, hipMemcpyAsync(field, h->d_ord_q + (size_t)q * n, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
  });
}

}  // extern "C"
