// An ensemble scored against a climatology on the device (include/gencast_hip.h, gc_ens_clim_score): one pass that reads
// TWO member stores -- the M members of handle h and the K climatological samples of a second, graph-only handle -- and
// forms the raw sums of the anomaly correlation of the ensemble mean and of the CRPS skill score against the
// climatological ensemble.  Kernels and their host code live together here; DESIGN.md section 8i has the definitions and
// the error bound the tests assert.
//
// Per point (g, b, c), from the float32 members x_0 .. x_{M-1}, the samples c_0 .. c_{K-1} and the truth y, in double:
//   m    = (sum_i x_i) / M                     ascending slot order: the m of gc_ens_score
//   cbar = (sum_j c_j) / K                     ascending slot order
//   fa = m - cbar,  oa = y - cbar
//   ae_x = (sum_i |x_i - y|) / M               ae_c = (sum_j |c_j - y|) / K
//   d_x  = sum_{k=1}^{M-1} k (M - k) (x_(k+1) - x_(k)) / (M (M - 1) / 2)     x_(1) <= .. <= x_(M): the members sorted
//   d_c  the same over the sorted samples      (= the mean of |x_i - x_j| over the pairs; every term is >= 0)
//   q_x  = (sum_i (x_i - cbar)^2) / M          ascending slot order
// A point counts when y, all M members and all K samples are finite.  Per column (b, c), over the counted nodes, w = node
// weight of h, the twelve sums in the order they are returned:
//   A0 = sum w        A1 = sum w fa      A2 = sum w oa     A3 = sum w fa oa    A4 = sum w fa^2    A5 = sum w oa^2
//   A6 = sum w q_x    A7 = sum w (m - y)^2                 F4 = sum w ae_x     F5 = sum w d_x
//   C4 = sum w ae_c   C5 = sum w d_c
// No atomics on floats: every accumulator has one writer and every sum a fixed order (a thread's nodes ascending, the
// node lanes of a column in lane order, the blocks in index order), so the same call twice returns identical bytes.
#include "gc_colsum.h"
#include "gc_sort.h"
#include "gc_store.h"

// the per-point arithmetic is the definition above, operation for operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace gc {

constexpr int kClimSums = 12;

// the mean absolute difference of the n <= P values of v over their n (n - 1) / 2 pairs, times that number of pairs: v is
// padded with +inf beyond n and sorted here; the gaps are guarded on n, so no padding enters a difference
template <int P>
__device__ inline double clim_gap_sum(float (&v)[P], int n) {
  ord_sort<P>(v);
  double d = 0.0;
#pragma unroll
  for (int k = 1; k < P; ++k)
    if (k < n) d += (double)(k * (n - k)) * ((double)v[k] - (double)v[k - 1]);
  return d;
}

// The pass, on the 256-wide cut of gc_colsum.h.  Per point the K samples are read once from HBM into P padded registers
// (load_padded); their slot-order sums are formed while loading, then they are sorted for d_c.  The M members follow into
// the SAME registers: cbar is known by then, so q_x is formed while loading as well.  A point with a non-finite value
// never enters the network.
// Out, as plain stores: part[block x][12][W] (double), cpart[block x][W] (counted points), ipart[block x][tile] (skipped).
template <int P>
__global__ __launch_bounds__(256) void gc_ens_clim_kernel(const float* __restrict__ mem, int M,
                                                           const float* __restrict__ clim, int K, size_t field,
                                                           const float* __restrict__ truth,
                                                           const float* __restrict__ node_w, int G, int W, int per,
                                                           double* __restrict__ part, unsigned* __restrict__ cpart,
                                                           unsigned* __restrict__ ipart) {
  __shared__ double lane_sum[256];
  __shared__ unsigned lane_cnt[256];
  __shared__ unsigned skipped;
  const ColTile ct(256, 256, W, blockIdx.y);
  const int tid = threadIdx.x, col = ct.col;
  if (tid == 0) skipped = 0u;
  __syncthreads();
  double s[kClimSums];
#pragma unroll
  for (int k = 0; k < kClimSums; ++k) s[k] = 0.0;
  unsigned cnt = 0, inv = 0;
  if (ct.active()) {
    const double dM = (double)M, dK = (double)K;
    const double pairs_x = 0.5 * dM * (dM - 1.0), pairs_c = 0.5 * dK * (dK - 1.0);
    const int n_end = ct.n_end(G, per);
    for (int n = ct.n_begin(per); n < n_end; n += ct.q) {
      const size_t i = (size_t)n * W + col;
      const float y = truth[i];
      const double yd = (double)y;
      float v[P];
      double csum = 0.0, ae_c = 0.0;
      const bool cfin = load_padded<P>(v, clim, field, i, K, [&](float c) {
        csum += (double)c;
        ae_c += fabs((double)c - yd);
      });
      if (!(cfin && isfinite(y))) {                // (the members are not looked at: the point adds to `invalid` alone)
        ++inv;
        continue;
      }
      const double cbar = csum / dK;
      const double d_c = clim_gap_sum<P>(v, K) / pairs_c;
      double sum = 0.0, ae_x = 0.0, q_x = 0.0;
      const bool xfin = load_padded<P>(v, mem, field, i, M, [&](float x) {
        sum += (double)x;
        ae_x += fabs((double)x - yd);
        const double dx = (double)x - cbar;
        q_x += dx * dx;
      });
      if (!xfin) {
        ++inv;
        continue;
      }
      const double d_x = clim_gap_sum<P>(v, M) / pairs_x;
      const double m = sum / dM;
      const double fa = m - cbar, oa = yd - cbar, e = m - yd;
      const double w = (double)node_w[n];
      s[0] += w;
      s[1] += w * fa;
      s[2] += w * oa;
      s[3] += w * (fa * oa);
      s[4] += w * (fa * fa);
      s[5] += w * (oa * oa);
      s[6] += w * (q_x / dM);
      s[7] += w * (e * e);
      s[8] += w * (ae_x / dM);
      s[9] += w * d_x;
      s[10] += w * (ae_c / dK);
      s[11] += w * d_c;
      ++cnt;
    }
  }
  if (inv) atomicAdd(&skipped, inv);               // (an integer: the order of these does not show)
#pragma unroll
  for (int k = 0; k < kClimSums; ++k) {
    const double t = col_total(lane_sum, s[k], ct);
    if (tid < ct.wt) part[((size_t)blockIdx.x * kClimSums + k) * W + col] = t;
  }
  const unsigned t = col_total(lane_cnt, cnt, ct);
  if (tid < ct.wt) cpart[(size_t)blockIdx.x * W + col] = t;
  if (tid == 0) ipart[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = skipped;
}

// The ascending block finish: e < 12 W: sum j = e / W of column e % W, as the partials lie -> out [W][12]; then W counts
// -> outc [W]; the skipped points -> outc[W].
struct ClimFinishMap {
  const double* part;
  const unsigned* cpart;
  int W;
  SkippedSum skipped;
  __host__ __device__ int sums() const { return kClimSums * W; }
  __host__ __device__ int counts() const { return W; }
  __device__ BlockSum<double> sum(int e) const {
    const int j = e / W, col = e - j * W;
    return {part + e, (size_t)kClimSums * W, (size_t)col * kClimSums + j};
  }
  __device__ BlockSum<unsigned> count(int col) const { return {cpart + col, (size_t)W, (size_t)col}; }
};

// ONE padded size for both samples, that of max(M, K): six instantiations
static hipError_t launch_ens_clim(hipStream_t s, const float* mem, int M, const float* clim, int K, size_t field,
                                  const float* truth, const float* node_w, int G, int B, int c_out, double* part,
                                  unsigned* cpart, unsigned* ipart) {
  const int W = B * c_out;
  const int blocks = loss_reduce_blocks(G, B, c_out);
  const int per = (G + blocks - 1) / blocks;
  const dim3 grid(blocks, (W + 255) / 256);
  return pad_dispatch(std::max(M, K), [&](auto p) {
    hipLaunchKernelGGL((gc_ens_clim_kernel<decltype(p)::value>), grid, dim3(256), 0, s, mem, M, clim, K, field, truth, node_w, G, W, per, part,
                       cpart, ipart);
    return hipGetLastError();
  });
}

static hipError_t launch_ens_clim_finish(hipStream_t s, const double* part, const unsigned* cpart, const unsigned* ipart,
                                         int blocks, int tiles, int W, double* out, unsigned long long* outc) {
  return launch_block_finish(s, ClimFinishMap{part, cpart, W, {ipart, tiles, (size_t)W}}, blocks, out, outc);
}

}  // namespace gc

using namespace gci;

extern "C" {

int gc_ens_clim_score(gc_handle* h, gc_handle* clim, const float* truth, double* sums, uint64_t* counts, uint64_t* invalid) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!clim || clim == h) return fail(h, GC_ERR_INVALID_ARGUMENT, "the climatology must be another handle");
  int rc;
  if ((rc = need_out(h, sums)) || (rc = need_graph(h)) || (rc = check_peer(h, clim, "climatology", false, h->cfg.c_out)) ||
      (rc = need_store(h)) || (rc = need(h, clim->ens_members != 0, "no member store on the climatology handle (gc_ens_reserve)")) ||
      (rc = store_complete(h, h)) || (rc = store_complete(h, clim, "climatology ")) || (rc = need_weights(h)))
    return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_clim_score"))) return rc;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, B = c.batch, W = B * c.c_out, M = h->ens_members, K = clim->ens_members;
  const int blocks = gc::loss_reduce_blocks(G, B, c.c_out), tiles = (W + 255) / 256;
  if (!h->d_clim_part) {                             // sized by G, B and c_out alone: made once
    if ((rc = alloc_all(h, h->clim_allocs, buf(&h->d_clim_part, (size_t)blocks * gc::kClimSums * W),
                        buf(&h->d_clim_cpart, (size_t)blocks * W + (size_t)blocks * tiles),
                        buf(&h->d_clim_out, (size_t)gc::kClimSums * W), buf(&h->d_clim_outc, (size_t)W + 1)))) {
      h->d_clim_part = nullptr;
      return rc;
    }
    GC_HIP(h, h->ev_clim_src.ensure());
  }
  hipStream_t s = h->stream;
  // the climatology's store is complete on ITS stream: this handle's stream goes on behind it
  if ((rc = order_behind(h, h->ev_clim_src, clim->stream, s))) return rc;
  unsigned* const ipart = h->d_clim_cpart + (size_t)blocks * W;
  std::vector<uint64_t> cnt((size_t)W + 1);
  // (on return the pass has read the climatology's store: it may be pushed into again)
  rc = timed(h, h->clim,
             [&] {
               return launch_each(h,
                   [&] {
                     return gc::launch_ens_clim(s, h->d_ens, M, clim->d_ens, K, field_len(h), h->d_ens_truth, h->d_ens_w, G, B, c.c_out,
                                                h->d_clim_part, h->d_clim_cpart, ipart);
                   },
                   [&] {
                     return gc::launch_ens_clim_finish(s, h->d_clim_part, h->d_clim_cpart, ipart, blocks, tiles, W, h->d_clim_out,
                                                       h->d_clim_outc);
                   });
             },
             [&]() -> int {
               if ((rc = read_back(h, sums, h->d_clim_out, (size_t)gc::kClimSums * W)) || (rc = read_back(h, cnt.data(), h->d_clim_outc, cnt.size())))
                 return rc;
               return GC_OK;
             });
  if (rc) return rc;
  h->clim.invalid = (int64_t)cnt.back();
  h->clim.blocks = blocks;
  if (counts)
    for (size_t i = 0; i + 1 < cnt.size(); ++i) counts[i] = cnt[i];
  if (invalid) invalid[0] = cnt.back();
  return GC_OK;
  });
}

}  // extern "C"
