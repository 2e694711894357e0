// Threshold-weighted CRPS on the device (include/gencast_hip.h, gc_ens_tail_*): how good the forecast distribution of the
// gc_ens_* store is in one tail, for T thresholds from one sort of the members.  Kernels and their host code live together
// here; DESIGN.md section 8l has the definition and the error bound.
//
// Members x_0..x_{M-1} (2 <= M <= 64) and truth y are [G,B,c_out] float32 in the sample layout.  w[g] are the float node
// weights of gc_ens_set_node_weight.  There are T threshold fields thr_t (1 <= T <= 8), each [G,B,c_out] float32, with a
// direction dir_t != 0.  This is the convention of gc_ens_event_set.
// A point counts for threshold t when y, all M members and thr_t are finite there.  A NaN threshold means "not evaluated"
// for that t only.
// Per counted point, with x_(0) <= ... <= x_(M-1) the members in ascending order:
//   v(z) = fmaxf(z, thr_t) when dir_t > 0.  This is the upper tail, weight 1{z >= thr}.
//   v(z) = fminf(z, thr_t) when dir_t < 0.  Both are exact in float32.
//   u_k = v(x_(k)), which is still ascending.
//   AE = sum_{k=0}^{M-1} |(double)u_k - (double)v(y)|, added in ascending k.  ae = AE / M.
//   PD = sum_{k=1}^{M-1} (double)(k (M-k)) ((double)u_k - (double)u_{k-1}), added in ascending k.  d = PD / (M(M-1)/2).
//     This "gap form" equals sum_{i<j} |u_i - u_j|.  Every term is non-negative, so there is no cancellation.
//   o = [y in the event], strict as in section 8f: y > thr_t for dir_t > 0, y < thr_t for dir_t < 0.
// Every operation is a rounded double operation with no contraction.
// Per (t, b, c), over the counted nodes:
//   sums[t][b][c][0..3] = sum w, sum w ae, sum w d, sum w o
//   counts[t][b][c] = counted points (uint64)
//   invalid[t] = points skipped
// All of these are raw and additive over batches and dates.
// No atomics on floats: every accumulator has one writer and every sum a fixed order (a thread's nodes ascending, the
// node lanes of a column in lane order, the blocks in index order), so the same call twice returns identical bytes.
#include "gc_colsum.h"
#include "gc_sort.h"
#include "gc_store.h"

// the per-point arithmetic is the definition above, operation for operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace gc {

constexpr int kTailMaxThresholds = 8;

// column tiles of equal width, at most 256 columns each: a thread keeps its accumulators in registers, so every thread
// of a workgroup may own a column (cap = 256)
static int tail_tiles(int W) { return (W + 255) / 256; }
static int tail_tile_width(int W) { const int t = tail_tiles(W); return (W + t - 1) / t; }
// node-range blocks: at most 1024.  (Two rounds of the workgroups a CU holds would be 1024 or more: the widest instance
// leaves room for two workgroups per CU.)
static int tail_blocks(int G, int W) { return node_blocks(G, 256 / tail_tile_width(W), 1024); }

// The pass.  The thread layout of gc_colsum.h, written out (this kernel keeps its own text: it timed slower on the shared
// pieces), on column tiles of tile_w <= 256 columns: inside a tile of wt columns thread t < q wt owns column t % wt of node lane t / wt, q = 256 / wt lanes; block x walks the contiguous node range
// [x per, (x + 1) per) in steps of q.  The M values of a point are read once from HBM (M loads of stride `field`, each
// coalesced across the wave) into P registers, padded with +inf, and sorted there once; every threshold then costs one
// more coalesced load and O(M) double operations.  Bit t of dir_up: threshold t is the upper tail.
// A thread's 4 T sums and T counts stay in REGISTERS (compile-time bound 8, `if (t < T)`); they pass through LDS only at
// the end, one threshold per round, where the q lanes of a column are added in lane order.
// Out, as plain stores: part [block x][T][4][W] (double), cpart [block x][T][W].
template <int P>
__global__ __launch_bounds__(256) void gc_ens_tail_kernel(const float* __restrict__ mem, size_t field, int M,
                                                           const float* __restrict__ truth,
                                                           const float* __restrict__ node_w,
                                                           const float* __restrict__ thr, int T, unsigned dir_up, int G,
                                                           int W, int per, int tile_w, double* __restrict__ part,
                                                           unsigned* __restrict__ cpart) {
  __shared__ double red[4][256];
  __shared__ unsigned redc[256];
  const int col0 = blockIdx.y * tile_w;
  const int wt = min(tile_w, W - col0);
  const int q = 256 / wt;
  const int tid = threadIdx.x;
  const int lane = tid / wt;
  const int cl = tid - lane * wt;
  const int col = col0 + cl;
  double acc[kTailMaxThresholds][4];
  unsigned cnt[kTailMaxThresholds];
#pragma unroll
  for (int t = 0; t < kTailMaxThresholds; ++t) {
    acc[t][0] = acc[t][1] = acc[t][2] = acc[t][3] = 0.0;
    cnt[t] = 0u;
  }
  const double members = (double)M, pairs = (double)(M * (M - 1) / 2);
  if (lane < q) {
    const int n_end = min(G, (int)(blockIdx.x + 1) * per);
    for (int n = blockIdx.x * per + lane; n < n_end; n += q) {
      const size_t i = (size_t)n * W + col;
      float v[P];
      bool xfin = true;
#pragma unroll
      for (int k = 0; k < P; ++k) {
        v[k] = __builtin_inff();
        if (k < M) {
          v[k] = mem[(size_t)k * field + i];
          xfin = xfin && isfinite(v[k]);
        }
      }
      const float y = truth[i];
      if (!(xfin && isfinite(y))) continue;         // skipped for every t; the network never sees a NaN
      ord_sort<P>(v);
      const double w = (double)node_w[n];
#pragma unroll
      for (int t = 0; t < kTailMaxThresholds; ++t) {
        if (t < T) {
          const float th = thr[(size_t)t * field + i];
          if (isfinite(th)) {
            const bool up = ((dir_up >> t) & 1u) != 0u;
            const double vy = (double)(up ? fmaxf(y, th) : fminf(y, th));
            double ae = 0.0, pd = 0.0;
            float below = 0.f;
#pragma unroll
            for (int k = 0; k < P; ++k) {           // guarded on M, not on P
              if (k < M) {
                const float u = up ? fmaxf(v[k], th) : fminf(v[k], th);
                ae += fabs((double)u - vy);
                if (k > 0) pd += (double)(k * (M - k)) * ((double)u - (double)below);
                below = u;
              }
            }
            const bool o = up ? y > th : y < th;
            acc[t][0] += w;
            acc[t][1] += w * (ae / members);
            acc[t][2] += w * (pd / pairs);
            acc[t][3] += w * (o ? 1.0 : 0.0);
            cnt[t] += 1u;
          }
        }
      }
    }
  }
  // one threshold per round: the q lanes of a column, added in lane order (idle threads hold zeros nobody reads)
#pragma unroll
  for (int t = 0; t < kTailMaxThresholds; ++t) {
    if (t < T) {                                    // (T is uniform: every thread reaches the barriers)
      __syncthreads();                              // the round before has been read
#pragma unroll
      for (int j = 0; j < 4; ++j) red[j][tid] = acc[t][j];
      redc[tid] = cnt[t];
      __syncthreads();
      for (int e = tid; e < 4 * wt; e += 256) {
        const int j = e / wt, c = e - j * wt;
        double s = red[j][c];
        for (int l = 1; l < q; ++l) s += red[j][l * wt + c];
        part[(((size_t)blockIdx.x * T + t) * 4 + j) * W + col0 + c] = s;
      }
      if (tid < wt) {
        unsigned s = redc[tid];
        for (int l = 1; l < q; ++l) s += redc[l * wt + tid];
        cpart[((size_t)blockIdx.x * T + t) * W + col0 + tid] = s;
      }
    }
  }
}

// One thread per result: the blocks of a sum are added in ascending block order (own text, as the pass: the shared finish
// of gc_colsum.h timed slower here).  e < 4 T W: sum j of column col of
// threshold t, e = (t 4 + j) W + col as the partials lie, stored at out [T][W][4]; then T W counts -> outc [T][W].
__global__ __launch_bounds__(256) void gc_ens_tail_finish_kernel(const double* __restrict__ part,
                                                                  const unsigned* __restrict__ cpart, int blocks, int T,
                                                                  int W, double* __restrict__ out,
                                                                  unsigned long long* __restrict__ outc) {
  const int nd = 4 * T * W, nc = T * W;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < nd) {
    const int tj = e / W, col = e - tj * W, t = tj >> 2, j = tj & 3;
    double s = 0.0;
#pragma unroll 8
    for (int b = 0; b < blocks; ++b) s += part[(size_t)b * nd + e];
    out[((size_t)t * W + col) * 4 + j] = s;
  } else if (e < nd + nc) {
    const int r = e - nd;
    unsigned long long s = 0ull;
#pragma unroll 8
    for (int b = 0; b < blocks; ++b) s += cpart[(size_t)b * nc + r];
    outc[r] = s;
  }
}

static hipError_t launch_ens_tail(hipStream_t s, const float* mem, size_t field, int M, const float* truth,
                                  const float* node_w, const float* thr, int T, unsigned dir_up, int G, int W, double* part,
                                  unsigned* cpart) {
  const int blocks = tail_blocks(G, W), tile_w = tail_tile_width(W);
  const int per = (G + blocks - 1) / blocks;
  const dim3 grid(blocks, tail_tiles(W));
  return pad_dispatch(M, [&](auto p) {
    hipLaunchKernelGGL((gc_ens_tail_kernel<decltype(p)::value>), grid, dim3(256), 0, s, mem, field, M, truth, node_w, thr, T,
                       dir_up, G, W, per, tile_w, part, cpart);
    return hipGetLastError();
  });
}

static hipError_t launch_ens_tail_finish(hipStream_t s, const double* part, const unsigned* cpart, int blocks, int T, int W,
                                         double* out, unsigned long long* outc) {
  const int total = 5 * T * W;
  hipLaunchKernelGGL(gc_ens_tail_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, s, part, cpart, blocks, T, W, out,
                     outc);
  return hipGetLastError();
}

}  // namespace gc

using namespace gci;

extern "C" {

int gc_ens_tail_set(gc_handle* h, int32_t n_thresholds, const float* thresholds, const int32_t* direction) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (!thresholds || !direction) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (n_thresholds < 1 || n_thresholds > gc::kTailMaxThresholds) return fail(h, GC_ERR_UNSUPPORTED, "n_thresholds must be in 1..8");
  unsigned up = 0;
  for (int t = 0; t < n_thresholds; ++t) {
    if (direction[t] == 0) return fail(h, GC_ERR_INVALID_ARGUMENT, "direction " + std::to_string(t) + " is zero");
    if (direction[t] > 0) up |= 1u << t;
  }
  GC_HIP(h, hipSetDevice(h->device));
  const int T = n_thresholds;
  const size_t field = field_len(h);
  int rc;
  if (T != h->tail_T) {
    GC_HIP(h, h->tail_allocs.drop(h->stream));       // nothing reads the old fields any more
    h->tail_T = 0;
    h->d_tail_thr = nullptr;
    if ((rc = dev_alloc(h, &h->d_tail_thr, (size_t)T * field, &h->tail_allocs))) return rc;
  }
  // on the handle's stream, behind whatever still reads the old values; the caller's arrays are free on return
  for (int t = 0; t < T; ++t)
    if ((rc = store_upload(h, h->d_tail_thr + (size_t)t * field, thresholds + (size_t)t * field, field * sizeof(float))))
      return rc;
  h->tail_dir_up = up;
  h->tail_T = T;
  return GC_OK;
  });
}

int gc_ens_tail_score(gc_handle* h, const float* truth, double* sums, uint64_t* counts, uint64_t* invalid) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_graph(h)) || (rc = need(h, h->tail_T != 0, "no thresholds (gc_ens_tail_set)")) || (rc = need_store(h)) ||
      (rc = need_out(h, sums)) || (rc = store_complete(h, h)) || (rc = need_weights(h)))
    return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_tail_score"))) return rc;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, W = c.batch * c.c_out, M = h->ens_members, T = h->tail_T;
  const int blocks = gc::tail_blocks(G, W);
  const size_t n_out = (size_t)4 * T * W, n_outc = (size_t)T * W;
  // sized by T (the layout does not depend on M)
  if ((rc = sized_for(h, h->tail_work_allocs, {(size_t)T}, buf(&h->d_tail_part, (size_t)blocks * n_out),
                      buf(&h->d_tail_cpart, (size_t)blocks * n_outc), buf(&h->d_tail_out, n_out), buf(&h->d_tail_outc, n_outc))))
    return rc;
  hipStream_t s = h->stream;
  std::vector<uint64_t> cnt(n_outc);
  rc = timed(h, h->tail,
             [&] {
               return launch_each(h,
                   [&] {
                     return gc::launch_ens_tail(s, h->d_ens, field_len(h), M, h->d_ens_truth, h->d_ens_w, h->d_tail_thr, T,
                                                h->tail_dir_up, G, W, h->d_tail_part, h->d_tail_cpart);
                   },
                   [&] { return gc::launch_ens_tail_finish(s, h->d_tail_part, h->d_tail_cpart, blocks, T, W, h->d_tail_out, h->d_tail_outc); });
             },
             [&]() -> int {
               if ((rc = read_back(h, sums, h->d_tail_out, n_out)) || (rc = read_back(h, cnt.data(), h->d_tail_outc, n_outc))) return rc;
               return GC_OK;
             });
  if (rc) return rc;
  // every point of the field is counted or skipped: the skipped ones are what the counts leave
  int64_t total = 0;
  for (int t = 0; t < T; ++t) {
    unsigned long long counted = 0ull;
    for (int col = 0; col < W; ++col) counted += cnt[(size_t)t * W + col];
    const unsigned long long skipped = (unsigned long long)G * W - counted;
    total += (int64_t)skipped;
    if (invalid) invalid[t] = skipped;
  }
  h->tail.invalid = total;
  h->tail.blocks = blocks;
  if (counts)
    for (size_t i = 0; i < cnt.size(); ++i) counts[i] = cnt[i];
  return GC_OK;
  });
}

}  // extern "C"
