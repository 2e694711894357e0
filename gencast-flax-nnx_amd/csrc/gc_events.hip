// Ensemble event verification on the device (include/gencast_hip.h, gc_ens_event_*): exceedance events of the members of
// the gc_ens_* store against threshold fields -- the joint table of (observed, members in the event) that the Brier score,
// the reliability curve, the ROC and the economic value are formed from.  Kernels and their host code live together here;
// DESIGN.md section 8f has the definitions.
//
// Per threshold t (field thr_t, direction dir_t) and point (g, b, c), from the float32 members x_0 .. x_{M-1} and the truth y:
//   event(v) = dir_t > 0 ? v > thr_t : v < thr_t            strict, on the float32 values
//   k = #{i : event(x_i)},  o = event(y)
// The point counts when y, all M members and thr_t are finite.  Per column (b, c), over the counted nodes:
//   weighted[t][b][c][o][k] += wq[g]     counts[t][b][c][o][k] += 1     (wq: uint32 node weights, quantised on the host)
// Everything is an integer: the LDS and global atomics commute, so the result does not depend on how the launch was
// scheduled, and the tests compare with ==.  Two passes: the code pass streams the M members once and leaves one byte
// per point and threshold (k | o << 7, 255 = not counted: the exceedance-probability map), the table pass reads those
// bytes and the weights.  Fusing them would need [T][W][2 (M + 1)] 64-bit bins per workgroup (268 KB at T = 4, W = 82,
// M = 50), which no workgroup has.
#include "gc_colsum.h"
#include "gc_store.h"

namespace gc {

constexpr int kEvtMaxThresholds = 8;
constexpr size_t kEvtTableLds = 40 * 1024;       // both tables of a workgroup: 4 workgroups = 16 waves per CU (160 KB)
constexpr int kEvtMaxWorkgroups = 1024;          // table pass: 4 per CU; every one flushes its bins with global atomics

template <int V>
__device__ inline void evt_load(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

// Code pass: a pure stream.  One thread owns V consecutive points (V = 4 where the field length is a multiple of 4: 16-byte
// loads, one 4-byte store per threshold; else V = 1).  y and the T thresholds sit in registers, the M members stream past
// (M loads of stride `field`, coalesced across the wave), T V counters stay in registers; nothing is read twice, so nothing
// goes through LDS.  Bit t of dir_up: the event of threshold t is `value > thr`.  code [T][field].
template <int T, int V>
__global__ __launch_bounds__(256) void gc_ens_event_code_kernel(const float* __restrict__ mem, size_t field, int M,
                                                                 const float* __restrict__ truth,
                                                                 const float* __restrict__ thr, unsigned dir_up,
                                                                 unsigned char* __restrict__ code) {
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * V;
  if (i >= field) return;                          // (V = 4 only with field % 4 == 0: a thread's points are all inside)
  float y[V], th[T][V];
  int cnt[T][V];
  bool fin[V];
  evt_load<V>(truth + i, y);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    evt_load<V>(thr + (size_t)t * field + i, th[t]);
#pragma unroll
    for (int j = 0; j < V; ++j) cnt[t][j] = 0;
  }
#pragma unroll
  for (int j = 0; j < V; ++j) fin[j] = isfinite(y[j]);
#pragma unroll 4
  for (int k = 0; k < M; ++k) {
    float x[V];
    evt_load<V>(mem + (size_t)k * field + i, x);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      fin[j] = fin[j] && isfinite(x[j]);
#pragma unroll
      for (int t = 0; t < T; ++t) cnt[t][j] += (((dir_up >> t) & 1u) ? x[j] > th[t][j] : x[j] < th[t][j]) ? 1 : 0;
    }
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    unsigned char c[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const bool o = ((dir_up >> t) & 1u) ? y[j] > th[t][j] : y[j] < th[t][j];
      c[j] = fin[j] && isfinite(th[t][j]) ? (unsigned char)(cnt[t][j] | (o ? 128 : 0)) : (unsigned char)255;
    }
    unsigned char* const out = code + (size_t)t * field + i;
    if constexpr (V == 4)
      *reinterpret_cast<unsigned*>(out) = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16) | ((unsigned)c[3] << 24);
    else
      out[0] = c[0];
  }
}

// Column tiles of the table pass: as few as fit the LDS budget, of equal width.  A column's bins are padded to an ODD
// stride 2 (M + 1) + 1: for a rare event nearly every point of a column lands in bin (o = 0, k = 0), the lanes of a wave
// own different columns (thread layout of gc_colsum.h), and an odd stride puts those bins on different banks.
static int evt_stride(int M) { return 2 * (M + 1) + 1; }
static int evt_tiles(int W, int M) {
  const int fit = std::max(1, std::min(256, (int)(kEvtTableLds / ((size_t)evt_stride(M) * 12))));
  return (W + fit - 1) / fit;
}
static int evt_tile_width(int W, int M) { const int tiles = evt_tiles(W, M); return (W + tiles - 1) / tiles; }
// node-range blocks: within kEvtMaxWorkgroups for the whole grid
static int evt_node_blocks(int G, int W, int M, int T) {
  return node_blocks(G, 256 / evt_tile_width(W, M), kEvtMaxWorkgroups / (T * evt_tiles(W, M)));
}

// Table pass.  grid = (node-range blocks, thresholds, column tiles): equal-width tiles of gc_colsum.h, cap = 256.
// Dynamic LDS: unsigned long long[wt][stride] weighted, then unsigned[wt][stride] counts.  A block's non-zero bins
// leave by integer atomics into the zeroed global tables weighted / counts [T][W][2][M + 1] and invalid [T]: per-block
// partials would be blocks x T x W x 2 (M + 1) x 12 bytes (hundreds of MB at the 1-degree size) for sums that need no order.
__global__ __launch_bounds__(256) void gc_ens_event_table_kernel(const unsigned char* __restrict__ code, size_t field,
                                                                  const unsigned* __restrict__ wq, int G, int W, int M,
                                                                  int tile_w, int per,
                                                                  unsigned long long* __restrict__ weighted,
                                                                  unsigned long long* __restrict__ counts,
                                                                  unsigned long long* __restrict__ invalid) {
  extern __shared__ __attribute__((aligned(16))) unsigned char evt_lds[];
  __shared__ unsigned skipped;
  const int t = blockIdx.y;
  const ColTile ct(tile_w, 256, W, blockIdx.z);
  const int col0 = ct.col0, wt = ct.wt, cl = ct.cl;
  const int tid = threadIdx.x;
  const int bins = 2 * (M + 1), stride = bins + 1;
  unsigned long long* const wtab = reinterpret_cast<unsigned long long*>(evt_lds);
  unsigned* const ctab = reinterpret_cast<unsigned*>(wtab + (size_t)tile_w * stride);
  for (int i = tid; i < wt * stride; i += 256) {
    wtab[i] = 0ull;
    ctab[i] = 0u;
  }
  if (tid == 0) skipped = 0u;
  __syncthreads();
  unsigned inv = 0;
  if (ct.active()) {
    const unsigned char* const my = code + (size_t)t * field + col0 + cl;
    const int n_end = ct.n_end(G, per);
#pragma unroll 4
    for (int n = ct.n_begin(per); n < n_end; n += ct.q) {
      const unsigned c = my[(size_t)n * W];
      if (c == 255u) {
        ++inv;
        continue;
      }
      const int bin = cl * stride + (int)(c >> 7) * (M + 1) + (int)(c & 127u);
      atomicAdd(&wtab[bin], (unsigned long long)wq[n]);
      atomicAdd(&ctab[bin], 1u);
    }
  }
  if (inv) atomicAdd(&skipped, inv);
  __syncthreads();
  const size_t base = ((size_t)t * W + col0) * bins;
  for (int i = tid; i < wt * bins; i += 256) {
    const int c = i / bins;
    const int l = c * stride + (i - c * bins);
    const unsigned n = ctab[l];
    if (n) {
      atomicAdd(&counts[base + i], (unsigned long long)n);
      const unsigned long long w = wtab[l];
      if (w) atomicAdd(&weighted[base + i], w);
    }
  }
  if (tid == 0 && skipped) atomicAdd(&invalid[t], (unsigned long long)skipped);
}

template <int T>
static void evt_code_launch(hipStream_t s, const float* mem, size_t field, int M, const float* truth, const float* thr,
                            unsigned dir_up, unsigned char* code) {
  if (field % 4 == 0)
    hipLaunchKernelGGL((gc_ens_event_code_kernel<T, 4>), dim3((unsigned)((field / 4 + 255) / 256)), dim3(256), 0, s, mem, field, M,
                       truth, thr, dir_up, code);
  else
    hipLaunchKernelGGL((gc_ens_event_code_kernel<T, 1>), dim3((unsigned)((field + 255) / 256)), dim3(256), 0, s, mem, field, M,
                       truth, thr, dir_up, code);
}

static hipError_t launch_ens_event_code(hipStream_t s, const float* mem, size_t field, int M, const float* truth, int T,
                                        const float* thr, unsigned dir_up, unsigned char* code) {
  switch (T) {
    case 1: evt_code_launch<1>(s, mem, field, M, truth, thr, dir_up, code); break;
    case 2: evt_code_launch<2>(s, mem, field, M, truth, thr, dir_up, code); break;
    case 3: evt_code_launch<3>(s, mem, field, M, truth, thr, dir_up, code); break;
    case 4: evt_code_launch<4>(s, mem, field, M, truth, thr, dir_up, code); break;
    case 5: evt_code_launch<5>(s, mem, field, M, truth, thr, dir_up, code); break;
    case 6: evt_code_launch<6>(s, mem, field, M, truth, thr, dir_up, code); break;
    case 7: evt_code_launch<7>(s, mem, field, M, truth, thr, dir_up, code); break;
    case 8: evt_code_launch<8>(s, mem, field, M, truth, thr, dir_up, code); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

static hipError_t launch_ens_event_table(hipStream_t s, const unsigned char* code, size_t field, const unsigned* wq, int G,
                                         int W, int M, int T, unsigned long long* weighted, unsigned long long* counts,
                                         unsigned long long* invalid) {
  const int tiles = evt_tiles(W, M), tile_w = evt_tile_width(W, M);
  const int blocks = evt_node_blocks(G, W, M, T);
  const int per = (G + blocks - 1) / blocks;
  const size_t lds = (size_t)tile_w * evt_stride(M) * (sizeof(unsigned long long) + sizeof(unsigned));
  hipLaunchKernelGGL(gc_ens_event_table_kernel, dim3(blocks, T, tiles), dim3(256), lds, s, code, field, wq, G, W, M, tile_w,
                     per, weighted, counts, invalid);
  return hipGetLastError();
}

}  // namespace gc

using namespace gci;

namespace {

// words of one table [T][W][2][M + 1]
size_t evt_table_len(const gc_handle* h, int T, int M) { return (size_t)T * h->cfg.batch * h->cfg.c_out * 2 * (M + 1); }

}  // namespace

extern "C" {

int gc_ens_event_set(gc_handle* h, int32_t n_thresholds, const float* thresholds, const int32_t* direction,
                     const uint32_t* node_weight_q) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (!thresholds || !direction || !node_weight_q) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (n_thresholds < 1 || n_thresholds > gc::kEvtMaxThresholds) return fail(h, GC_ERR_UNSUPPORTED, "n_thresholds must be in 1..8");
  unsigned up = 0;
  for (int t = 0; t < n_thresholds; ++t) {
    if (direction[t] == 0) return fail(h, GC_ERR_INVALID_ARGUMENT, "direction " + std::to_string(t) + " is zero");
    if (direction[t] > 0) up |= 1u << t;
  }
  GC_HIP(h, hipSetDevice(h->device));
  const int T = n_thresholds;
  const size_t field = field_len(h);
  int rc;
  h->evt_scored = false;
  if (T != h->evt_T) {
    GC_HIP(h, h->evt_allocs.drop(h->stream));        // nothing reads the old buffers any more
    h->evt_table_allocs.free();
    h->evt_T = 0;
    if ((rc = alloc_all(h, h->evt_allocs, buf(&h->d_evt_thr, (size_t)T * field), buf(&h->d_evt_code, (size_t)T * field),
                        buf(&h->d_evt_wq, (size_t)h->hg.G))))
      return rc;
  }
  // on the handle's stream, behind whatever still reads the old values; the caller's arrays are free on return
  for (int t = 0; t < T; ++t)
    if ((rc = store_upload(h, h->d_evt_thr + (size_t)t * field, thresholds + (size_t)t * field, field * sizeof(float))))
      return rc;
  if ((rc = store_upload(h, h->d_evt_wq, node_weight_q, (size_t)h->hg.G * sizeof(uint32_t)))) return rc;
  h->evt_dir_up = up;
  h->evt_T = T;
  return GC_OK;
  });
}

int gc_ens_event_score(gc_handle* h, const float* truth, uint64_t* weighted, uint64_t* counts, uint64_t* invalid) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_graph(h)) || (rc = need(h, h->evt_T != 0, "no thresholds (gc_ens_event_set)")) || (rc = need_store(h)) ||
      (rc = need_out(h, weighted)) || (rc = store_complete(h, h)))
    return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_event_score"))) return rc;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, W = c.batch * c.c_out, M = h->ens_members, T = h->evt_T;
  const size_t field = field_len(h), len = evt_table_len(h, T, M);
  if ((rc = sized_for(h, h->evt_table_allocs, {(size_t)T, (size_t)M}, buf(&h->d_evt_table, 2 * len + (size_t)T)))) return rc;
  hipStream_t s = h->stream;
  unsigned long long* const d_w = h->d_evt_table;
  unsigned long long* const d_c = d_w + len;
  unsigned long long* const d_inv = d_c + len;
  std::vector<uint64_t> inv((size_t)T);
  rc = timed(h, h->evt,
             [&]() -> int {
               GC_HIP(h, hipMemsetAsync(d_w, 0, (2 * len + (size_t)T) * sizeof(unsigned long long), s));
               return launch_each(h,
                   [&] {
                     return gc::launch_ens_event_code(s, h->d_ens, field, M, h->d_ens_truth, T, h->d_evt_thr, h->evt_dir_up, h->d_evt_code);
                   },
                   [&] { return gc::launch_ens_event_table(s, h->d_evt_code, field, h->d_evt_wq, G, W, M, T, d_w, d_c, d_inv); });
             },
             [&]() -> int {
               if ((rc = read_back(h, weighted, d_w, len)) || (counts && (rc = read_back(h, counts, d_c, len))) ||
                   (rc = read_back(h, inv.data(), d_inv, inv.size())))
                 return rc;
               return GC_OK;
             });
  if (rc) return rc;
  int64_t total = 0;
  for (int t = 0; t < T; ++t) {
    total += (int64_t)inv[(size_t)t];
    if (invalid) invalid[t] = inv[(size_t)t];
  }
  h->evt.invalid = total;
  h->evt.blocks = gc::evt_node_blocks(G, W, M, T);
  h->evt_scored = true;
  return GC_OK;
  });
}

int gc_ens_event_download(gc_handle* h, int32_t threshold, uint8_t* code) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (h->evt_T == 0) return fail(h, GC_ERR_STATE, "no thresholds (gc_ens_event_set)");
  if (!code) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (threshold < 0 || threshold >= h->evt_T) return fail(h, GC_ERR_INVALID_ARGUMENT, "threshold outside [0, n_thresholds)");
  if (!h->evt_scored) return fail(h, GC_ERR_STATE, "no event codes on the device (gc_ens_event_score)");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t field = field_len(h);
  GC_HIP(h, hipMemcpyAsync(code, h->d_evt_code + (size_t)threshold * field, field, hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
  });
}

}  // extern "C"
