// Fractions skill score on the device (include/gencast_hip.h, gc_ens_fss_*): the neighbourhood ensemble probability of the
// events of gc_ens_event_score against the observed fraction, at up to 8 neighbourhood sizes from one pass over the code
// bytes that call left on the device.  Kernels and their host code live together here; DESIGN.md section 8o has the
// definitions.
//
// Per threshold t, scale s and counted centre p = (i, j) of a column (b, c), over the counted points q of the window
// Win_s(p) of gc_ens_derive (latitude clipped, longitude wrapping, a row's width that of the row i'), in integers:
//   A = sum row_wq[i'] k(q),  B = sum row_wq[i'] o(q),  N = sum row_wq[i']
// then in double, every operation rounded once:  P = (double) A / ((double) M (double) N),  O = (double) B / (double) N, and
// per (t, s, b, c) four sums over the counted centres with w = (double) wq[g]:
//   w (P - O)(P - O),   w (P P + O O),   w P,   w O.
// Three launches per threshold and chunk of columns:
//   row     one latitude row of one tile of columns: the code bytes staged, inclusive prefix sums of k and of the packed pair
//           (o, counts) along the longitude in LDS, and the row-window sums of every scale from that one prefix (a window is
//           two prefix differences, three where it wraps) into the work buffer: 8 bytes per point and scale.
//   column  per counted centre and scale the at most 2 r_lat + 1 row sums above and below combined with row_wq in uint64,
//           ascending i'; P and O; the four terms into registers, the lanes of a column added in lane order through LDS.
//   finish  the blocks of a sum added in ascending block order.
// No atomics on floats and every sum in a fixed order: two calls give the same bytes.  The work buffer holds the row sums of
// one threshold and one chunk of columns for every scale and every row (a window reaches any row, a column none but its own):
// chunks of columns need no halo.
#include "gc_colsum.h"
#include "gc_store.h"

// the per-point arithmetic is the definition above, operation for operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace gc {

constexpr int kFssMaxScales = 8;
constexpr int kFssMaxLon = 16384;                // the two packed counts of a row fit 16 bits each
constexpr size_t kFssRowLds = 64 * 1024;         // the staged row tile of a workgroup: 2 workgroups per CU (160 KB)
constexpr int kFssMaxTile = 32;                  // columns of a row tile
constexpr int kFssElemBytes = 8;                 // an int32 prefix of k and a uint32 prefix of o | counts << 16 per tile element
constexpr int kFssMaxChunk = 256;                // columns of a chunk: the column pass has one thread per column at least
constexpr size_t kFssWorkBudget = 256u << 20;    // bytes of the work buffer, unless one tile of columns alone needs more
constexpr int kFssMaxBlocks = 256;               // node-range blocks of the column pass (times S workgroups)

// Row pass.  grid = (column tiles of wt inside the chunk, n_lat); wt is a power of two that divides 256.  Thread layout and
// scan of gc_ens_pool_row_mean_kernel: thread t owns column t % wt of longitude lane t / wt; lane l scans its contiguous
// segment of ceil(n_lon / q) longitudes, reads the totals of the segments in front of it, a barrier, and adds them.  All
// integers: k <= 64 per point, so the prefix of k stays below 2^20 and the two counts below 2^14 + 1 each (n_lon <= 16384);
// a field of the packed word never borrows from the other, because every prefix difference taken is that of a sub-range.
// code: the bytes of one threshold [G][W]; the chunk is the columns [c0, c0 + wc); r_lon [S][n_lat];
// work [S][G][wc] (k sum, o | counts << 16).
__global__ __launch_bounds__(256) void gc_ens_fss_row_kernel(const unsigned char* __restrict__ code, int n_lon, int W, int c0,
                                                              int wc, int wt, int S, const int* __restrict__ r_lon,
                                                              uint2* __restrict__ work) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fss_lds[];
  int* const K = reinterpret_cast<int*>(fss_lds);
  unsigned* const C = reinterpret_cast<unsigned*>(K + (size_t)n_lon * wt);
  const int q = 256 / wt;
  const int tid = threadIdx.x;
  const int lane = tid / wt;
  const int cl = tid - lane * wt;
  const int cc = blockIdx.x * wt + cl;             // column inside the chunk
  const bool live = cc < wc && c0 + cc < W;
  const int i = blockIdx.y, n_lat = gridDim.y;
  const unsigned char* const row = code + (size_t)i * n_lon * W + c0 + cc;
  const int seg = (n_lon + q - 1) / q;
  const int j0 = min(n_lon, lane * seg), j1 = min(n_lon, j0 + seg);
  int k = 0;
  unsigned c = 0u;
  for (int j = j0; j < j1; ++j) {
    const unsigned v = live ? (unsigned)row[(size_t)j * W] : 255u;
    if (v != 255u) {
      k += (int)(v & 127u);
      c += (v >> 7) + 65536u;
    }
    K[j * wt + cl] = k;
    C[j * wt + cl] = c;
  }
  __syncthreads();
  int pk = 0;
  unsigned pc = 0u;
  for (int l = 0; l < lane; ++l) {                 // the segments in front of this one
    const int e = min(n_lon, (l + 1) * seg);
    if (e > l * seg) {
      pk += K[(e - 1) * wt + cl];
      pc += C[(e - 1) * wt + cl];
    }
  }
  __syncthreads();
  for (int j = j0; j < j1; ++j) {
    K[j * wt + cl] += pk;
    C[j * wt + cl] += pc;
  }
  __syncthreads();
  if (!live) return;
  const int tot = K[(n_lon - 1) * wt + cl];
  const unsigned ctot = C[(n_lon - 1) * wt + cl];
  const size_t G = (size_t)n_lat * n_lon;
  for (int s = 0; s < S; ++s) {
    const int r = r_lon[s * n_lat + i];
    uint2* const o = work + ((size_t)s * G + (size_t)i * n_lon) * wc + cc;
    for (int j = lane; j < n_lon; j += q) {
      const int lo = j - r, hi = j + r;            // 2 r + 1 <= n_lon: the window wraps at one end at the most
      int wk;
      unsigned wn;
      if (lo < 0) {
        wk = (tot - K[(lo + n_lon - 1) * wt + cl]) + K[hi * wt + cl];
        wn = (ctot - C[(lo + n_lon - 1) * wt + cl]) + C[hi * wt + cl];
      } else if (hi >= n_lon) {
        wk = (tot - K[(lo - 1) * wt + cl]) + K[(hi - n_lon) * wt + cl];
        wn = (ctot - C[(lo - 1) * wt + cl]) + C[(hi - n_lon) * wt + cl];
      } else {
        wk = K[hi * wt + cl] - (lo > 0 ? K[(lo - 1) * wt + cl] : 0);
        wn = C[hi * wt + cl] - (lo > 0 ? C[(lo - 1) * wt + cl] : 0u);
      }
      o[(size_t)j * wc] = make_uint2((unsigned)wk, wn);
    }
  }
}

// P and O of the counted centre n (row i) of one column: ws points at the column's element of node 0 in the scale's slab
// of the work buffer, whose nodes lie wc elements apart.
__device__ inline void fss_point(const uint2* __restrict__ ws, const unsigned* __restrict__ row_wq, int n, int i, int r_lat,
                                 int n_lat, int n_lon, int wc, double members, double* P, double* O) {
  const int i0 = max(0, i - r_lat), i1 = min(n_lat - 1, i + r_lat);
  unsigned long long A = 0ull, B = 0ull, N = 0ull;
  for (int k = i0; k <= i1; ++k) {
    const uint2 v = ws[(size_t)(n + (k - i) * n_lon) * wc];
    const unsigned long long rw = row_wq[k];
    A += rw * v.x;
    B += rw * (v.y & 0xffffu);
    N += rw * (v.y >> 16);
  }
  *P = (double)A / (members * (double)N);
  *O = (double)B / (double)N;
}

// Column pass with the reduction.  grid = (node-range blocks, S).  Thread t owns column t % wc of the chunk and node lane
// t / wc (q = 256 / wc lanes; the threads past q wc idle); block x walks the nodes [x per, (x + 1) per) in steps of q, so a
// wave reads consecutive elements of the work buffer.  part [blocks][S][4][wc].
__global__ __launch_bounds__(256) void gc_ens_fss_col_kernel(const unsigned char* __restrict__ code,
                                                              const unsigned* __restrict__ wq,
                                                              const unsigned* __restrict__ row_wq,
                                                              const int* __restrict__ r_lat, const uint2* __restrict__ work,
                                                              int G, int n_lat, int n_lon, int W, int c0, int wc, int M,
                                                              int per, double* __restrict__ part) {
  __shared__ double red[4][256];
  const int s = blockIdx.y, S = gridDim.y;
  const int q = 256 / wc;
  const int tid = threadIdx.x;
  const int lane = tid / wc;
  const int cl = tid - lane * wc;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (lane < q && c0 + cl < W) {
    const int rl = r_lat[s];
    const double members = (double)M;
    const uint2* const ws = work + (size_t)s * G * wc + cl;
    const unsigned char* const my = code + c0 + cl;
    const int n_end = min(G, (int)(blockIdx.x + 1) * per);
    for (int n = blockIdx.x * per + lane; n < n_end; n += q) {
      if (my[(size_t)n * W] == 255) continue;
      double P, O;
      fss_point(ws, row_wq, n, n / n_lon, rl, n_lat, n_lon, wc, members, &P, &O);
      const double w = (double)wq[n];
      acc[0] += w * ((P - O) * (P - O));
      acc[1] += w * (P * P + O * O);
      acc[2] += w * P;
      acc[3] += w * O;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[j][tid] = acc[j];
  __syncthreads();
  for (int e = tid; e < 4 * wc; e += 256) {          // the lane fold (gc_colsum.h) on each of the four rows
    const int j = e / wc, c = e - j * wc;
    part[(((size_t)blockIdx.x * S + s) * 4 + j) * wc + c] = lane_fold(red[j], c, wc, q);
  }
}

// The ascending block finish (gc_colsum.h) of the chunk: e = (s 4 + j) wc + c as the partials lie -> out [S][W][4] of the
// threshold; a column of the chunk past W stands for no result.  No counts, no skipped points.
struct FssFinishMap {
  const double* part;
  int S, W, c0, wc;
  SkippedSum skipped;
  __host__ __device__ int sums() const { return 4 * S * wc; }
  __host__ __device__ int counts() const { return 0; }
  __device__ BlockSum<double> sum(int e) const {
    const int sj = e / wc, c = e - sj * wc, s = sj >> 2, j = sj & 3;
    if (c0 + c >= W) return {nullptr, 0, 0};
    return {part + e, (size_t)sums(), ((size_t)s * W + c0 + c) * 4 + j};
  }
  __device__ BlockSum<unsigned> count(int) const { return {nullptr, 0, 0}; }
};

// Fields: the column pass of one scale (slab 0 of the work buffer), one thread per point of the chunk, writing
// prob = (float) P and obs = (float) O into the chunk's [G][wc] arrays instead of reducing; NaN where the point does not count.
__global__ __launch_bounds__(256) void gc_ens_fss_field_kernel(const unsigned char* __restrict__ code,
                                                                const unsigned* __restrict__ row_wq, int r_lat,
                                                                const uint2* __restrict__ work, int G, int n_lat, int n_lon,
                                                                int W, int c0, int wc, int M, float* __restrict__ prob,
                                                                float* __restrict__ obs) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)G * wc) return;
  const int n = (int)(e / wc), cl = (int)(e - (size_t)n * wc);
  if (c0 + cl >= W) return;
  float p = __builtin_nanf(""), o = __builtin_nanf("");
  if (code[(size_t)n * W + c0 + cl] != 255) {
    double P, O;
    fss_point(work + cl, row_wq, n, n / n_lon, r_lat, n_lat, n_lon, wc, (double)M, &P, &O);
    p = (float)P;
    o = (float)O;
  }
  prob[e] = p;
  obs[e] = o;
}

static int fss_pow2_floor(int v) {
  int p = 1;
  while (2 * p <= v) p *= 2;
  return p;
}

// columns of a row tile: a power of two, within the LDS budget, no wider than the field needs.  A row of more than 8192
// longitudes takes a tile of one column and up to 128 KB of LDS (one workgroup per CU); 0: n_lon is beyond the limit
static int fss_tile(int n_lon, int W) {
  if (n_lon > kFssMaxLon) return 0;
  const size_t per = (size_t)n_lon * kFssElemBytes;
  if (per > kFssRowLds) return 1;
  int wt = std::min(kFssMaxTile, fss_pow2_floor((int)(kFssRowLds / per)));
  while (wt / 2 >= W) wt /= 2;
  return wt;
}

// columns of a chunk: whole tiles, S + 1 slabs of them within the budget (one tile at the least), kFssMaxChunk at the most
static int fss_chunk(int S, int G, int W, int wt) {
  const size_t per_col = (size_t)kFssElemBytes * (S + 1) * G;
  const int fit = (int)std::min<size_t>(kFssMaxChunk, kFssWorkBudget / per_col);
  const int cap = std::max(wt, fit / wt * wt);
  return std::min(cap, gci::round_up(W, wt));
}

static int fss_blocks(int G, int wc) { return node_blocks(G, 256 / wc, kFssMaxBlocks); }

static hipError_t launch_ens_fss_row(hipStream_t s, const unsigned char* code, int n_lat, int n_lon, int W, int c0, int wc,
                                     int wt, int S, const int* r_lon, uint2* work) {
  const size_t lds = (size_t)n_lon * wt * kFssElemBytes;
  if (lds > kFssRowLds) {                            // (a per-device property of the kernel; setting it again is harmless)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gc_ens_fss_row_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(gc_ens_fss_row_kernel, dim3(wc / wt, n_lat), dim3(256), lds, s, code, n_lon, W, c0, wc, wt, S, r_lon, work);
  return hipGetLastError();
}

static hipError_t launch_ens_fss_col(hipStream_t s, const unsigned char* code, const unsigned* wq, const unsigned* row_wq,
                                     const int* r_lat, const uint2* work, int G, int n_lat, int n_lon, int W, int c0, int wc,
                                     int M, int S, int blocks, double* part) {
  const int per = (G + blocks - 1) / blocks;
  hipLaunchKernelGGL(gc_ens_fss_col_kernel, dim3(blocks, S), dim3(256), 0, s, code, wq, row_wq, r_lat, work, G, n_lat, n_lon, W,
                     c0, wc, M, per, part);
  return hipGetLastError();
}

static hipError_t launch_ens_fss_finish(hipStream_t s, const double* part, int blocks, int S, int W, int c0, int wc, double* out) {
  return launch_block_finish(s, FssFinishMap{part, S, W, c0, wc, {}}, blocks, out, nullptr);
}

static hipError_t launch_ens_fss_field(hipStream_t s, const unsigned char* code, const unsigned* row_wq, int r_lat,
                                       const uint2* work, int G, int n_lat, int n_lon, int W, int c0, int wc, int M, float* prob,
                                       float* obs) {
  const size_t points = (size_t)G * wc;
  hipLaunchKernelGGL(gc_ens_fss_field_kernel, dim3((unsigned)((points + 255) / 256)), dim3(256), 0, s, code, row_wq, r_lat, work,
                     G, n_lat, n_lon, W, c0, wc, M, prob, obs);
  return hipGetLastError();
}

}  // namespace gc

using namespace gci;

namespace {

// what both calls need before they launch: a plan, codes that are those of the store as it stands
int fss_ready(gc_handle* h) {
  int rc;
  if ((rc = need_graph(h)) || (rc = need(h, h->fss_S != 0, "no plan (gc_ens_fss_set)"))) return rc;
  return need(h, h->evt_T != 0 && h->evt_scored && h->ens_members != 0, "no valid event codes on the device (gc_ens_event_score)");
}

// The work buffer (S + 1 slabs of [G][wc] 8-byte elements: the row sums of every scale; the last slab takes the two float
// fields of gc_ens_fss_fields), the per-block partials and the sums of T thresholds: made again by the call that finds any
// of the three sizes changed.
int fss_work(gc_handle* h, int wc, int blocks) {
  const int S = h->fss_S, T = h->evt_T, W = h->cfg.batch * h->cfg.c_out;
  const size_t n_work = (size_t)(S + 1) * h->hg.G * wc, n_part = (size_t)blocks * S * 4 * wc, n_out = (size_t)T * S * W * 4;
  return sized_for(h, h->fss_work_allocs, {n_work, n_part, n_out}, buf(&h->d_fss_work, n_work), buf(&h->d_fss_part, n_part),
                   buf(&h->d_fss_out, n_out));
}

}  // namespace

extern "C" {

int gc_ens_fss_set(gc_handle* h, int32_t n_scales, int32_t n_lat, int32_t n_lon, const int32_t* r_lat, const int32_t* r_lon,
                   const uint32_t* row_wq) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (!r_lat || !r_lon || !row_wq) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (n_scales < 1 || n_scales > gc::kFssMaxScales) return fail(h, GC_ERR_UNSUPPORTED, "n_scales must be in 1..8");
  if (n_lon > gc::kFssMaxLon) return fail(h, GC_ERR_UNSUPPORTED, "n_lon is too large for the packed row counts (n_lon > 16384)");
  if (n_lat < 1 || n_lon < 1 || (int64_t)n_lat * n_lon != (int64_t)h->hg.G)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "n_lat * n_lon must equal the number of grid nodes");
  const int S = n_scales;
  for (int s = 0; s < S; ++s) {
    if (r_lat[s] < 0) return fail(h, GC_ERR_INVALID_ARGUMENT, "r_lat[" + std::to_string(s) + "] is negative");
    for (int i = 0; i < n_lat; ++i)
      if (r_lon[(size_t)s * n_lat + i] < 0 || r_lon[(size_t)s * n_lat + i] > (n_lon - 1) / 2)
        return fail(h, GC_ERR_INVALID_ARGUMENT, "r_lon[" + std::to_string(s) + "][" + std::to_string(i) + "] outside 0 .. (n_lon - 1) / 2");
  }
  for (int i = 0; i < n_lat; ++i)
    if (row_wq[i] < 1u || row_wq[i] > (1u << 24) - 1u)
      return fail(h, GC_ERR_INVALID_ARGUMENT, "row_wq[" + std::to_string(i) + "] outside 1 .. 2^24 - 1");
  GC_HIP(h, hipSetDevice(h->device));
  // one blob of 32-bit words: r_lat [S] (no window reaches further than n_lat rows), r_lon [S][n_lat], row_wq [n_lat]
  std::vector<int32_t> blob((size_t)S + (size_t)S * n_lat + n_lat);
  for (int s = 0; s < S; ++s) blob[(size_t)s] = std::min(r_lat[s], n_lat);
  std::copy(r_lon, r_lon + (size_t)S * n_lat, blob.begin() + S);
  std::memcpy(blob.data() + (size_t)S + (size_t)S * n_lat, row_wq, (size_t)n_lat * sizeof(uint32_t));
  GC_HIP(h, h->fss_allocs.drop(h->stream));          // nothing reads the old plan any more
  h->fss_S = 0;
  int rc;
  int32_t* d_blob = nullptr;
  if ((rc = dev_alloc(h, &d_blob, blob.size(), &h->fss_allocs))) return rc;
  if ((rc = store_upload(h, d_blob, blob.data(), blob.size() * sizeof(int32_t)))) return rc;
  h->d_fss_rlat = d_blob;
  h->d_fss_rlon = d_blob + S;
  h->d_fss_roww = reinterpret_cast<unsigned*>(d_blob + (size_t)S + (size_t)S * n_lat);
  h->fss_rlat.assign(blob.begin(), blob.begin() + S);
  h->fss_n_lat = n_lat;
  h->fss_n_lon = n_lon;
  h->fss_S = S;
  return GC_OK;
  });
}

int gc_ens_fss_score(gc_handle* h, double* sums) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = fss_ready(h)) || (rc = need_out(h, sums))) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  const gc_config& c = h->cfg;
  const int G = h->hg.G, W = c.batch * c.c_out, M = h->ens_members, T = h->evt_T, S = h->fss_S;
  const int n_lat = h->fss_n_lat, n_lon = h->fss_n_lon;
  const size_t field = field_len(h);
  const int wt = gc::fss_tile(n_lon, W), wc = gc::fss_chunk(S, G, W, wt), blocks = gc::fss_blocks(G, wc);
  if ((rc = fss_work(h, wc, blocks))) return rc;
  hipStream_t s = h->stream;
  h->fss.blocks = blocks;                            // of the column pass
  h->fss.chunks = (W + wc - 1) / wc;                 // column chunks every threshold goes through
  return timed(h, h->fss,
               [&]() -> int {
                 for (int t = 0; t < T; ++t) {
                   const unsigned char* const code = h->d_evt_code + (size_t)t * field;
                   for (int c0 = 0; c0 < W; c0 += wc)
                     if ((rc = launch_each(h,
                              [&] { return gc::launch_ens_fss_row(s, code, n_lat, n_lon, W, c0, wc, wt, S, h->d_fss_rlon, h->d_fss_work); },
                              [&] {
                                return gc::launch_ens_fss_col(s, code, h->d_evt_wq, h->d_fss_roww, h->d_fss_rlat, h->d_fss_work, G, n_lat,
                                                              n_lon, W, c0, wc, M, S, blocks, h->d_fss_part);
                              },
                              [&] {
                                return gc::launch_ens_fss_finish(s, h->d_fss_part, blocks, S, W, c0, wc,
                                                                 h->d_fss_out + (size_t)t * S * W * 4);
                              })))
                       return rc;
                 }
                 return GC_OK;
               },
               [&] { return read_back(h, sums, h->d_fss_out, (size_t)T * S * W * 4); });
  });
}

int gc_ens_fss_fields(gc_handle* h, int32_t threshold, int32_t scale, float* prob, float* obs) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = fss_ready(h)) || (rc = need_out(h, prob && obs))) return rc;
  if (threshold < 0 || threshold >= h->evt_T) return fail(h, GC_ERR_INVALID_ARGUMENT, "threshold outside [0, n_thresholds)");
  if (scale < 0 || scale >= h->fss_S) return fail(h, GC_ERR_INVALID_ARGUMENT, "scale outside [0, n_scales)");
  GC_HIP(h, hipSetDevice(h->device));
  const gc_config& c = h->cfg;
  const int G = h->hg.G, W = c.batch * c.c_out, M = h->ens_members, S = h->fss_S;
  const int n_lat = h->fss_n_lat, n_lon = h->fss_n_lon;
  const int wt = gc::fss_tile(n_lon, W), wc = gc::fss_chunk(S, G, W, wt);
  if ((rc = fss_work(h, wc, gc::fss_blocks(G, wc)))) return rc;
  hipStream_t s = h->stream;
  const unsigned char* const code = h->d_evt_code + (size_t)threshold * field_len(h);
  // slab 0: the row sums of the one scale; the last slab: prob [G][wc], then obs [G][wc], 4 bytes per point each
  float* const d_prob = reinterpret_cast<float*>(h->d_fss_work + (size_t)S * G * wc);
  float* const d_obs = d_prob + (size_t)G * wc;
  for (int c0 = 0; c0 < W; c0 += wc) {
    const int wl = std::min(wc, W - c0);
    if ((rc = launch(h, gc::KC_PACK, [&] {
           return gc::launch_ens_fss_row(s, code, n_lat, n_lon, W, c0, wc, wt, 1, h->d_fss_rlon + (size_t)scale * n_lat, h->d_fss_work);
         })))
      return rc;
    if ((rc = launch(h, gc::KC_PACK, [&] {
           return gc::launch_ens_fss_field(s, code, h->d_fss_roww, h->fss_rlat[(size_t)scale], h->d_fss_work, G, n_lat, n_lon, W, c0,
                                           wc, M, d_prob, d_obs);
         })))
      return rc;
    GC_HIP(h, hipMemcpy2DAsync(prob + c0, (size_t)W * sizeof(float), d_prob, (size_t)wc * sizeof(float), (size_t)wl * sizeof(float),
                               (size_t)G, hipMemcpyDeviceToHost, s));
    GC_HIP(h, hipMemcpy2DAsync(obs + c0, (size_t)W * sizeof(float), d_obs, (size_t)wc * sizeof(float), (size_t)wl * sizeof(float),
                               (size_t)G, hipMemcpyDeviceToHost, s));
    GC_HIP(h, hipStreamSynchronize(s));            // the next chunk writes the same device arrays
  }
  return GC_OK;
  });
}

}  // extern "C"
