// Ensemble feature detection on the device (include/gencast_hip.h, gc_ens_feature_*): per member and for the truth of one
// handle's gc_ens_* store, the centres of D detectors -- local extrema of one source channel over the latitude-adaptive
// window of gc_ens_derive that pass a threshold and a ring (depth) test -- as sparse lists, and as dense 0 / 1 strike fields
// in the store of a second handle, which every scorer of the library then reads as it is.  Kernels and their host code
// live together here; DESIGN.md section 8n has the definitions.
//
// A column is one (field z, batch entry b, detector d); the M + 1 fields go through the work buffers in chunks of 8.
// Four passes per chunk:
//   gather   the detection channel, one float of every B c_src wide node row, becomes a dense array of 64-bit keys per
//            column: the order-preserving bits of the signed value s (both zeros on one key) above the node index, all
//            ones where s is not finite.  The smallest key of a window is its argmin under the tie rule of the definition.
//            The same pass writes 0 (NaN where the source is not finite) into the destination.
//   row      one latitude row of keys, minimum over |t| <= r_lon[i'] along the wrapping longitude, by span doubling in LDS.
//   column   per node the minimum of the row results over |i' - i| <= r_lat: the node is an extremum iff that is its own
//            key.  The few extrema that pass the threshold walk their ring; a centre is flagged, counted per block, and the
//            block's threads together store 1 over its strike rectangle (several writers, one value).
//   list     per column the block counts become offsets (a fixed order), and the flagged nodes of the blocks that have
//            any are written in ascending node index.
// Integer comparisons, one double subtraction, no float atomics: two calls give the same bytes.
#include "gc_store.h"

#pragma clang fp contract(off)

namespace gc {

constexpr int kFeatChunk = 8;                    // fields the work buffers hold
constexpr int kFeatMaxD = 8;
constexpr int kFeatMaxCentres = 1024;
constexpr size_t kFeatRowLds = 64 * 1024;        // two rows of keys, ping and pong: 2 workgroups per CU (160 KB)
constexpr unsigned long long kFeatNone = ~0ull;  // the key of a value that is not finite

// the int32 tables of a plan, [D] each, in this order; then r_lon, ring_lon, strike_lon [D][n_lat]
enum { kFtChannel = 0, kFtDir, kFtUseThr, kFtThr /* float bits */, kFtRLat, kFtRingLat, kFtStrikeLat, kFtTables };

__device__ inline const float* feat_field(const float* mem, const float* truth, size_t field, int M, int z) {
  return z < M ? mem + (size_t)z * field : truth;
}
__device__ inline float* feat_field(float* mem, float* truth, size_t field, int M, int z) {
  return z < M ? mem + (size_t)z * field : truth;
}

// ascending in s, -0.0 and +0.0 on one key; s finite
__device__ inline unsigned feat_order_bits(float s) {
  if (s == 0.0f) s = 0.0f;
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float feat_value(unsigned long long key) {
  const unsigned k = (unsigned)(key >> 32);
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// grid = (node blocks, columns of the chunk); column = (zl B + b) D + d
__global__ __launch_bounds__(256) void gc_feat_gather_kernel(const float* __restrict__ smem, const float* __restrict__ struth,
                                                              float* __restrict__ dmem, float* __restrict__ dtruth, int M, int z0,
                                                              int G, int B, int c_src, int D, const int* __restrict__ tab,
                                                              unsigned long long* __restrict__ key) {
  const int col = blockIdx.y;
  const int d = col % D, b = (col / D) % B, zl = col / (D * B);
  const int ch = tab[kFtChannel * D + d];
  const bool neg = tab[kFtDir * D + d] > 0;
  const float* const from = feat_field(smem, struth, (size_t)G * B * c_src, M, z0 + zl) + (size_t)b * c_src + ch;
  float* const to = feat_field(dmem, dtruth, (size_t)G * B * D, M, z0 + zl) + (size_t)b * D + d;
  unsigned long long* const k = key + (size_t)col * G;
  for (size_t n = (size_t)blockIdx.x * 256 + threadIdx.x; n < (size_t)G; n += (size_t)gridDim.x * 256) {
    const float x = from[n * B * c_src];
    const bool fin = isfinite(x);
    k[n] = fin ? ((unsigned long long)feat_order_bits(neg ? -x : x) << 32) | (unsigned)n : kFeatNone;
    to[n * B * D] = fin ? 0.0f : __builtin_nanf("");
  }
}

// grid = (n_lat, columns of the chunk).  The row of keys is staged once and doubled over power-of-two spans, S_k[j] = min
// key[j .. j + 2^k - 1] (circular), from one LDS row into the other; a window of w = 2 r + 1 longitudes is the minimum of the
// two spans of length 2^k <= w that cover it (gc_ens_pool_row_max_kernel has the same form in place, on floats).
__global__ __launch_bounds__(256) void gc_feat_row_kernel(const unsigned long long* __restrict__ key, int G, int n_lat, int n_lon,
                                                           int D, const int* __restrict__ r_lon,
                                                           unsigned long long* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char feat_lds[];
  unsigned long long* cur = reinterpret_cast<unsigned long long*>(feat_lds);
  unsigned long long* nxt = cur + n_lon;
  const int i = blockIdx.x, col = blockIdx.y, d = col % D;
  const size_t base = (size_t)col * G + (size_t)i * n_lon;
  for (int j = threadIdx.x; j < n_lon; j += 256) cur[j] = key[base + j];
  __syncthreads();
  const int r = r_lon[d * n_lat + i], w = 2 * r + 1;
  int span = 1;
  while (2 * span <= w) {
    for (int j = threadIdx.x; j < n_lon; j += 256) {
      int j2 = j + span;
      if (j2 >= n_lon) j2 -= n_lon;
      const unsigned long long a = cur[j], c = cur[j2];
      nxt[j] = a < c ? a : c;
    }
    __syncthreads();
    unsigned long long* const t = cur;
    cur = nxt;
    nxt = t;
    span *= 2;
  }
  for (int j = threadIdx.x; j < n_lon; j += 256) {
    int a = j - r;
    if (a < 0) a += n_lon;
    int c = j + r - span + 1;                      // in (-n_lon, n_lon): span <= w <= n_lon
    if (c < 0) c += n_lon;
    const unsigned long long x = cur[a], y = cur[c];
    out[base + j] = x < y ? x : y;
  }
}

// grid = (blocks of 256 nodes, columns of the chunk)
__global__ __launch_bounds__(256) void gc_feat_col_kernel(const unsigned long long* __restrict__ key,
                                                           const unsigned long long* __restrict__ rowmin, float* __restrict__ dmem,
                                                           float* __restrict__ dtruth, int M, int z0, int G, int n_lat, int n_lon,
                                                           int B, int D, const int* __restrict__ tab,
                                                           const double* __restrict__ depth, unsigned char* __restrict__ flag,
                                                           int* __restrict__ bcount) {
  __shared__ int s_n;
  __shared__ int s_node[256];
  const int col = blockIdx.y;
  const int d = col % D, b = (col / D) % B, zl = col / (D * B);
  const unsigned long long* const k = key + (size_t)col * G;
  const unsigned long long* const rm = rowmin + (size_t)col * G;
  const int* const ring_lon = tab + kFtTables * D + (size_t)(D + d) * n_lat;
  const int* const strike_lon = tab + kFtTables * D + (size_t)(2 * D + d) * n_lat;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const int p = blockIdx.x * 256 + threadIdx.x;
  bool centre = false;
  if (p < G) {
    const unsigned long long own = k[p];
    const int i = p / n_lon, j = p - i * n_lon;
    if (own != kFeatNone) {
      const int r_lat = tab[kFtRLat * D + d];
      const int i0 = max(0, i - r_lat), i1 = min(n_lat - 1, i + r_lat);
      unsigned long long m = kFeatNone;
      for (int ii = i0; ii <= i1; ++ii) {
        const unsigned long long v = rm[(size_t)ii * n_lon + j];
        m = v < m ? v : m;
      }
      centre = m == own;
    }
    if (centre) {
      const float s = feat_value(own);
      if (tab[kFtUseThr * D + d]) {
        const float thr = __int_as_float(tab[kFtThr * D + d]);
        centre = s <= (tab[kFtDir * D + d] > 0 ? -thr : thr);
      }
      const int ring_lat = tab[kFtRingLat * D + d];
      if (centre && ring_lat > 0) {
        unsigned best = 0xFFFFFFFFu;                // the order bits of the smallest finite ring value
        for (int ii = max(0, i - ring_lat); ii <= min(n_lat - 1, i + ring_lat); ++ii) {
          const int rl = ring_lon[ii];
          const bool whole = ii == i - ring_lat || ii == i + ring_lat;
          const unsigned long long* const row = k + (size_t)ii * n_lon;
          for (int t = -rl; t <= rl; t += whole ? 1 : max(1, 2 * rl)) {
            int jj = j + t;
            if (jj < 0) jj += n_lon;
            if (jj >= n_lon) jj -= n_lon;
            const unsigned v = (unsigned)(row[jj] >> 32);
            best = v < best ? v : best;
          }
        }
        centre = best != 0xFFFFFFFFu &&
                 (double)feat_value((unsigned long long)best << 32) - (double)s >= depth[d];
      }
    }
    flag[(size_t)col * G + p] = centre ? 1 : 0;
  }
  if (centre) s_node[atomicAdd(&s_n, 1)] = p;     // (an LDS integer counter: the order inside a block is of no consequence here)
  __syncthreads();
  const int n = s_n;
  if (threadIdx.x == 0) bcount[(size_t)col * gridDim.x + blockIdx.x] = n;
  if (n == 0) return;
  float* const to = feat_field(dmem, dtruth, (size_t)G * B * D, M, z0 + zl) + (size_t)b * D + d;
  const int s_lat = tab[kFtStrikeLat * D + d];
  for (int c = 0; c < n; ++c) {                   // the centre lies in window(n'; strike) iff n' lies in this rectangle
    const int ic = s_node[c] / n_lon, jc = s_node[c] - ic * n_lon;
    const int sl = strike_lon[ic], wdt = 2 * sl + 1;
    const int i0 = max(0, ic - s_lat), i1 = min(n_lat - 1, ic + s_lat);
    const int total = (i1 - i0 + 1) * wdt;
    for (int e = threadIdx.x; e < total; e += 256) {
      const int ii = i0 + e / wdt;
      int jj = jc + (e % wdt) - sl;
      if (jj < 0) jj += n_lon;
      if (jj >= n_lon) jj -= n_lon;
      const size_t nn = (size_t)ii * n_lon + jj;
      if (k[nn] != kFeatNone) to[nn * B * D] = 1.0f;
    }
  }
}

// grid = (columns of the chunk).  Thread t owns the blocks [t seg, (t + 1) seg) of the column pass: its offset is the sum of
// the counts in front of it.  count / node / value are those of the whole call, [M + 1][B][D](...).
__global__ __launch_bounds__(256) void gc_feat_list_kernel(const float* __restrict__ smem, const float* __restrict__ struth, int M,
                                                            int z0, int G, int B, int c_src, int D, const int* __restrict__ tab,
                                                            const unsigned char* __restrict__ flag,
                                                            const int* __restrict__ bcount, int nblk, int max_centres,
                                                            int* __restrict__ count, int* __restrict__ node,
                                                            float* __restrict__ value) {
  __shared__ int s_sum[256];
  const int col = blockIdx.x;
  const int d = col % D, b = (col / D) % B, zl = col / (D * B);
  const int* const bc = bcount + (size_t)col * nblk;
  const int seg = (nblk + 255) / 256;
  const int k0 = min(nblk, (int)threadIdx.x * seg), k1 = min(nblk, k0 + seg);
  int mine = 0;
  for (int kb = k0; kb < k1; ++kb) mine += bc[kb];
  s_sum[threadIdx.x] = mine;
  __syncthreads();
  int off = 0, total = 0;
  for (int t = 0; t < 256; ++t) {
    const int v = s_sum[t];
    if (t < (int)threadIdx.x) off += v;
    total += v;
  }
  const size_t out = (size_t)(z0 + zl) * B * D + (size_t)b * D + d;
  int* const o_node = node + out * max_centres;
  unsigned* const o_val = reinterpret_cast<unsigned*>(value) + out * max_centres;
  if (threadIdx.x == 0) count[out] = total;
  for (int e = total + (int)threadIdx.x; e < max_centres; e += 256) {   // past the last centre: node -1, value 0
    o_node[e] = -1;
    o_val[e] = 0u;
  }
  if (mine == 0 || off >= max_centres) return;
  const unsigned* const from = reinterpret_cast<const unsigned*>(feat_field(smem, struth, (size_t)G * B * c_src, M, z0 + zl)) +
                               (size_t)b * c_src + tab[kFtChannel * D + d];
  const unsigned char* const f = flag + (size_t)col * G;
  for (int kb = k0; kb < k1; ++kb) {
    if (bc[kb] == 0) continue;
    const int p1 = min(G, (kb + 1) * 256);
    for (int p = kb * 256; p < p1; ++p) {
      if (!f[p]) continue;
      if (off >= max_centres) return;
      o_node[off] = p;
      o_val[off] = from[(size_t)p * B * c_src];   // x, the same bits
      ++off;
    }
  }
}

static size_t feat_row_lds(int n_lon) { return (size_t)2 * n_lon * sizeof(unsigned long long); }

}  // namespace gc

using namespace gci;

extern "C" {

int gc_ens_feature_set(gc_handle* h, int32_t c_src, int32_t D, const int32_t* channel, const int32_t* direction,
                       const int32_t* use_threshold, const float* threshold, int32_t n_lat, int32_t n_lon, const int32_t* r_lat,
                       const int32_t* r_lon, const int32_t* ring_lat, const int32_t* ring_lon, const double* depth,
                       const int32_t* strike_lat, const int32_t* strike_lon, int32_t max_centres) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (!channel || !direction || !use_threshold || !threshold || !r_lat || !r_lon || !ring_lat || !ring_lon || !depth ||
      !strike_lat || !strike_lon)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (c_src < 1) return fail(h, GC_ERR_INVALID_ARGUMENT, "c_src must be positive");
  if (D < 1 || D > gc::kFeatMaxD || D != h->cfg.c_out)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "D must lie in 1 .. 8 and equal c_out of the handle");
  if (n_lat < 1 || n_lon < 1 || (int64_t)n_lat * n_lon != (int64_t)h->hg.G)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "n_lat * n_lon must equal the number of grid nodes");
  if (max_centres < 1 || max_centres > gc::kFeatMaxCentres) return fail(h, GC_ERR_INVALID_ARGUMENT, "max_centres outside 1 .. 1024");
  for (int d = 0; d < D; ++d) {
    const std::string det = "detector " + std::to_string(d) + ": ";
    if (channel[d] < 0 || channel[d] >= c_src) return fail(h, GC_ERR_INVALID_ARGUMENT, det + "source channel outside [0, c_src)");
    if (direction[d] == 0) return fail(h, GC_ERR_INVALID_ARGUMENT, det + "direction is 0 (< 0: minimum, > 0: maximum)");
    if (use_threshold[d] && !std::isfinite(threshold[d])) return fail(h, GC_ERR_INVALID_ARGUMENT, det + "threshold is not finite");
    if (r_lat[d] < 0) return fail(h, GC_ERR_INVALID_ARGUMENT, det + "r_lat is negative");
    if (ring_lat[d] < 0) return fail(h, GC_ERR_INVALID_ARGUMENT, det + "ring_lat is negative");
    if (strike_lat[d] < 0) return fail(h, GC_ERR_INVALID_ARGUMENT, det + "strike_lat is negative");
    if (ring_lat[d] > 0 && !std::isfinite(depth[d])) return fail(h, GC_ERR_INVALID_ARGUMENT, det + "depth is not finite");
    const int32_t* const lons[3] = {r_lon, ring_lon, strike_lon};
    const char* const names[3] = {"r_lon", "ring_lon", "strike_lon"};
    for (int a = 0; a < 3; ++a)
      for (int i = 0; i < n_lat; ++i) {
        const int32_t v = lons[a][(size_t)d * n_lat + i];
        if (v < 0 || v > (n_lon - 1) / 2)
          return fail(h, GC_ERR_INVALID_ARGUMENT, det + names[a] + "[" + std::to_string(i) + "] outside 0 .. (n_lon - 1) / 2");
      }
  }
  if (gc::feat_row_lds(n_lon) > gc::kFeatRowLds) return fail(h, GC_ERR_UNSUPPORTED, "n_lon is too large for the two key rows of the row pass (64 KB of LDS)");
  GC_HIP(h, hipSetDevice(h->device));
  // one blob: depth [D] doubles, then the int32 tables [kFtTables][D] and r_lon, ring_lon, strike_lon [D][n_lat]
  const size_t n_i = (size_t)gc::kFtTables * D + (size_t)3 * D * n_lat;
  std::vector<double> blob((size_t)D + (n_i + 1) / 2);
  for (int d = 0; d < D; ++d) blob[d] = ring_lat[d] > 0 ? depth[d] : 0.0;
  int32_t* const ib = reinterpret_cast<int32_t*>(blob.data() + D);
  for (int d = 0; d < D; ++d) {
    ib[gc::kFtChannel * D + d] = channel[d];
    ib[gc::kFtDir * D + d] = direction[d] > 0 ? 1 : -1;
    ib[gc::kFtUseThr * D + d] = use_threshold[d] ? 1 : 0;
    const float t = use_threshold[d] ? threshold[d] : 0.0f;
    std::memcpy(&ib[gc::kFtThr * D + d], &t, sizeof(float));
    ib[gc::kFtRLat * D + d] = r_lat[d];
    ib[gc::kFtRingLat * D + d] = ring_lat[d];
    ib[gc::kFtStrikeLat * D + d] = strike_lat[d];
  }
  int32_t* const lb = ib + (size_t)gc::kFtTables * D;
  std::copy(r_lon, r_lon + (size_t)D * n_lat, lb);
  std::copy(ring_lon, ring_lon + (size_t)D * n_lat, lb + (size_t)D * n_lat);
  std::copy(strike_lon, strike_lon + (size_t)D * n_lat, lb + (size_t)2 * D * n_lat);
  GC_HIP(h, h->feat_allocs.drop(h->stream));         // nothing reads the old plan any more
  h->feat_set = false;
  h->feat_listed = false;
  int rc;
  double* d_blob = nullptr;
  if ((rc = dev_alloc(h, &d_blob, blob.size(), &h->feat_allocs))) return rc;
  GC_HIP(h, h->ev_feat_src.ensure());
  if ((rc = store_upload(h, d_blob, blob.data(), blob.size() * sizeof(double)))) return rc;
  h->d_feat_depth = d_blob;
  h->d_feat_tab = reinterpret_cast<int*>(d_blob + D);
  h->feat_c_src = c_src;
  h->feat_n_lat = n_lat;
  h->feat_n_lon = n_lon;
  h->feat_max = max_centres;
  h->feat_set = true;
  return GC_OK;
  });
}

int gc_ens_feature(gc_handle* h, gc_handle* src, const float* truth) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_source(h, src)) || (rc = need_graph(h)) || (rc = need(h, h->feat_set, "no plan (gc_ens_feature_set)"))) return rc;
  const int G = h->hg.G, B = h->cfg.batch, D = h->cfg.c_out, M = h->ens_members, c_src = h->feat_c_src;
  const int n_lat = h->feat_n_lat, n_lon = h->feat_n_lon, maxc = h->feat_max;
  const int chunk = std::min(gc::kFeatChunk, M + 1);
  const int nblk = (G + 255) / 256;
  // the work of a chunk: keys and row minima (8 bytes each), block counts (4 bytes per 256 nodes), flags (1 byte), per
  // column; then the lists of the whole call: count, node, value
  const size_t cols = (size_t)gc::kFeatChunk * B * D, per_list = (size_t)(M + 1) * B * D;
  const size_t o_row = cols * G * 8, o_bc = 2 * o_row, o_flag = o_bc + cols * nblk * 4;
  const size_t o_count = (o_flag + cols * G + 7) / 8 * 8, o_node = o_count + (per_list * 4 + 7) / 8 * 8;
  const size_t o_value = o_node + per_list * maxc * 4, bytes = o_value + per_list * maxc * 4;
  rc = fill_open(h, src, c_src, truth, "gc_ens_feature", h->ev_feat_src, [&] {   // sized by the field, M and max_centres
    if (h->feat_work_allocs.differs({bytes})) h->feat_listed = false;          // the lists go with the buffer
    return sized_for(h, h->feat_work_allocs, {bytes}, buf(&h->d_feat_work, bytes));
  });
  if (rc) return rc;
  unsigned char* const wk = h->d_feat_work;
  unsigned long long* const key = reinterpret_cast<unsigned long long*>(wk);
  unsigned long long* const rowmin = reinterpret_cast<unsigned long long*>(wk + o_row);
  int* const bcount = reinterpret_cast<int*>(wk + o_bc);
  unsigned char* const flag = wk + o_flag;
  int* const l_count = reinterpret_cast<int*>(wk + o_count);
  int* const l_node = reinterpret_cast<int*>(wk + o_node);
  float* const l_value = reinterpret_cast<float*>(wk + o_value);
  hipStream_t s = h->stream;
  h->feat_listed = false;
  const int* const tab = h->d_feat_tab;
  rc = timed(h, h->feat,
             [&]() -> int {
               for (int z0 = 0; z0 <= M; z0 += chunk) {
                 const int nc = std::min(chunk, M + 1 - z0) * B * D;
                 if ((rc = launch_each(h,
                          [&] {
                            hipLaunchKernelGGL(gc::gc_feat_gather_kernel, dim3(std::min(nblk, 1024), nc), dim3(256), 0, s, src->d_ens,
                                               src->d_ens_truth, h->d_ens, h->d_ens_truth, M, z0, G, B, c_src, D, tab, key);
                            return hipGetLastError();
                          },
                          [&] {
                            hipLaunchKernelGGL(gc::gc_feat_row_kernel, dim3(n_lat, nc), dim3(256), gc::feat_row_lds(n_lon), s, key, G, n_lat,
                                               n_lon, D, tab + gc::kFtTables * D, rowmin);
                            return hipGetLastError();
                          },
                          [&] {
                            hipLaunchKernelGGL(gc::gc_feat_col_kernel, dim3(nblk, nc), dim3(256), 0, s, key, rowmin, h->d_ens, h->d_ens_truth,
                                               M, z0, G, n_lat, n_lon, B, D, tab, h->d_feat_depth, flag, bcount);
                            return hipGetLastError();
                          },
                          [&] {
                            hipLaunchKernelGGL(gc::gc_feat_list_kernel, dim3(nc), dim3(256), 0, s, src->d_ens, src->d_ens_truth, M, z0, G, B,
                                               c_src, D, tab, flag, bcount, nblk, maxc, l_count, l_node, l_value);
                            return hipGetLastError();
                          })))
                   return rc;
               }
               return GC_OK;
             },
             no_readbacks);
  if (rc) return rc;
  h->feat.blocks = std::min(nblk, 1024);             // of the gather, the one pass that walks the nodes grid-stride
  fill_close(h);
  h->d_feat_count = l_count;
  h->d_feat_node = l_node;
  h->d_feat_value = l_value;
  h->feat_list_M = M;
  h->feat_listed = true;
  return GC_OK;
  });
}

int gc_ens_feature_centres(gc_handle* h, int32_t* count, int32_t* node, float* value) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (!count || !node || !value) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (!h->feat_listed) return fail(h, GC_ERR_STATE, "no centre lists (gc_ens_feature has not run since the plan or the store changed)");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t n = (size_t)(h->feat_list_M + 1) * h->cfg.batch * h->cfg.c_out;
  GC_HIP(h, hipStreamSynchronize(h->stream));
  GC_HIP(h, hipMemcpy(count, h->d_feat_count, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  GC_HIP(h, hipMemcpy(node, h->d_feat_node, n * h->feat_max * sizeof(int32_t), hipMemcpyDeviceToHost));
  GC_HIP(h, hipMemcpy(value, h->d_feat_value, n * h->feat_max * sizeof(float), hipMemcpyDeviceToHost));
  return GC_OK;
  });
}

}  // extern "C"
