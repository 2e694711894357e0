// Multivariate ensemble scores on the device (include/gencast_hip.h, gc_ens_energy_*, gc_ens_variogram_*): the raw sums of
// the energy score over groups of channels and whole fields, and of the variogram score over pairs of grid points a fixed
// offset apart, formed from the gc_ens_* store.  Kernels and their host code live together here; DESIGN.md section 8k has
// the definitions and the error bounds the tests assert.
//
// Members x_0 .. x_{M-1} and the truth y are [G, B, c_out] float32, w[g] the node weight.  A point (g, b, c) is valid iff y
// and all M members are finite there.  Write x_M = y.
// Energy.  The plan gives K groups (1 <= K <= 32) and a per-channel scale: group[c] in {-1, 0 .. K-1} (-1: in no group,
// every group non-empty), a[c] finite and > 0 for grouped channels.  Per batch member b, group k and pair 0 <= i < j <= M,
// pair index p = j (j - 1) / 2 + i, P = M (M + 1) / 2:
//   D2[b][k][p] = sum omega (d d) over the valid points of the group     omega = (double)w[g] a[c],  d = (double)x_i - (double)x_j
//   S0[b][k]    = sum omega over the same points                         invalid = skipped points of grouped channels
// The difference is exact; each product and each addition is a rounded double operation with no contraction.  Invalid
// points are skipped, not multiplied by zero.
// Variogram.  The plan gives the grid n_lat n_lon = G (node = i n_lon + j), O offsets (di, dj) (1 <= O <= 16, not (0, 0),
// |di| < n_lat, |dj| < n_lon) and an order p in {0.5, 1, 2} -- formed with sqrt, identity and a product, no pow.  The
// partner of (i, j) is (i + di, (j + dj) mod n_lon); the pair is skipped when i + di leaves [0, n_lat) and when either end
// is invalid.  Per valid pair, in double:
//   omega = (w[g] + w[g']) / 2     v(u) = |u_g - u_g'|^p     vx = (sum_i v(x_i)) / M, ascending slot order     vy = v(y)
// Per (b, c, o):  V0 = sum omega   V1 = sum omega (vy - vx)^2   V2 = sum omega vx   V3 = sum omega vy   and a pair count.
// No atomics on floats: every accumulator has one writer and every sum a fixed order (a thread's points ascending, the
// slices or node lanes in index order, the blocks in index order), so the same call twice returns identical bytes.
#include "gc_colsum.h"
#include "gc_store.h"

// the per-point arithmetic is the definition above, operation for operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace gc {

constexpr int kMvMaxGroups = 32;
constexpr int kMvMaxOffsets = 16;
constexpr int kMvTile = 256;                     // points of a tile: one per thread while staging
// row stride = 1 mod 32: at one column, rows i and i' share a ds_read_b32 bank only when i = i' mod 32.  The lanes of a
// 32-lane half own consecutive pairs, so their rows i are consecutive but for one wrap (pair (j - 1, j) is followed by
// (0, j + 1)): at most a 2-way conflict on the lanes around the wrap, none elsewhere
constexpr int kMvLd = kMvTile + 1;
constexpr int kMvMaxWorkgroups = 2048;           // of the energy pass, over all (b, k): about eight per CU

static int mv_pairs(int M) { return M * (M + 1) / 2; }
// pairs a thread owns: 1 (P <= 256, the spare threads then take slices of the tile), 3 or 9 (P <= 2080 at M = 64)
static int mv_npp(int P) { return P <= 256 ? 1 : P <= 768 ? 3 : 9; }
// node-range blocks of one (b, k): a tile of work each or more, kMvMaxWorkgroups in all.  That cap also bounds the
// per-block partials: blocks BK <= 2048 rows of P <= 2080 doubles, 32.5 MB at the most.
static int mv_energy_blocks(int G, int BK, int nc_max) {
  const long tiles = ((long)G * nc_max + kMvTile - 1) / kMvTile;
  return (int)std::max<long>(1, std::min({tiles, (long)std::max(1, kMvMaxWorkgroups / BK), (long)G}));
}

// The energy pass.  Workgroup (x, y): node range [x per, (x + 1) per) of batch member b = y / K and group k = y % K; its
// points are (node, channel of the group), node-major, in tiles of 256.  Staging: thread t reads the M + 1 values of point
// t of the tile (each load coalesced across the wave where the group's channels are neighbours), decides its validity and
// writes them to LDS as float tile[M + 1][257]; omega and the flag go beside them.  Then every thread walks the tile for
// the pairs it owns -- pair tid + 256 q, q < NPP, accumulators in registers; with P <= 256 the threads form 256 / P slices
// that take every (256 / P)-th point and are added in slice order at the end.  A point that is not valid is skipped: its
// values never enter the arithmetic.
// Out, as plain stores: part[x][y][P], s0part[x][y], ipart[x][y].
template <int NPP>
__global__ __launch_bounds__(256) void gc_ens_energy_kernel(const float* __restrict__ mem, size_t field, int M,
                                                             const float* __restrict__ truth,
                                                             const float* __restrict__ node_w,
                                                             const double* __restrict__ scale,
                                                             const int* __restrict__ gchan, const int* __restrict__ goff,
                                                             int G, int B, int C, int K, int per,
                                                             double* __restrict__ part, double* __restrict__ s0part,
                                                             unsigned* __restrict__ ipart) {
  extern __shared__ __attribute__((aligned(16))) float mv_tile[];
  __shared__ double omega[kMvTile];
  __shared__ double red[kMvTile];
  __shared__ int ok[kMvTile];
  __shared__ unsigned skipped;
  const int tid = threadIdx.x;
  const int b = blockIdx.y / K, k = blockIdx.y - b * K;
  const int P = M * (M + 1) / 2;
  const int c0 = goff[k], nc = goff[k + 1] - c0;
  const int n0 = min(G, (int)blockIdx.x * per), n1 = min(G, n0 + per);
  const int npts = (n1 - n0) * nc;
  // the pairs of this thread as LDS row offsets; a pair beyond P reads row 0 twice (d = 0 adds +0.0, and is not stored)
  const int L = NPP == 1 ? max(1, kMvTile / P) : 1;
  const int slice = NPP == 1 ? tid / P : 0;
  int ia[NPP], ja[NPP];
#pragma unroll
  for (int q = 0; q < NPP; ++q) {
    const int p = NPP == 1 ? tid - slice * P : tid + kMvTile * q;
    ia[q] = ja[q] = 0;
    if (p < P) {
      int j = (int)((1.f + sqrtf(1.f + 8.f * (float)p)) * 0.5f);
      while (j * (j - 1) / 2 > p) --j;
      while ((j + 1) * j / 2 <= p) ++j;
      ia[q] = (p - j * (j - 1) / 2) * kMvLd;
      ja[q] = j * kMvLd;
    }
  }
  const int t0 = slice < L ? slice : kMvTile;      // (the threads beyond the last whole slice walk nothing)
  double acc[NPP];
#pragma unroll
  for (int q = 0; q < NPP; ++q) acc[q] = 0.0;
  double s0 = 0.0;
  unsigned inv = 0;
  if (tid == 0) skipped = 0u;
  for (int base = 0; base < npts; base += kMvTile) {
    const int pt = base + tid;
    double om = 0.0;
    int valid = 0;
    if (pt < npts) {
      const int dn = pt / nc;
      const int c = gchan[c0 + pt - dn * nc], n = n0 + dn;
      const size_t at = ((size_t)n * B + b) * C + c;
      bool fin = true;
#pragma unroll 4
      for (int r = 0; r < M; ++r) {
        const float v = mem[(size_t)r * field + at];
        fin = fin && isfinite(v);
        mv_tile[r * kMvLd + tid] = v;
      }
      const float y = truth[at];
      fin = fin && isfinite(y);
      mv_tile[M * kMvLd + tid] = y;
      if (fin) {
        om = (double)node_w[n] * scale[c];
        s0 += om;
        valid = 1;
      } else {
        ++inv;
      }
    }
    omega[tid] = om;
    ok[tid] = valid;
    __syncthreads();
    const int tn = min(kMvTile, npts - base);
    for (int t = t0; t < tn; t += L) {
      if (!ok[t]) continue;
      const double w = omega[t];
#pragma unroll
      for (int q = 0; q < NPP; ++q) {
        const double d = (double)mv_tile[ia[q] + t] - (double)mv_tile[ja[q] + t];
        acc[q] += w * (d * d);
      }
    }
    __syncthreads();
  }
  if (inv) atomicAdd(&skipped, inv);               // (an integer: the order of these does not show)
  const size_t row = (size_t)blockIdx.x * gridDim.y + blockIdx.y;
  if constexpr (NPP == 1) {                        // the slices of a pair, added in slice order
    red[tid] = acc[0];
    __syncthreads();
    if (tid < P) {
      double t = red[tid];
      for (int l = 1; l < L; ++l) t += red[l * P + tid];
      part[row * P + tid] = t;
    }
    __syncthreads();
  } else {
#pragma unroll
    for (int q = 0; q < NPP; ++q) {
      const int p = tid + kMvTile * q;
      if (p < P) part[row * P + p] = acc[q];
    }
  }
  red[tid] = s0;
  __syncthreads();
  if (tid == 0) {
    double t = red[0];
    for (int l = 1; l < kMvTile; ++l) t += red[l];
    s0part[row] = t;
    ipart[row] = skipped;
  }
}

// The ascending block finish (gc_colsum.h): e < BK P: D2, as the partials lie; then BK sums S0 from their own array -> out
// behind them; no counts; the skipped points -> outc[0].
struct EnergyFinishMap {
  const double* part;
  const double* s0part;
  int BK, P;
  SkippedSum skipped;
  __host__ __device__ int sums() const { return BK * P + BK; }
  __host__ __device__ int counts() const { return 0; }
  __device__ BlockSum<double> sum(int e) const {
    const int nd = BK * P;
    if (e < nd) return {part + e, (size_t)nd, (size_t)e};
    return {s0part + (e - nd), (size_t)BK, (size_t)e};
  }
  __device__ BlockSum<unsigned> count(int) const { return {nullptr, 0, 0}; }
};

static hipError_t launch_ens_energy(hipStream_t s, const float* mem, size_t field, int M, const float* truth,
                                    const float* node_w, const double* scale, const int* gchan, const int* goff, int G, int B,
                                    int C, int K, int blocks, double* part, double* s0part, unsigned* ipart) {
  const int P = mv_pairs(M);
  const int per = (G + blocks - 1) / blocks;
  const size_t lds = (size_t)(M + 1) * kMvLd * sizeof(float);
  const dim3 grid(blocks, B * K);
#define GC_MV_CASE(NPP)                                                                                                      \
  {                                                                                                                          \
    if (lds > 48 * 1024) {                         /* (a per-device property of the kernel; setting it again is harmless) */ \
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gc_ens_energy_kernel<NPP>),                           \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                              \
      if (e != hipSuccess) return e;                                                                                         \
    }                                                                                                                        \
    hipLaunchKernelGGL((gc_ens_energy_kernel<NPP>), grid, dim3(256), lds, s, mem, field, M, truth, node_w, scale, gchan,     \
                       goff, G, B, C, K, per, part, s0part, ipart);                                                          \
    return hipGetLastError();                                                                                                \
  }
  switch (mv_npp(P)) {
    case 1: GC_MV_CASE(1);
    case 3: GC_MV_CASE(3);
    default: GC_MV_CASE(9);
  }
#undef GC_MV_CASE
}

static hipError_t launch_ens_energy_finish(hipStream_t s, const double* part, const double* s0part, const unsigned* ipart,
                                           int blocks, int BK, int P, double* out, unsigned long long* outc) {
  return launch_block_finish(s, EnergyFinishMap{part, s0part, BK, P, {ipart, BK, 0}}, blocks, out, outc);
}

// |u|^p for the three orders: PK = 0 sqrt, 1 identity, 2 a product
template <int PK>
__device__ inline double mv_vpow(double u) {
  const double a = fabs(u);
  return PK == 0 ? sqrt(a) : PK == 1 ? a : a * a;
}

// The variogram pass, on the 256-wide cut of gc_colsum.h; grid.z is the offset.  The M + 1 values of the point and of its
// partner are read from HBM, each load coalesced across the wave.
// Out, as plain stores: part[block x][offset][4][W] (double), cpart[block x][offset][W] (valid pairs).
template <int PK>
__global__ __launch_bounds__(256) void gc_ens_variogram_kernel(const float* __restrict__ mem, size_t field, int M,
                                                                const float* __restrict__ truth,
                                                                const float* __restrict__ node_w,
                                                                const int* __restrict__ offs, int n_lat, int n_lon, int W,
                                                                int per, double* __restrict__ part,
                                                                unsigned* __restrict__ cpart) {
  __shared__ double lane_sum[256];
  __shared__ unsigned lane_cnt[256];
  const int G = n_lat * n_lon;
  const int o = blockIdx.z, O = gridDim.z;
  const int di = offs[2 * o], dj = offs[2 * o + 1];
  const ColTile ct(256, 256, W, blockIdx.y);
  const int tid = threadIdx.x, col = ct.col;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned cnt = 0;
  if (ct.active()) {
    const double dM = (double)M;
    const int n_end = ct.n_end(G, per);
    for (int n = ct.n_begin(per); n < n_end; n += ct.q) {
      const int i = n / n_lon, j = n - i * n_lon;
      const int i2 = i + di;
      if (i2 < 0 || i2 >= n_lat) continue;
      int j2 = (j + dj) % n_lon;
      if (j2 < 0) j2 += n_lon;
      const int n2 = i2 * n_lon + j2;
      const size_t a = (size_t)n * W + col, c = (size_t)n2 * W + col;
      const float ya = truth[a], yc = truth[c];
      bool fin = isfinite(ya) && isfinite(yc);
      double vsum = 0.0;
#pragma unroll 4
      for (int k = 0; k < M; ++k) {
        const float xa = mem[(size_t)k * field + a], xc = mem[(size_t)k * field + c];
        fin = fin && isfinite(xa) && isfinite(xc);
        vsum += mv_vpow<PK>((double)xa - (double)xc);
      }
      if (!fin) continue;
      const double vx = vsum / dM, vy = mv_vpow<PK>((double)ya - (double)yc);
      const double w = 0.5 * ((double)node_w[n] + (double)node_w[n2]);
      const double e = vy - vx;
      s[0] += w;
      s[1] += w * (e * e);
      s[2] += w * vx;
      s[3] += w * vy;
      ++cnt;
    }
  }
  const size_t row = (size_t)blockIdx.x * O + o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double t = col_total(lane_sum, s[k], ct);
    if (tid < ct.wt) part[(row * 4 + k) * W + col] = t;
  }
  const unsigned t = col_total(lane_cnt, cnt, ct);
  if (tid < ct.wt) cpart[row * W + col] = t;
}

// The ascending block finish: e < 4 W O: sum k of column col at offset o, e = (k O + o) W + col -> out [4][W][O]; then W O
// counts, as the partials lie -> outc [W][O].
struct VariogramFinishMap {
  const double* part;
  const unsigned* cpart;
  int W, O;
  SkippedSum skipped;
  __host__ __device__ int sums() const { return 4 * W * O; }
  __host__ __device__ int counts() const { return W * O; }
  __device__ BlockSum<double> sum(int e) const {
    const int k = e / (W * O), r = e - k * W * O, o = r / W, col = r - o * W;
    return {part + ((size_t)o * 4 + k) * W + col, (size_t)sums(), ((size_t)k * W + col) * O + o};
  }
  __device__ BlockSum<unsigned> count(int r) const {
    const int o = r / W, col = r - o * W;
    return {cpart + r, (size_t)counts(), (size_t)col * O + o};
  }
};

static hipError_t launch_ens_variogram(hipStream_t s, int pk, const float* mem, size_t field, int M, const float* truth,
                                       const float* node_w, const int* offs, int O, int n_lat, int n_lon, int B, int c_out,
                                       double* part, unsigned* cpart) {
  const int W = B * c_out, G = n_lat * n_lon;
  const int blocks = loss_reduce_blocks(G, B, c_out);
  const int per = (G + blocks - 1) / blocks;
  const dim3 grid(blocks, (W + 255) / 256, O);
#define GC_MV_CASE(PK)                                                                                                     \
  case PK:                                                                                                                 \
    hipLaunchKernelGGL((gc_ens_variogram_kernel<PK>), grid, dim3(256), 0, s, mem, field, M, truth, node_w, offs, n_lat,    \
                       n_lon, W, per, part, cpart);                                                                        \
    break
  switch (pk) {
    GC_MV_CASE(0);
    GC_MV_CASE(1);
    GC_MV_CASE(2);
  }
#undef GC_MV_CASE
  return hipGetLastError();
}

static hipError_t launch_ens_variogram_finish(hipStream_t s, const double* part, const unsigned* cpart, int blocks, int W, int O,
                                              double* out, unsigned long long* outc) {
  return launch_block_finish(s, VariogramFinishMap{part, cpart, W, O, {}}, blocks, out, outc);
}

}  // namespace gc

using namespace gci;

namespace {

// validation shared by the two scoring entries: a graph, a plan, a complete store, weights
int mv_ready(gc_handle* h, bool plan, const char* no_plan) {
  int rc;
  if ((rc = need_graph(h)) || (rc = need(h, plan, no_plan)) || (rc = need_store(h)) || (rc = store_complete(h, h))) return rc;
  return need_weights(h);
}

}  // namespace

extern "C" {

int gc_ens_energy_set(gc_handle* h, int32_t n_groups, const int32_t* group, const double* scale) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (n_groups < 1 || n_groups > gc::kMvMaxGroups) return fail(h, GC_ERR_UNSUPPORTED, "n_groups must be in 1..32");
  if (!group || !scale) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  const int C = h->cfg.c_out, K = n_groups;
  std::vector<int> goff((size_t)K + 1, 0), gchan;
  for (int c = 0; c < C; ++c) {
    if (group[c] < -1 || group[c] >= K)
      return fail(h, GC_ERR_INVALID_ARGUMENT, "group of channel " + std::to_string(c) + " is outside -1 .. n_groups - 1");
    if (group[c] >= 0 && !(std::isfinite(scale[c]) && scale[c] > 0.0))
      return fail(h, GC_ERR_INVALID_ARGUMENT, "scale of channel " + std::to_string(c) + " is not finite and > 0");
  }
  for (int k = 0; k < K; ++k) {                       // the channels of a group, ascending
    for (int c = 0; c < C; ++c)
      if (group[c] == k) gchan.push_back(c);
    goff[(size_t)k + 1] = (int)gchan.size();
    if (goff[(size_t)k + 1] == goff[(size_t)k]) return fail(h, GC_ERR_INVALID_ARGUMENT, "group " + std::to_string(k) + " is empty");
  }
  std::vector<double> a(scale, scale + C);
  for (int c = 0; c < C; ++c)
    if (group[c] < 0) a[(size_t)c] = 0.0;             // (never read)
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, h->en_allocs.drop(h->stream));            // nothing reads the old plan any more
  h->en_set = false;
  if (int rc = alloc_all(h, h->en_allocs, buf(&h->d_en_gchan, gchan), buf(&h->d_en_goff, goff), buf(&h->d_en_scale, a))) return rc;
  h->en_K = K;
  h->en_nc_max = 0;
  for (int k = 0; k < K; ++k) h->en_nc_max = std::max(h->en_nc_max, goff[(size_t)k + 1] - goff[(size_t)k]);
  h->en_set = true;
  return GC_OK;
  });
}

int gc_ens_energy_score(gc_handle* h, const float* truth, double* d2, double* s0, uint64_t* invalid) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = mv_ready(h, h->en_set, "no plan (gc_ens_energy_set)")) || (rc = need_out(h, d2 && s0))) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_energy_score"))) return rc;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, B = c.batch, M = h->ens_members, K = h->en_K, BK = B * K, P = gc::mv_pairs(M);
  const int blocks = gc::mv_energy_blocks(G, BK, h->en_nc_max);
  const size_t n_out = (size_t)BK * P + BK;
  // sized by M and the plan
  if ((rc = sized_for(h, h->en_work_allocs, {(size_t)M, (size_t)K, (size_t)blocks}, buf(&h->d_en_part, (size_t)blocks * n_out),
                      buf(&h->d_en_ipart, (size_t)blocks * BK), buf(&h->d_en_out, n_out), buf(&h->d_en_outc, 1))))
    return rc;
  hipStream_t s = h->stream;
  double* const s0part = h->d_en_part + (size_t)blocks * BK * P;
  uint64_t inv = 0;
  rc = timed(h, h->en,
             [&] {
               return launch_each(h,
                   [&] {
                     return gc::launch_ens_energy(s, h->d_ens, field_len(h), M, h->d_ens_truth, h->d_ens_w, h->d_en_scale, h->d_en_gchan,
                                                  h->d_en_goff, G, B, c.c_out, K, blocks, h->d_en_part, s0part, h->d_en_ipart);
                   },
                   [&] {
                     return gc::launch_ens_energy_finish(s, h->d_en_part, s0part, h->d_en_ipart, blocks, BK, P, h->d_en_out, h->d_en_outc);
                   });
             },
             [&]() -> int {
               if ((rc = read_back(h, d2, h->d_en_out, (size_t)BK * P)) || (rc = read_back(h, s0, h->d_en_out + (size_t)BK * P, (size_t)BK)) ||
                   (rc = read_back(h, &inv, h->d_en_outc, 1)))
                 return rc;
               return GC_OK;
             });
  if (rc) return rc;
  h->en.invalid = (int64_t)inv;
  h->en.blocks = blocks;
  if (invalid) invalid[0] = inv;
  return GC_OK;
  });
}

int gc_ens_variogram_set(gc_handle* h, int32_t n_lat, int32_t n_lon, int32_t n_offsets, const int32_t* offsets, double p) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (n_offsets < 1 || n_offsets > gc::kMvMaxOffsets) return fail(h, GC_ERR_UNSUPPORTED, "n_offsets must be in 1..16");
  const int pk = p == 0.5 ? 0 : p == 1.0 ? 1 : p == 2.0 ? 2 : -1;
  if (pk < 0) return fail(h, GC_ERR_UNSUPPORTED, "the order p must be 0.5, 1 or 2");
  if (!offsets) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (n_lat < 1 || n_lon < 1 || (int64_t)n_lat * n_lon != h->hg.G)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "n_lat * n_lon is not the number of grid nodes");
  const int O = n_offsets;
  for (int o = 0; o < O; ++o) {
    const int64_t di = offsets[2 * o], dj = offsets[2 * o + 1];
    if ((di == 0 && dj == 0) || std::llabs(di) >= n_lat || std::llabs(dj) >= n_lon)
      return fail(h, GC_ERR_INVALID_ARGUMENT, "offset " + std::to_string(o) + " is (0, 0) or reaches beyond the grid");
  }
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, h->vg_allocs.drop(h->stream));            // the plan and the buffers sized by it
  h->vg_set = false;
  const gc_config& c = h->cfg;
  const int W = c.batch * c.c_out;
  const size_t blocks = (size_t)gc::loss_reduce_blocks(h->hg.G, c.batch, c.c_out);
  const std::vector<int> offs(offsets, offsets + 2 * O);
  if (int rc = alloc_all(h, h->vg_allocs, buf(&h->d_vg_offs, offs), buf(&h->d_vg_part, blocks * O * 4 * W),
                         buf(&h->d_vg_cpart, blocks * O * W), buf(&h->d_vg_out, (size_t)4 * W * O), buf(&h->d_vg_outc, (size_t)W * O)))
    return rc;
  h->vg_O = O;
  h->vg_pk = pk;
  h->vg_n_lat = n_lat;
  h->vg_n_lon = n_lon;
  h->vg_set = true;
  return GC_OK;
  });
}

int gc_ens_variogram_score(gc_handle* h, const float* truth, double* sums, uint64_t* counts) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = mv_ready(h, h->vg_set, "no plan (gc_ens_variogram_set)")) || (rc = need_out(h, sums))) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_variogram_score"))) return rc;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, B = c.batch, W = B * c.c_out, M = h->ens_members, O = h->vg_O;
  const int blocks = gc::loss_reduce_blocks(G, B, c.c_out);
  hipStream_t s = h->stream;
  h->vg.blocks = blocks;
  return timed(h, h->vg,
               [&] {
                 return launch_each(h,
                     [&] {
                       return gc::launch_ens_variogram(s, h->vg_pk, h->d_ens, field_len(h), M, h->d_ens_truth, h->d_ens_w, h->d_vg_offs, O,
                                                       h->vg_n_lat, h->vg_n_lon, B, c.c_out, h->d_vg_part, h->d_vg_cpart);
                     },
                     [&] { return gc::launch_ens_variogram_finish(s, h->d_vg_part, h->d_vg_cpart, blocks, W, O, h->d_vg_out, h->d_vg_outc); });
               },
               [&]() -> int {
                 if ((rc = read_back(h, sums, h->d_vg_out, (size_t)4 * W * O)) ||
                     (counts && (rc = read_back(h, counts, h->d_vg_outc, (size_t)W * O))))
                   return rc;
                 return GC_OK;
               });
  });
}

}  // extern "C"
