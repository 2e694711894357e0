// Derived and pooled ensemble fields on the device (include/gencast_hip.h, gc_ens_derive_*): the members and the truth of
// one handle's gc_ens_* store become, in the store of a second handle, fields of derived channels (a copy of a source
// channel, or the norm of two: wind speed) pooled over a latitude-adaptive window (max, min or an area-weighted mean).
// Every scorer of the library then works on that store as it is.  Kernels and their host code live together here;
// DESIGN.md section 8g has the definitions.
//
// Three passes per call, fields z = 0 .. M (the M members, then the truth):
//   derive   d = x[src_a] (the same bits), or (float) sqrt(u u + v v) with u = (double) x[src_a] sa + la (v likewise), into
//            the destination slot.  With pool == NONE this is the whole call.
//   row      one latitude row i' of d pooled along the longitude over |t| <= r_lon[i'], wrapping, non-finite values
//            skipped, into an intermediate: one float per point (max; min is max of the negated values), or a double sum
//            and an int32 count of the finite values (mean).
//   column   per point the intermediates of the rows |i' - i| <= r_lat (clipped at the poles) combined -- the mean with
//            row_weight[i'] -- and written over the centre; NaN where the centre itself is not finite.
// No atomics: every output has one writer and every sum a fixed order, so two calls give the same bytes.
//
// A plan set through gc_ens_derive_set_expr has four more derive ops, all in physical units
// p(c) = (double) x[c] scale[c] + loc[c] and rounded to float32 once: SUM and NORM of term lists sum_t coef_t p(a_t) [p(b_t)]
// (thickness, shear, column integrals, IVT), and VORTICITY and DIVERGENCE of a (u, v) pair by centred differences on the
// sphere.  Its derive pass is gc_ens_derive_expr_kernel, followed -- where the grid has pole rows and the plan one of the
// last two ops -- by gc_ens_derive_pole_kernel; the pooling passes behind them are the same.
#include "gc_store.h"

// the per-point arithmetic is the definition above, operation for operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace gc {

enum { kDrvCopy = 0, kDrvNorm2 = 1, kDrvSum = 2, kDrvNorm = 3, kDrvVort = 4, kDrvDiv = 5 };
enum { kPoolNone = 0, kPoolMax = 1, kPoolMin = 2, kPoolMean = 3 };
constexpr int kDrvChunk = 8;                     // fields the intermediate holds: the M + 1 fields go through it in chunks
constexpr size_t kDrvRowLds = 64 * 1024;         // the staged row tile of a workgroup: 2 workgroups per CU (160 KB)
constexpr int kDrvMaxTile = 32;                  // columns of a row tile: 32 lanes x 4 bytes = one 128-byte line per longitude
constexpr int kDrvRegs = 64;                     // max pass: tile elements per thread (kDrvRowLds / 4 / 256)
constexpr int kDrvMeanBytes = 12;                // mean pass: a double prefix sum and an int32 prefix count per tile element
constexpr int kDrvListTerms = 64;                // terms of one list (37 ERA5 levels fit), and of a whole plan: the term table
constexpr int kDrvPlanTerms = 1024;              // is staged in LDS at kDrvTermBytes a term, 48 KB at the most
constexpr int kDrvTermBytes = 48;                // coef, sa, la, sb, lb (double), a, b (int32)
constexpr int kDrvPoleLon = 8191;                // pole pass: n_lon + 1 doubles of LDS, 64 KB at the most

// field z of a store: member z, or the truth behind the last member
__device__ inline const float* drv_field(const float* mem, const float* truth, size_t field, int M, int z) {
  return z < M ? mem + (size_t)z * field : truth;
}
__device__ inline float* drv_field(float* mem, float* truth, size_t field, int M, int z) {
  return z < M ? mem + (size_t)z * field : truth;
}

// Derive pass.  Thread layout of gc_ens_state_kernel: thread t owns derived column t % wt = (b, j) of node lane t / wt, so
// its row of the table (op, the two source channels, the affine) sits in registers for the whole node loop; the active
// threads of a block store q whole consecutive destination rows.  grid = (node blocks, column tiles of 256, M + 1).
__global__ __launch_bounds__(256) void gc_ens_derive_kernel(const float* __restrict__ smem, const float* __restrict__ struth,
                                                             float* __restrict__ dmem, float* __restrict__ dtruth, int M,
                                                             int G, int B, int c_src, int c_d, const int* __restrict__ op,
                                                             const int* __restrict__ src_a, const int* __restrict__ src_b,
                                                             const double* __restrict__ affine) {
  const int W = B * c_d, Ws = B * c_src;
  const int col0 = blockIdx.y * 256;
  const int wt = min(256, W - col0);
  const int q = 256 / wt;
  const int lane = threadIdx.x / wt;
  if (lane >= q) return;
  const int col = col0 + ((int)threadIdx.x - lane * wt);
  const int b = col / c_d, j = col - b * c_d;
  const int z = blockIdx.z;
  const unsigned* const from = reinterpret_cast<const unsigned*>(drv_field(smem, struth, (size_t)G * Ws, M, z)) + (size_t)b * c_src;
  unsigned* const to = reinterpret_cast<unsigned*>(drv_field(dmem, dtruth, (size_t)G * W, M, z)) + col;
  const int ca = src_a[j];
  if (op[j] == kDrvCopy) {                         // the same bits: a NaN keeps its payload
    for (size_t n = (size_t)blockIdx.x * q + lane; n < (size_t)G; n += (size_t)gridDim.x * q) to[n * W] = from[n * Ws + ca];
    return;
  }
  const int cb = src_b[j];
  const double sa = affine[4 * j], la = affine[4 * j + 1], sb = affine[4 * j + 2], lb = affine[4 * j + 3];
  for (size_t n = (size_t)blockIdx.x * q + lane; n < (size_t)G; n += (size_t)gridDim.x * q) {
    const double u = (double)__uint_as_float(from[n * Ws + ca]) * sa + la;
    const double v = (double)__uint_as_float(from[n * Ws + cb]) * sb + lb;
    to[n * W] = __float_as_uint((float)sqrt(u * u + v * v));
  }
}

// ---- the ops of gc_ens_derive_set_expr ---------------------------------------------------------------------------------------
// the tables of such a plan, all in device memory (one blob: gc_ens_derive_set_expr)
struct DrvExpr {
  const int *op, *src_a, *src_b;                   // [c_d]; VORTICITY / DIVERGENCE: the u and the v channel
  const double* affine;                            // [c_d][4]: NORM2 as given; VORTICITY / DIVERGENCE (su, lu, sv, lv)
  const int* tstart;                               // [c_d][3]: list 1 is [s0, s1), list 2 [s1, s2) of the term table
  const double* tq;                                // [5][n_terms]: coef, scale[a], loc[a], scale[b], loc[b]
  const int *ta, *tb;                              // [n_terms]; tb = -1: no second factor
  const double *coslat, *inv_rcos, *inv_dphi;      // [n_lat]
  const int* pole;                                 // [n_lat]
  double inv_2dlam;
  int n_terms, n_lat, n_lon;
};

// S = sum_t coef_t p(a_t) [p(b_t)] over the terms [t0, t1), ascending; q, ta, tb: the staged term table; row: the thread's
// (node, b) row of source channels
__device__ inline double drv_term_sum(const unsigned* __restrict__ row, int t0, int t1, const double* q, const int* ta,
                                      const int* tb, int nT) {
  double S = 0.0;
  for (int t = t0; t < t1; ++t) {
    double term = q[t] * ((double)__uint_as_float(row[ta[t]]) * q[nT + t] + q[2 * nT + t]);
    const int b = tb[t];
    if (b >= 0) term = term * ((double)__uint_as_float(row[b]) * q[3 * nT + t] + q[4 * nT + t]);
    S = S + term;
  }
  return S;
}

// The double result of VORTICITY (vort) or DIVERGENCE at row i (not a pole row), longitude l.  from: the field's batch b.
// One field is differenced along the longitude (v for the vorticity, u for the divergence), the other, times cos(lat),
// along the latitude over the rows i- = max(i - 1, 0) and i+ = min(i + 1, n_lat - 1).
__device__ inline double drv_curl(const unsigned* __restrict__ from, size_t Ws, int i, int l, bool vort, int cu, int cv,
                                  double su, double lu, double sv, double lv, const DrvExpr& g) {
  const int lm = l == 0 ? g.n_lon - 1 : l - 1, lp = l + 1 == g.n_lon ? 0 : l + 1;
  const int im = max(i - 1, 0), ip = min(i + 1, g.n_lat - 1);
  const int ca = vort ? cv : cu, cb = vort ? cu : cv;
  const double sa = vort ? sv : su, la = vort ? lv : lu, sb = vort ? su : sv, lb = vort ? lu : lv;
  const size_t r = (size_t)i * g.n_lon;
  const double ap = (double)__uint_as_float(from[(r + lp) * Ws + ca]) * sa + la;
  const double am = (double)__uint_as_float(from[(r + lm) * Ws + ca]) * sa + la;
  const double bp = (double)__uint_as_float(from[((size_t)ip * g.n_lon + l) * Ws + cb]) * sb + lb;
  const double bm = (double)__uint_as_float(from[((size_t)im * g.n_lon + l) * Ws + cb]) * sb + lb;
  const double x = ap - am;
  const double y = bp * g.coslat[ip] - bm * g.coslat[im];
  const double t1 = x * g.inv_2dlam, t2 = y * g.inv_dphi[i];
  return (vort ? t1 - t2 : t1 + t2) * g.inv_rcos[i];
}

// Derive pass of a gc_ens_derive_set_expr plan: grid and thread layout of gc_ens_derive_kernel.  The term table is staged
// in LDS once per workgroup (dynamic, kDrvTermBytes a term): the lanes of a wave own different derived columns and walk
// different lists, which LDS serves at a few cycles a step where a global table would cost a cache line each.  The source
// row of a node is read straight from global memory by the c_d threads of its (node, b): with few derived columns the lanes
// of a wave sit on different rows and every load touches a line per lane, which is what bounds a long list (DESIGN.md
// section 8p has the measurement).  A pole row of VORTICITY / DIVERGENCE is left to gc_ens_derive_pole_kernel.
__global__ __launch_bounds__(256) void gc_ens_derive_expr_kernel(const float* __restrict__ smem, const float* __restrict__ struth,
                                                                  float* __restrict__ dmem, float* __restrict__ dtruth, int M,
                                                                  int G, int B, int c_src, int c_d, DrvExpr g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char drv_lds[];
  const int nT = g.n_terms;
  double* const q = reinterpret_cast<double*>(drv_lds);
  int* const ta = reinterpret_cast<int*>(q + (size_t)5 * nT);
  int* const tb = ta + nT;
  for (int t = threadIdx.x; t < 5 * nT; t += 256) q[t] = g.tq[t];
  for (int t = threadIdx.x; t < nT; t += 256) {
    ta[t] = g.ta[t];
    tb[t] = g.tb[t];
  }
  __syncthreads();
  const int W = B * c_d, Ws = B * c_src;
  const int col0 = blockIdx.y * 256;
  const int wt = min(256, W - col0);
  const int nq = 256 / wt;
  const int lane = threadIdx.x / wt;
  if (lane >= nq) return;
  const int col = col0 + ((int)threadIdx.x - lane * wt);
  const int b = col / c_d, j = col - b * c_d;
  const int z = blockIdx.z;
  const unsigned* const from = reinterpret_cast<const unsigned*>(drv_field(smem, struth, (size_t)G * Ws, M, z)) + (size_t)b * c_src;
  unsigned* const to = reinterpret_cast<unsigned*>(drv_field(dmem, dtruth, (size_t)G * W, M, z)) + col;
  const int o = g.op[j];
  const size_t n0 = (size_t)blockIdx.x * nq + lane, dn = (size_t)gridDim.x * nq;
  if (o == kDrvCopy) {                             // the same bits: a NaN keeps its payload
    const int ca = g.src_a[j];
    for (size_t n = n0; n < (size_t)G; n += dn) to[n * W] = from[n * Ws + ca];
    return;
  }
  if (o == kDrvSum || o == kDrvNorm) {
    const int s0 = g.tstart[3 * j], s1 = g.tstart[3 * j + 1], s2 = g.tstart[3 * j + 2];
    for (size_t n = n0; n < (size_t)G; n += dn) {
      const unsigned* const row = from + n * Ws;
      double S = drv_term_sum(row, s0, s1, q, ta, tb, nT);
      if (o == kDrvNorm) {
        const double S2 = drv_term_sum(row, s1, s2, q, ta, tb, nT);
        S = sqrt(S * S + S2 * S2);
      }
      to[n * W] = __float_as_uint((float)S);
    }
    return;
  }
  const int ca = g.src_a[j], cb = g.src_b[j];
  const double sa = g.affine[4 * j], la = g.affine[4 * j + 1], sb = g.affine[4 * j + 2], lb = g.affine[4 * j + 3];
  if (o == kDrvNorm2) {
    for (size_t n = n0; n < (size_t)G; n += dn) {
      const double u = (double)__uint_as_float(from[n * Ws + ca]) * sa + la;
      const double v = (double)__uint_as_float(from[n * Ws + cb]) * sb + lb;
      to[n * W] = __float_as_uint((float)sqrt(u * u + v * v));
    }
    return;
  }
  for (size_t n = n0; n < (size_t)G; n += dn) {      // VORTICITY, DIVERGENCE
    const int i = (int)(n / g.n_lon), l = (int)(n - (size_t)i * g.n_lon);
    if (g.pole[i]) continue;
    to[n * W] = __float_as_uint((float)drv_curl(from, Ws, i, l, o == kDrvVort, ca, cb, sa, la, sb, lb, g));
  }
}

// Pole pass of VORTICITY / DIVERGENCE: a pole is one point, so every longitude of a pole row gets the zonal mean of the
// adjacent row's double results, summed in ascending longitude by one thread (a fixed order) and divided by n_lon.
// grid = (derived columns, the two end rows, M + 1); a workgroup whose column has another op, or whose row is no pole row,
// returns at once.  Dynamic LDS: n_lon + 1 doubles.
__global__ __launch_bounds__(256) void gc_ens_derive_pole_kernel(const float* __restrict__ smem, const float* __restrict__ struth,
                                                                  float* __restrict__ dmem, float* __restrict__ dtruth, int M,
                                                                  int G, int B, int c_src, int c_d, DrvExpr g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char drv_lds[];
  double* const val = reinterpret_cast<double*>(drv_lds);
  const int col = blockIdx.x;
  const int b = col / c_d, j = col - b * c_d;
  const int o = g.op[j];
  const int i = blockIdx.y ? g.n_lat - 1 : 0;
  if ((o != kDrvVort && o != kDrvDiv) || !g.pole[i]) return;
  const int ia = i == 0 ? 1 : g.n_lat - 2;         // n_lat >= 2, and the row next to a pole row is no pole row: the plan
  const int W = B * c_d, Ws = B * c_src;
  const int z = blockIdx.z;
  const unsigned* const from = reinterpret_cast<const unsigned*>(drv_field(smem, struth, (size_t)G * Ws, M, z)) + (size_t)b * c_src;
  unsigned* const to = reinterpret_cast<unsigned*>(drv_field(dmem, dtruth, (size_t)G * W, M, z)) + col;
  const int ca = g.src_a[j], cb = g.src_b[j];
  const double sa = g.affine[4 * j], la = g.affine[4 * j + 1], sb = g.affine[4 * j + 2], lb = g.affine[4 * j + 3];
  for (int l = threadIdx.x; l < g.n_lon; l += 256) val[l] = drv_curl(from, Ws, ia, l, o == kDrvVort, ca, cb, sa, la, sb, lb, g);
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int l = 0; l < g.n_lon; ++l) s = s + val[l];
    val[g.n_lon] = s / (double)g.n_lon;
  }
  __syncthreads();
  const unsigned out = __float_as_uint((float)val[g.n_lon]);
  for (int l = threadIdx.x; l < g.n_lon; l += 256) to[((size_t)i * g.n_lon + l) * W] = out;
}

// Row pass, max (and min, on the negated values).  grid = (column tiles of wt, n_lat, fields of the chunk); wt is a power
// of two that divides 256.  Thread t owns column t % wt of longitude lane t / wt (q = 256 / wt lanes): the lanes of a wave
// own different columns at the same longitude, so their LDS addresses are consecutive.  The row tile [n_lon][wt] is staged
// once, non-finite values as -inf, and doubled IN PLACE over power-of-two spans, S_k[j] = max x[j .. j + 2^k - 1] (circular):
// every thread reads its (at most kDrvRegs) elements and their partners at distance 2^(k-1) into registers, a barrier, then
// writes.  A window of w = 2 r + 1 longitudes is the max of the two spans of length 2^k <= w that cover it: floor(log2 w)
// doubling steps of two LDS reads and a write per element, then two reads per output, whatever r is -- near the poles the
// window is the whole row.  (The prefix / suffix form of van Herk needs two more arrays and a row extended past the wrap;
// the doubling form needs the staged tile only.)  out [chunk][G][W]: the pooled row in the max domain, -inf where no
// finite value.
__global__ __launch_bounds__(256) void gc_ens_pool_row_max_kernel(const float* __restrict__ mem, const float* __restrict__ truth,
                                                                   size_t field, int M, int z0, int n_lon, int W, int wt,
                                                                   const int* __restrict__ r_lon, int negate,
                                                                   float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char drv_lds[];
  float* const S = reinterpret_cast<float*>(drv_lds);
  const int q = 256 / wt;
  const int tid = threadIdx.x;
  const int lane = tid / wt;
  const int cl = tid - lane * wt;
  const int col = blockIdx.x * wt + cl;
  const bool live = col < W;
  const int i = blockIdx.y;
  const float* const row = drv_field(mem, truth, field, M, z0 + (int)blockIdx.z) + (size_t)i * n_lon * W + col;
  const float ninf = -__builtin_inff();
  for (int j = lane; j < n_lon; j += q) {
    float x = live ? row[(size_t)j * W] : ninf;
    if (negate) x = -x;
    S[j * wt + cl] = isfinite(x) ? x : ninf;
  }
  __syncthreads();
  const int r = r_lon[i], w = 2 * r + 1;
  int span = 1;
  while (2 * span <= w) {                          // S_k -> S_(k+1), span = 2^k
    float v[kDrvRegs];
#pragma unroll
    for (int e = 0; e < kDrvRegs; ++e) {
      const int j = lane + e * q;
      if (j < n_lon) {
        int j2 = j + span;
        if (j2 >= n_lon) j2 -= n_lon;
        v[e] = fmaxf(S[j * wt + cl], S[j2 * wt + cl]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kDrvRegs; ++e) {
      const int j = lane + e * q;
      if (j < n_lon) S[j * wt + cl] = v[e];
    }
    __syncthreads();
    span *= 2;
  }
  if (!live) return;
  float* const o = out + ((size_t)blockIdx.z * gridDim.y + i) * n_lon * W + col;
  for (int j = lane; j < n_lon; j += q) {
    int a = j - r;
    if (a < 0) a += n_lon;
    int b = j + r - span + 1;                      // in (-n_lon, n_lon): span <= w <= n_lon
    if (b < 0) b += n_lon;
    o[(size_t)j * W] = fmaxf(S[a * wt + cl], S[b * wt + cl]);
  }
}

// Row pass, mean.  The same grid and thread layout.  Dynamic LDS: double P[n_lon][wt], the inclusive prefix sum of the
// finite values along the row, then int C[n_lon][wt], the prefix count.  Lane l scans its contiguous segment of
// ceil(n_lon / q) longitudes, reads the totals of the segments in front of it (ascending: a fixed order), a barrier, and
// adds them to its segment.  A window is the difference of two prefix values (three where it wraps): the cost per output
// does not depend on r.  sum [chunk][G][W] double, cnt [chunk][G][W] int.
__global__ __launch_bounds__(256) void gc_ens_pool_row_mean_kernel(const float* __restrict__ mem, const float* __restrict__ truth,
                                                                    size_t field, int M, int z0, int n_lon, int W, int wt,
                                                                    const int* __restrict__ r_lon, double* __restrict__ sum,
                                                                    int* __restrict__ cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char drv_lds[];
  double* const P = reinterpret_cast<double*>(drv_lds);
  int* const C = reinterpret_cast<int*>(P + (size_t)n_lon * wt);
  const int q = 256 / wt;
  const int tid = threadIdx.x;
  const int lane = tid / wt;
  const int cl = tid - lane * wt;
  const int col = blockIdx.x * wt + cl;
  const bool live = col < W;
  const int i = blockIdx.y;
  const float* const row = drv_field(mem, truth, field, M, z0 + (int)blockIdx.z) + (size_t)i * n_lon * W + col;
  const int seg = (n_lon + q - 1) / q;
  const int j0 = min(n_lon, lane * seg), j1 = min(n_lon, j0 + seg);
  double s = 0.0;
  int c = 0;
  for (int j = j0; j < j1; ++j) {
    const float x = live ? row[(size_t)j * W] : 0.f;
    if (isfinite(x)) {
      s += (double)x;
      ++c;
    }
    P[j * wt + cl] = s;
    C[j * wt + cl] = c;
  }
  __syncthreads();
  double ps = 0.0;
  int pc = 0;
  for (int l = 0; l < lane; ++l) {                 // the segments in front of this one, ascending
    const int e = min(n_lon, (l + 1) * seg);
    if (e > l * seg) {
      ps += P[(e - 1) * wt + cl];
      pc += C[(e - 1) * wt + cl];
    }
  }
  __syncthreads();
  for (int j = j0; j < j1; ++j) {
    P[j * wt + cl] += ps;
    C[j * wt + cl] += pc;
  }
  __syncthreads();
  if (!live) return;
  const int r = r_lon[i];
  const size_t base = ((size_t)blockIdx.z * gridDim.y + i) * n_lon * W + col;
  const double tot = P[(n_lon - 1) * wt + cl];
  const int ctot = C[(n_lon - 1) * wt + cl];
  for (int j = lane; j < n_lon; j += q) {
    const int lo = j - r, hi = j + r;              // 2 r + 1 <= n_lon: the window wraps at one end at the most
    double ws;
    int wc;
    if (lo < 0) {
      ws = (tot - P[(lo + n_lon - 1) * wt + cl]) + P[hi * wt + cl];
      wc = (ctot - C[(lo + n_lon - 1) * wt + cl]) + C[hi * wt + cl];
    } else if (hi >= n_lon) {
      ws = (tot - P[(lo - 1) * wt + cl]) + P[(hi - n_lon) * wt + cl];
      wc = (ctot - C[(lo - 1) * wt + cl]) + C[(hi - n_lon) * wt + cl];
    } else {
      ws = P[hi * wt + cl] - (lo > 0 ? P[(lo - 1) * wt + cl] : 0.0);
      wc = C[hi * wt + cl] - (lo > 0 ? C[(lo - 1) * wt + cl] : 0);
    }
    sum[base + (size_t)j * W] = ws;
    cnt[base + (size_t)j * W] = wc;
  }
}

// Column pass: a stream over the points of the chunk's fields, one thread per point.  The at most 2 r_lat + 1 intermediates
// above and below lie n_lon W elements apart (coalesced across the wave, L2 hits between neighbouring rows); the centre is
// read from, and the result written over, the thread's own element of the destination field.
template <int POOL>
__global__ __launch_bounds__(256) void gc_ens_pool_col_kernel(float* __restrict__ mem, float* __restrict__ truth, size_t field,
                                                               int M, int z0, int n_lat, size_t rowlen, int r_lat,
                                                               const float* __restrict__ rmax, const double* __restrict__ rsum,
                                                               const int* __restrict__ rcnt,
                                                               const double* __restrict__ row_weight) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= field) return;
  float* const f = drv_field(mem, truth, field, M, z0 + (int)blockIdx.y);
  const int i = (int)(p / rowlen);
  const int i0 = max(0, i - r_lat), i1 = min(n_lat - 1, i + r_lat);
  const size_t at = (size_t)blockIdx.y * field + p - (size_t)(i - i0) * rowlen;
  float out;
  if constexpr (POOL == kPoolMean) {
    double num = 0.0, den = 0.0;
    for (int k = i0; k <= i1; ++k) {
      const size_t e = at + (size_t)(k - i0) * rowlen;
      const double w = row_weight[k];
      num += w * rsum[e];
      den += w * (double)rcnt[e];
    }
    out = (float)(num / den);
  } else {
    float m = -__builtin_inff();
    for (int k = i0; k <= i1; ++k) m = fmaxf(m, rmax[at + (size_t)(k - i0) * rowlen]);
    out = POOL == kPoolMin ? -m : m;
  }
  if (!isfinite(f[p])) out = __builtin_nanf("");
  f[p] = out;
}

static int drv_pow2_floor(int v) {
  int p = 1;
  while (2 * p <= v) p *= 2;
  return p;
}

// columns of a row tile: a power of two, within the LDS budget, no wider than the field needs; 0: the row does not fit
static int drv_tile(int pool, int n_lon, int W) {
  const size_t per = (size_t)n_lon * (pool == kPoolMean ? kDrvMeanBytes : 4);
  if (per > kDrvRowLds) return 0;
  int wt = std::min(kDrvMaxTile, drv_pow2_floor((int)(kDrvRowLds / per)));
  while (wt / 2 >= W) wt /= 2;
  return wt;
}

// node blocks of the point pass: q nodes each per trip of its grid-stride walk, at most 1024
static int drv_point_blocks(int G, int W) {
  const int q = 256 / std::min(256, W);
  return std::max(1, std::min(1024, (G + q - 1) / q));
}

static hipError_t launch_ens_derive(hipStream_t s, const float* smem, const float* struth, float* dmem, float* dtruth, int M,
                                    int G, int B, int c_src, int c_d, const int* op, const int* src_a, const int* src_b,
                                    const double* affine) {
  const int W = B * c_d;
  const int blocks = drv_point_blocks(G, W);
  hipLaunchKernelGGL(gc_ens_derive_kernel, dim3(blocks, (W + 255) / 256, M + 1), dim3(256), 0, s, smem, struth, dmem, dtruth, M,
                     G, B, c_src, c_d, op, src_a, src_b, affine);
  return hipGetLastError();
}

static hipError_t launch_ens_derive_expr(hipStream_t s, const float* smem, const float* struth, float* dmem, float* dtruth, int M,
                                         int G, int B, int c_src, int c_d, const DrvExpr& g) {
  const int W = B * c_d;
  const int blocks = drv_point_blocks(G, W);
  hipLaunchKernelGGL(gc_ens_derive_expr_kernel, dim3(blocks, (W + 255) / 256, M + 1), dim3(256), (size_t)g.n_terms * kDrvTermBytes,
                     s, smem, struth, dmem, dtruth, M, G, B, c_src, c_d, g);
  return hipGetLastError();
}

static hipError_t launch_ens_derive_pole(hipStream_t s, const float* smem, const float* struth, float* dmem, float* dtruth, int M,
                                         int G, int B, int c_src, int c_d, const DrvExpr& g) {
  const int W = B * c_d;
  hipLaunchKernelGGL(gc_ens_derive_pole_kernel, dim3(W, 2, M + 1), dim3(256), (size_t)(g.n_lon + 1) * sizeof(double), s, smem,
                     struth, dmem, dtruth, M, G, B, c_src, c_d, g);
  return hipGetLastError();
}

static hipError_t launch_ens_pool_row(hipStream_t s, int pool, const float* mem, const float* truth, size_t field, int M, int z0,
                                      int nz, int n_lat, int n_lon, int W, const int* r_lon, void* inter) {
  const int wt = drv_tile(pool, n_lon, W);
  const dim3 grid((W + wt - 1) / wt, n_lat, nz);
  if (pool == kPoolMean) {
    double* const sum = reinterpret_cast<double*>(inter);
    int* const cnt = reinterpret_cast<int*>(sum + (size_t)kDrvChunk * field);
    hipLaunchKernelGGL(gc_ens_pool_row_mean_kernel, grid, dim3(256), (size_t)n_lon * wt * kDrvMeanBytes, s, mem, truth, field, M,
                       z0, n_lon, W, wt, r_lon, sum, cnt);
  } else {
    hipLaunchKernelGGL(gc_ens_pool_row_max_kernel, grid, dim3(256), (size_t)n_lon * wt * sizeof(float), s, mem, truth, field, M,
                       z0, n_lon, W, wt, r_lon, pool == kPoolMin ? 1 : 0, reinterpret_cast<float*>(inter));
  }
  return hipGetLastError();
}

static hipError_t launch_ens_pool_col(hipStream_t s, int pool, float* mem, float* truth, size_t field, int M, int z0, int nz,
                                      int n_lat, int n_lon, int W, int r_lat, void* inter, const double* row_weight) {
  const dim3 grid((unsigned)((field + 255) / 256), nz);
  const size_t rowlen = (size_t)n_lon * W;
  float* const rmax = reinterpret_cast<float*>(inter);
  double* const rsum = reinterpret_cast<double*>(inter);
  int* const rcnt = reinterpret_cast<int*>(rsum + (size_t)kDrvChunk * field);
  if (pool == kPoolMean)
    hipLaunchKernelGGL((gc_ens_pool_col_kernel<kPoolMean>), grid, dim3(256), 0, s, mem, truth, field, M, z0, n_lat, rowlen, r_lat,
                       nullptr, rsum, rcnt, row_weight);
  else if (pool == kPoolMin)
    hipLaunchKernelGGL((gc_ens_pool_col_kernel<kPoolMin>), grid, dim3(256), 0, s, mem, truth, field, M, z0, n_lat, rowlen, r_lat,
                       rmax, nullptr, nullptr, row_weight);
  else
    hipLaunchKernelGGL((gc_ens_pool_col_kernel<kPoolMax>), grid, dim3(256), 0, s, mem, truth, field, M, z0, n_lat, rowlen, r_lat,
                       rmax, nullptr, nullptr, row_weight);
  return hipGetLastError();
}

}  // namespace gc

using namespace gci;

extern "C" {

int gc_ens_derive_set(gc_handle* h, int32_t c_src, const int32_t* op, const int32_t* src_a, const int32_t* src_b,
                      const double* affine, int32_t pool, int32_t n_lat, int32_t n_lon, int32_t r_lat, const int32_t* r_lon,
                      const double* row_weight) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (pool < gc::kPoolNone || pool > gc::kPoolMean) return fail(h, GC_ERR_UNSUPPORTED, "pool must be 0 (none), 1 (max), 2 (min) or 3 (mean)");
  if (!op || !src_a || !src_b || !affine || (pool != gc::kPoolNone && (!r_lon || !row_weight)))
    return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (c_src < 1) return fail(h, GC_ERR_INVALID_ARGUMENT, "c_src must be positive");
  if (n_lat < 1 || n_lon < 1 || (int64_t)n_lat * n_lon != (int64_t)h->hg.G)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "n_lat * n_lon must equal the number of grid nodes");
  const int c_d = h->cfg.c_out, W = h->cfg.batch * c_d;
  for (int j = 0; j < c_d; ++j) {
    if (op[j] != gc::kDrvCopy && op[j] != gc::kDrvNorm2) return fail(h, GC_ERR_UNSUPPORTED, "op " + std::to_string(j) + " is neither 0 (copy) nor 1 (norm2)");
    if (src_a[j] < 0 || src_a[j] >= c_src || (op[j] == gc::kDrvNorm2 && (src_b[j] < 0 || src_b[j] >= c_src)))
      return fail(h, GC_ERR_INVALID_ARGUMENT, "derived channel " + std::to_string(j) + ": source channel outside [0, c_src)");
  }
  if (r_lat < 0) return fail(h, GC_ERR_INVALID_ARGUMENT, "r_lat is negative");
  if (pool != gc::kPoolNone) {
    for (int i = 0; i < n_lat; ++i) {
      if (r_lon[i] < 0 || r_lon[i] > (n_lon - 1) / 2) return fail(h, GC_ERR_INVALID_ARGUMENT, "r_lon[" + std::to_string(i) + "] outside 0 .. (n_lon - 1) / 2");
      if (!(std::isfinite(row_weight[i]) && row_weight[i] > 0.0)) return fail(h, GC_ERR_INVALID_ARGUMENT, "row_weight[" + std::to_string(i) + "] is not finite and positive");
    }
    if (gc::drv_tile(pool, n_lon, W) == 0) return fail(h, GC_ERR_UNSUPPORTED, "n_lon is too large for the row tile of this pool (64 KB of LDS)");
  }
  GC_HIP(h, hipSetDevice(h->device));
  // one blob: affine [c_d][4] and row_weight [n_lat] doubles, then op, src_a, src_b [c_d] and r_lon [n_lat] int32
  const size_t n_d = (size_t)4 * c_d + n_lat, n_i = (size_t)3 * c_d + n_lat;
  std::vector<double> blob(n_d + (n_i + 1) / 2);
  std::copy(affine, affine + 4 * c_d, blob.begin());
  for (int i = 0; i < n_lat; ++i) blob[(size_t)4 * c_d + i] = pool != gc::kPoolNone ? row_weight[i] : 1.0;
  int32_t* const ib = reinterpret_cast<int32_t*>(blob.data() + n_d);
  for (int j = 0; j < c_d; ++j) {
    ib[j] = op[j];
    ib[c_d + j] = src_a[j];
    ib[2 * c_d + j] = op[j] == gc::kDrvNorm2 ? src_b[j] : src_a[j];
  }
  for (int i = 0; i < n_lat; ++i) ib[3 * c_d + i] = pool != gc::kPoolNone ? r_lon[i] : 0;
  GC_HIP(h, h->drv_allocs.drop(h->stream));          // nothing reads the old plan any more
  h->drv_set = false;
  int rc;
  double* d_blob = nullptr;
  if ((rc = dev_alloc(h, &d_blob, blob.size(), &h->drv_allocs))) return rc;
  GC_HIP(h, h->ev_drv_src.ensure());
  if ((rc = store_upload(h, d_blob, blob.data(), blob.size() * sizeof(double)))) return rc;
  h->d_drv_affine = d_blob;
  h->d_drv_roww = d_blob + (size_t)4 * c_d;
  h->d_drv_op = reinterpret_cast<int*>(d_blob + n_d);
  h->d_drv_a = h->d_drv_op + c_d;
  h->d_drv_b = h->d_drv_a + c_d;
  h->d_drv_rlon = h->d_drv_b + c_d;
  h->drv_c_src = c_src;
  h->drv_pool = pool;
  h->drv_n_lat = n_lat;
  h->drv_n_lon = n_lon;
  h->drv_r_lat = r_lat;
  h->drv_expr = false;
  h->drv_set = true;
  return GC_OK;
  });
}

int gc_ens_derive_set_expr(gc_handle* h, int32_t c_src, const int32_t* op, const int32_t* src_a, const int32_t* src_b,
                           const double* affine, int32_t pool, int32_t n_lat, int32_t n_lon, int32_t r_lat, const int32_t* r_lon,
                           const double* row_weight, const double* scale, const double* loc, const int32_t* term_start,
                           int32_t n_terms, const double* term_coef, const int32_t* term_a, const int32_t* term_b,
                           const double* coslat, const double* inv_rcos, const double* inv_dphi, double inv_2dlam,
                           const int32_t* pole_row) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (pool < gc::kPoolNone || pool > gc::kPoolMean) return fail(h, GC_ERR_UNSUPPORTED, "pool must be 0 (none), 1 (max), 2 (min) or 3 (mean)");
  if (!op || !src_a || !src_b || !affine || !scale || !loc || (pool != gc::kPoolNone && (!r_lon || !row_weight)))
    return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (c_src < 1) return fail(h, GC_ERR_INVALID_ARGUMENT, "c_src must be positive");
  if (n_lat < 1 || n_lon < 1 || (int64_t)n_lat * n_lon != (int64_t)h->hg.G)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "n_lat * n_lon must equal the number of grid nodes");
  for (int c = 0; c < c_src; ++c)
    if (!std::isfinite(scale[c]) || !std::isfinite(loc[c])) return fail(h, GC_ERR_INVALID_ARGUMENT, "scale / loc of source channel " + std::to_string(c) + " is not finite");
  if (n_terms < 0) return fail(h, GC_ERR_INVALID_ARGUMENT, "n_terms is negative");
  if (n_terms > gc::kDrvPlanTerms) return fail(h, GC_ERR_UNSUPPORTED, "more than " + std::to_string(gc::kDrvPlanTerms) + " terms in one plan");
  if (n_terms > 0 && (!term_coef || !term_a || !term_b)) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  for (int t = 0; t < n_terms; ++t) {
    if (!std::isfinite(term_coef[t])) return fail(h, GC_ERR_INVALID_ARGUMENT, "the coefficient of term " + std::to_string(t) + " is not finite");
    if (term_a[t] < 0 || term_a[t] >= c_src || term_b[t] < -1 || term_b[t] >= c_src)
      return fail(h, GC_ERR_INVALID_ARGUMENT, "term " + std::to_string(t) + ": source channel outside [0, c_src)");
  }
  const int c_d = h->cfg.c_out, W = h->cfg.batch * c_d;
  bool curl = false;
  for (int j = 0; j < c_d; ++j) {
    const std::string who = "derived channel " + std::to_string(j);
    if (op[j] < gc::kDrvCopy || op[j] > gc::kDrvDiv)
      return fail(h, GC_ERR_UNSUPPORTED, "op " + std::to_string(j) + " is none of 0 (copy), 1 (norm2), 2 (sum), 3 (norm), 4 (vorticity), 5 (divergence)");
    if (op[j] == gc::kDrvSum || op[j] == gc::kDrvNorm) {
      if (!term_start) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
      const int s0 = term_start[3 * j], s1 = term_start[3 * j + 1], s2 = term_start[3 * j + 2];
      if (s0 < 0 || s1 <= s0 || s2 < s1 || s2 > n_terms || (s2 > s1) != (op[j] == gc::kDrvNorm))
        return fail(h, GC_ERR_INVALID_ARGUMENT, who + ": a sum takes one list of terms inside the table, a norm two, none of them empty");
      if (s1 - s0 > gc::kDrvListTerms || s2 - s1 > gc::kDrvListTerms)
        return fail(h, GC_ERR_UNSUPPORTED, who + ": more than " + std::to_string(gc::kDrvListTerms) + " terms in one list");
      continue;
    }
    curl = curl || op[j] >= gc::kDrvVort;
    if (src_a[j] < 0 || src_a[j] >= c_src || (op[j] != gc::kDrvCopy && (src_b[j] < 0 || src_b[j] >= c_src)))
      return fail(h, GC_ERR_INVALID_ARGUMENT, who + ": source channel outside [0, c_src)");
  }
  bool poles = false;
  if (curl) {
    if (!coslat || !inv_rcos || !inv_dphi || !pole_row) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_lon < 3 || n_lat < 2) return fail(h, GC_ERR_INVALID_ARGUMENT, "vorticity and divergence need n_lon >= 3 and n_lat >= 2");
    if (!(std::isfinite(inv_2dlam) && inv_2dlam != 0.0)) return fail(h, GC_ERR_INVALID_ARGUMENT, "1 / (2 dlambda) is not finite and non-zero");
    for (int i = 0; i < n_lat; ++i) {
      const std::string row = "row " + std::to_string(i);
      if (!std::isfinite(coslat[i]) || !(std::isfinite(inv_dphi[i]) && inv_dphi[i] != 0.0))
        return fail(h, GC_ERR_INVALID_ARGUMENT, row + ": cos(lat) or 1 / dphi is not finite (or 1 / dphi is zero)");
      if (pole_row[i]) {
        const int next = i == 0 ? 1 : n_lat - 2;
        if ((i != 0 && i != n_lat - 1) || coslat[i] != 0.0 || pole_row[next])
          return fail(h, GC_ERR_INVALID_ARGUMENT, row + ": a pole row is an end row with cos(lat) = 0 next to a row that is none");
        poles = true;
      } else if (!std::isfinite(inv_rcos[i])) {
        return fail(h, GC_ERR_INVALID_ARGUMENT, row + ": 1 / (R cos(lat)) is not finite");
      }
    }
    if (poles && n_lon > gc::kDrvPoleLon) return fail(h, GC_ERR_UNSUPPORTED, "n_lon is too large for the pole pass (64 KB of LDS)");
  }
  if (r_lat < 0) return fail(h, GC_ERR_INVALID_ARGUMENT, "r_lat is negative");
  if (pool != gc::kPoolNone) {
    for (int i = 0; i < n_lat; ++i) {
      if (r_lon[i] < 0 || r_lon[i] > (n_lon - 1) / 2) return fail(h, GC_ERR_INVALID_ARGUMENT, "r_lon[" + std::to_string(i) + "] outside 0 .. (n_lon - 1) / 2");
      if (!(std::isfinite(row_weight[i]) && row_weight[i] > 0.0)) return fail(h, GC_ERR_INVALID_ARGUMENT, "row_weight[" + std::to_string(i) + "] is not finite and positive");
    }
    if (gc::drv_tile(pool, n_lon, W) == 0) return fail(h, GC_ERR_UNSUPPORTED, "n_lon is too large for the row tile of this pool (64 KB of LDS)");
  }
  GC_HIP(h, hipSetDevice(h->device));
  // one blob.  doubles: affine [c_d][4], row_weight [n_lat], the term table [5][n_terms], the row tables [3][n_lat];
  // int32: op, src_a, src_b [c_d], r_lon [n_lat], term_start [c_d][3], term_a, term_b [n_terms], pole_row [n_lat]
  const size_t nT = (size_t)n_terms;
  const size_t o_roww = (size_t)4 * c_d, o_tq = o_roww + n_lat, o_rows = o_tq + 5 * nT, n_d = o_rows + (size_t)3 * n_lat;
  const size_t i_rlon = (size_t)3 * c_d, i_ts = i_rlon + n_lat, i_ta = i_ts + (size_t)3 * c_d, i_tb = i_ta + nT, i_pole = i_tb + nT,
               n_i = i_pole + n_lat;
  std::vector<double> blob(n_d + (n_i + 1) / 2);
  int32_t* const ib = reinterpret_cast<int32_t*>(blob.data() + n_d);
  for (int j = 0; j < c_d; ++j) {
    const bool pair = op[j] == gc::kDrvNorm2 || op[j] >= gc::kDrvVort, list = op[j] == gc::kDrvSum || op[j] == gc::kDrvNorm;
    const int a = list ? 0 : src_a[j], b = pair ? src_b[j] : a;
    ib[j] = op[j];
    ib[c_d + j] = a;
    ib[2 * c_d + j] = b;
    for (int k = 0; k < 3; ++k) ib[i_ts + 3 * j + k] = list ? term_start[3 * j + k] : 0;
    double* const aff = blob.data() + 4 * j;
    if (op[j] >= gc::kDrvVort) {                     // (su, lu, sv, lv): the components in physical units
      aff[0] = scale[a], aff[1] = loc[a], aff[2] = scale[b], aff[3] = loc[b];
    } else {
      std::copy(affine + 4 * j, affine + 4 * j + 4, aff);
    }
  }
  for (int i = 0; i < n_lat; ++i) {
    blob[o_roww + i] = pool != gc::kPoolNone ? row_weight[i] : 1.0;
    ib[i_rlon + i] = pool != gc::kPoolNone ? r_lon[i] : 0;
    blob[o_rows + i] = curl ? coslat[i] : 0.0;
    blob[o_rows + n_lat + i] = curl && !pole_row[i] ? inv_rcos[i] : 0.0;
    blob[o_rows + 2 * (size_t)n_lat + i] = curl ? inv_dphi[i] : 0.0;
    ib[i_pole + i] = curl && pole_row[i] ? 1 : 0;
  }
  for (size_t t = 0; t < nT; ++t) {
    const int a = term_a[t], b = term_b[t];
    blob[o_tq + t] = term_coef[t];
    blob[o_tq + nT + t] = scale[a];
    blob[o_tq + 2 * nT + t] = loc[a];
    blob[o_tq + 3 * nT + t] = b >= 0 ? scale[b] : 1.0;
    blob[o_tq + 4 * nT + t] = b >= 0 ? loc[b] : 0.0;
    ib[i_ta + t] = a;
    ib[i_tb + t] = b;
  }
  GC_HIP(h, h->drv_allocs.drop(h->stream));          // nothing reads the old plan any more
  h->drv_set = false;
  int rc;
  double* d_blob = nullptr;
  if ((rc = dev_alloc(h, &d_blob, blob.size(), &h->drv_allocs))) return rc;
  GC_HIP(h, h->ev_drv_src.ensure());
  if ((rc = store_upload(h, d_blob, blob.data(), blob.size() * sizeof(double)))) return rc;
  int* const d_ib = reinterpret_cast<int*>(d_blob + n_d);
  h->d_drv_affine = d_blob;
  h->d_drv_roww = d_blob + o_roww;
  h->d_drv_tq = d_blob + o_tq;
  h->d_drv_rows = d_blob + o_rows;
  h->d_drv_op = d_ib;
  h->d_drv_a = d_ib + c_d;
  h->d_drv_b = d_ib + 2 * c_d;
  h->d_drv_rlon = d_ib + i_rlon;
  h->d_drv_tstart = d_ib + i_ts;
  h->d_drv_ta = d_ib + i_ta;
  h->d_drv_tb = d_ib + i_tb;
  h->d_drv_pole = d_ib + i_pole;
  h->drv_n_terms = n_terms;
  h->drv_inv_2dlam = curl ? inv_2dlam : 0.0;
  h->drv_poles = poles;
  h->drv_c_src = c_src;
  h->drv_pool = pool;
  h->drv_n_lat = n_lat;
  h->drv_n_lon = n_lon;
  h->drv_r_lat = r_lat;
  h->drv_expr = true;
  h->drv_set = true;
  return GC_OK;
  });
}

int gc_ens_derive(gc_handle* h, gc_handle* src, const float* truth) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_source(h, src)) || (rc = need_graph(h)) || (rc = need(h, h->drv_set, "no plan (gc_ens_derive_set)"))) return rc;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, B = c.batch, c_d = c.c_out, W = B * c_d, pool = h->drv_pool, M = h->ens_members;
  const size_t field = field_len(h);
  const int chunk = std::min(gc::kDrvChunk, M + 1);
  // the intermediate of a pooled plan, sized by the pool kind and the field
  const size_t bytes = pool == gc::kPoolNone ? 0 : (size_t)gc::kDrvChunk * field * (pool == gc::kPoolMean ? gc::kDrvMeanBytes : 4);
  rc = fill_open(h, src, h->drv_c_src, truth, "gc_ens_derive", h->ev_drv_src,
                 [&] { return bytes ? sized_for(h, h->drv_work_allocs, {bytes}, buf(&h->d_drv_work, bytes)) : GC_OK; });
  if (rc) return rc;
  hipStream_t s = h->stream;
  const int n_lat = h->drv_n_lat;
  const gc::DrvExpr g{h->d_drv_op, h->d_drv_a, h->d_drv_b, h->d_drv_affine, h->d_drv_tstart, h->d_drv_tq, h->d_drv_ta, h->d_drv_tb,
                      h->d_drv_rows, h->d_drv_rows + n_lat, h->d_drv_rows + 2 * (size_t)n_lat, h->d_drv_pole, h->drv_inv_2dlam,
                      h->drv_n_terms, n_lat, h->drv_n_lon};      // read by the plans of gc_ens_derive_set_expr only
  rc = timed(h, h->drv,
             [&]() -> int {
               if ((rc = launch_each(h, [&] {
                     if (h->drv_expr)
                       return gc::launch_ens_derive_expr(s, src->d_ens, src->d_ens_truth, h->d_ens, h->d_ens_truth, M, G, B,
                                                         src->cfg.c_out, c_d, g);
                     return gc::launch_ens_derive(s, src->d_ens, src->d_ens_truth, h->d_ens, h->d_ens_truth, M, G, B, src->cfg.c_out,
                                                  c_d, h->d_drv_op, h->d_drv_a, h->d_drv_b, h->d_drv_affine);
                   })))
                 return rc;
               if (h->drv_expr && h->drv_poles && (rc = launch_each(h, [&] {
                     return gc::launch_ens_derive_pole(s, src->d_ens, src->d_ens_truth, h->d_ens, h->d_ens_truth, M, G, B,
                                                       src->cfg.c_out, c_d, g);
                   })))
                 return rc;
               if (pool == gc::kPoolNone) return GC_OK;
               for (int z0 = 0; z0 <= M; z0 += chunk) {
                 const int nz = std::min(chunk, M + 1 - z0);
                 if ((rc = launch_each(h,
                          [&] {
                            return gc::launch_ens_pool_row(s, pool, h->d_ens, h->d_ens_truth, field, M, z0, nz, h->drv_n_lat,
                                                           h->drv_n_lon, W, h->d_drv_rlon, h->d_drv_work);
                          },
                          [&] {
                            return gc::launch_ens_pool_col(s, pool, h->d_ens, h->d_ens_truth, field, M, z0, nz, h->drv_n_lat,
                                                           h->drv_n_lon, W, h->drv_r_lat, h->d_drv_work, h->d_drv_roww);
                          })))
                   return rc;
               }
               return GC_OK;
             },
             no_readbacks);
  if (rc) return rc;
  h->drv.blocks = gc::drv_point_blocks(G, W);
  fill_close(h);
  return GC_OK;
  });
}

}  // extern "C"
