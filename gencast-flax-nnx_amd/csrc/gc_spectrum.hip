// Spherical-harmonic power spectra on the device (include/gencast_hip.h, gc_spec_* / gc_ens_spectrum): the analysis
// direction of the transform gc_noise.hip synthesises with, and the reductions on top of it.  Kernels and their host code
// live together here; DESIGN.md section 8d has the definitions and the error bound the tests assert.
//
// A field is [n_lat][n_lon][N] float32, N = B c_out independent columns.  With the float32 tables T (cosine and sine rows,
// amp_m / n_lon folded in) and Q (the pseudo-inverse of the Legendre synthesis matrix of every m, zero for l < m):
//   Fourier step   F[part][m][lat][n] = sum_j   T[part][m][j] f[lat][j][n]          j ascending
//   Legendre step  a[part][m][l][n]   = sum_lat Q[m][l][lat] F[part][m][lat][n]     lat ascending
//   power          p[n][l]            = (sum_m a[0][m][l][n]^2 + a[1][m][l][n]^2) / (4 pi)   m ascending, cosine then sine
// Every product and sum is binary64.  The Fourier products are exact (float32 x float32), so fused and unfused
// multiply-adds give the same bits there; the Legendre step uses fused multiply-adds (one rounding per term); the
// squares of the power step are rounded before they are added.  Every sum has one writer and a fixed order; the only
// atomics are integer ORs into the per-column "not finite" flags, which commute.  Both products run on the vector ALUs
// (as gc_noise_* do): a wave keeps 16 output rows of one 64-column group in registers, its table values are
// wave-uniform and come through the scalar cache.
#include "gc_store.h"

namespace gc {

constexpr int kSpecRows = 16;                    // output rows (wavenumbers) a wave accumulates
constexpr int kSpecBlockRows = 4 * kSpecRows;    // per workgroup of 4 waves
constexpr double kFourPi = 12.566370614359172;   // 4 pi, as the host's 4.0 * pi rounds

// Fourier step.  grid = (n_lat, ceil(2 L / 64), ceil(N / 64)); lane = column.  Row r < L is the cosine row of m = r,
// row L + m the sine row.  The workgroups of row block 0 also note a value that is not finite in flags[n].
__global__ __launch_bounds__(256) void gc_spec_fourier_kernel(const float* __restrict__ f,      // [n_lat][n_lon][N]
                                                               const float* __restrict__ tab,    // [2 L][n_lon]
                                                               int L, int n_lat, int n_lon, int N,
                                                               double* __restrict__ F,           // [2 L][n_lat][N]
                                                               unsigned* __restrict__ flags) {   // [N]
  const int lat = blockIdx.x, R = 2 * L;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int n = blockIdx.z * 64 + lane;
  const int r0 = blockIdx.y * kSpecBlockRows + wave * kSpecRows;
  if (r0 >= R) return;
  const float* trow[kSpecRows];
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k) trow[k] = tab + (size_t)min(r0 + k, R - 1) * n_lon;
  double acc[kSpecRows];
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k) acc[k] = 0.0;
  const float* frow = f + (size_t)lat * n_lon * N + min(n, N - 1);
  bool bad = false;
  for (int j = 0; j < n_lon; ++j) {
    const float xf = frow[(size_t)j * N];
    bad = bad || !isfinite(xf);
    const double x = (double)xf;
#pragma unroll
    for (int k = 0; k < kSpecRows; ++k) acc[k] = fma((double)trow[k][j], x, acc[k]);
  }
  if (n >= N) return;
  if (bad && r0 == 0) atomicOr(&flags[n], 1u);
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k)
    if (r0 + k < R) F[((size_t)(r0 + k) * n_lat + lat) * N + n] = acc[k];
}

// Legendre step.  grid = (L, 2 ceil(L / 64), ceil(N / 64)): blockIdx.x = m, blockIdx.y = part + 2 (block of 64 l).  A wave
// whose 16 l are all below m has nothing to do (those coefficients do not exist and are never read).
__global__ __launch_bounds__(256) void gc_spec_legendre_kernel(const float* __restrict__ Q,      // [L m][L l][n_lat]
                                                                const double* __restrict__ F,     // [2][L][n_lat][N]
                                                                int L, int n_lat, int N,
                                                                double* __restrict__ coef) {      // [2][L m][L l][N]
  const int m = blockIdx.x, part = blockIdx.y & 1;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int n = blockIdx.z * 64 + lane;
  const int l0 = (blockIdx.y >> 1) * kSpecBlockRows + wave * kSpecRows;
  if (l0 >= L || l0 + kSpecRows <= m) return;
  const float* qrow[kSpecRows];
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k) qrow[k] = Q + ((size_t)m * L + min(l0 + k, L - 1)) * n_lat;
  double acc[kSpecRows];
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k) acc[k] = 0.0;
  const double* fcol = F + ((size_t)part * L + m) * n_lat * N + min(n, N - 1);
  for (int lat = 0; lat < n_lat; ++lat) {
    const double x = fcol[(size_t)lat * N];
#pragma unroll
    for (int k = 0; k < kSpecRows; ++k) acc[k] = fma((double)qrow[k][lat], x, acc[k]);
  }
  if (n >= N) return;
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k)
    if (l0 + k < L) coef[(((size_t)part * L + m) * L + l0 + k) * N + n] = acc[k];
}

#pragma clang fp contract(off)   // from here on a square is rounded before it is added: the order the header states

// sum_m (c^2 + s^2) / (4 pi) of the coefficients u - v (v may be null), m ascending, cosine before sine
__device__ __forceinline__ double spec_power_of(const double* __restrict__ u, const double* __restrict__ v, int L, int N,
                                                int l, int n) {
  const size_t part = (size_t)L * L * N, step = (size_t)L * N;
  size_t e = (size_t)l * N + n;
  double s = 0.0;
  for (int m = 0; m <= l; ++m, e += step) {
    const double c = v ? u[e] - v[e] : u[e];
    const double d = v ? u[part + e] - v[part + e] : u[part + e];
    s += c * c;
    s += d * d;
  }
  return s / kFourPi;
}

// One thread per (l, n).  out [N][L]: the power of one coefficient set; NaN for a flagged column.
__global__ __launch_bounds__(256) void gc_spec_power_kernel(const double* __restrict__ coef, const unsigned* __restrict__ flags,
                                                             int L, int N, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= L * N) return;
  const int l = i / N, n = i - l * N;
  out[(size_t)n * L + l] = flags[n] ? __builtin_nan("") : spec_power_of(coef, nullptr, L, N, l, n);
}

// Mean coefficients: mean = (sum_i set_i) / M, members in ascending slot order, on every (part, m, l >= m, n).
__global__ __launch_bounds__(256) void gc_spec_mean_kernel(const double* __restrict__ members, size_t set, int M, int L, int N,
                                                            double* __restrict__ mean) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= set) return;
  const int l = (int)((e / N) % L), m = (int)((e / ((size_t)N * L)) % L);
  double s = 0.0;
  if (l >= m) {
    for (int i = 0; i < M; ++i) s += members[(size_t)i * set + e];
    s /= (double)M;
  }
  mean[e] = s;
}

// The six ensemble sums of one (l, n), from the coefficient sets [truth | member 0 .. M-1 | mean]:
//   P0 = p(y)  P1 = sum_i p(x_i)  P2 = p(mean)  P3 = sum_i p(x_i - y)  P4 = p(mean - y)  P5 = sum_i p(x_i - mean)
// each p() complete (divided by 4 pi) before it is added, members in ascending slot order; differences on the
// coefficients.  sums [6][N][L]; member_power [M][N][L] (may be null): p(x_i).
__global__ __launch_bounds__(256) void gc_spec_ens_kernel(const double* __restrict__ sets, size_t set, int M,
                                                           const unsigned* __restrict__ flags, int L, int N,
                                                           double* __restrict__ sums, double* __restrict__ member_power) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= L * N) return;
  const int l = i / N, n = i - l * N;
  const size_t o = (size_t)n * L + l, plane = (size_t)N * L;
  const bool bad = flags[n] != 0u;
  const double qnan = __builtin_nan("");
  const double* y = sets;
  const double* mean = sets + (size_t)(M + 1) * set;
  double p[6] = {qnan, qnan, qnan, qnan, qnan, qnan};
  if (!bad) {
    p[0] = spec_power_of(y, nullptr, L, N, l, n);
    p[2] = spec_power_of(mean, nullptr, L, N, l, n);
    p[4] = spec_power_of(mean, y, L, N, l, n);
    p[1] = p[3] = p[5] = 0.0;
  }
  for (int k = 0; k < M; ++k) {
    const double* x = sets + (size_t)(k + 1) * set;
    double px = qnan;
    if (!bad) {
      px = spec_power_of(x, nullptr, L, N, l, n);
      p[1] += px;
      p[3] += spec_power_of(x, y, L, N, l, n);
      p[5] += spec_power_of(x, mean, L, N, l, n);
    }
    if (member_power) member_power[(size_t)k * plane + o] = px;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) sums[(size_t)k * plane + o] = p[k];
}

// ---- spectral band views (gc_ens_band_*) ---------------------------------------------------------------
// One field (a member or the truth) at a time: the distinct source columns the plan reads are gathered side by side (the
// same bits), analysed by the two kernels above, and every derived column (b, j) is synthesised back from the coefficients
// of its source column weighted with the response of its band:
//   Legendre synthesis  G[part][m][lat][col] = sum_{l >= m} S[m][lat][l] (w_k[l] a[part][m][l][u(col)])        l ascending
//   Fourier synthesis   g[lat][j][col] = sum_m (cos_s[m][j] G[0][m][lat][col] + sin_s[m][j] G[1][m][lat][col])  m ascending
//   epilogue            d = (float) g, or (float) ((double) f - g) with the band's complement flag; NaN for a flagged column
// The layout is the one of the analysis: lane = column, a wave keeps 16 output rows (latitudes, then longitudes) in
// registers, the table values of a row are wave-uniform and consecutive in the summed index.  The response is per lane (the
// lanes of a wave own different bands): K L doubles that stay in the vector cache.

// gathered [G][Nu] <- the source columns (b, ulist[u]) of a field [G][B c_src]; one thread per element
__global__ __launch_bounds__(256) void gc_band_gather_kernel(const float* __restrict__ field, size_t G, int B, int c_src, int nu,
                                                              const int* __restrict__ ulist, float* __restrict__ out) {
  const int Nu = B * nu;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= G * (size_t)Nu) return;
  const size_t node = e / Nu;
  const int col = (int)(e - node * Nu), b = col / nu, u = col - b * nu;
  reinterpret_cast<unsigned*>(out)[e] = reinterpret_cast<const unsigned*>(field)[node * ((size_t)B * c_src) + (size_t)b * c_src + ulist[u]];
}

// Legendre synthesis.  grid = (L, 2 ceil(n_lat / 64), ceil(Nd / 64)): blockIdx.x = m, blockIdx.y = part + 2 (block of 64
// latitudes); lane = derived column.  The loader forms b = w a, rounded, before it enters the fused multiply-adds.
__global__ __launch_bounds__(256) void gc_band_legendre_kernel(const float* __restrict__ S,        // [L m][n_lat][L l]
                                                                const double* __restrict__ coef,    // [2][L m][L l][Nu]
                                                                const double* __restrict__ resp,    // [K][L]
                                                                const int* __restrict__ band_of, const int* __restrict__ ucol,
                                                                int L, int n_lat, int B, int c_d, int nu,
                                                                double* __restrict__ Gs) {           // [2][L m][n_lat][Nd]
  const int m = blockIdx.x, part = blockIdx.y & 1;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int Nd = B * c_d, Nu = B * nu;
  const int col = blockIdx.z * 64 + lane;
  const int lat0 = (blockIdx.y >> 1) * kSpecBlockRows + wave * kSpecRows;
  if (lat0 >= n_lat) return;
  const float* srow[kSpecRows];
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k) srow[k] = S + ((size_t)m * n_lat + min(lat0 + k, n_lat - 1)) * L;
  double acc[kSpecRows];
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k) acc[k] = 0.0;
  const int cc = min(col, Nd - 1), b = cc / c_d, j = cc - b * c_d;
  const double* const w = resp + (size_t)band_of[j] * L;
  const double* const a = coef + ((size_t)part * L + m) * L * Nu + (size_t)b * nu + ucol[j];
  for (int l = m; l < L; ++l) {
    const double x = w[l] * a[(size_t)l * Nu];
#pragma unroll
    for (int k = 0; k < kSpecRows; ++k) acc[k] = fma((double)srow[k][l], x, acc[k]);
  }
  if (col >= Nd) return;
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k)
    if (lat0 + k < n_lat) Gs[(((size_t)part * L + m) * n_lat + lat0 + k) * Nd + col] = acc[k];
}

// Fourier synthesis and epilogue.  grid = (n_lat, ceil(n_lon / 64), ceil(Nd / 64)); lane = derived column, a wave keeps 16
// longitudes.  tab [n_lon][L][2]: (cos_s, sin_s) of a longitude, consecutive in m.  The result goes straight to channel j of
// the destination field; src is the field the complement subtracts from.
__global__ __launch_bounds__(256) void gc_band_fourier_kernel(const float* __restrict__ tab, const double* __restrict__ Gs,
                                                               const float* __restrict__ src,       // [G][B c_src]
                                                               const unsigned* __restrict__ flags,  // [Nu] of this field
                                                               const int* __restrict__ comp, const int* __restrict__ band_of,
                                                               const int* __restrict__ chan, const int* __restrict__ ucol,
                                                               int L, int n_lat, int n_lon, int B, int c_src, int c_d, int nu,
                                                               float* __restrict__ dst) {            // [G][Nd]
  const int lat = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int Nd = B * c_d;
  const int col = blockIdx.z * 64 + lane;
  const int j0 = blockIdx.y * kSpecBlockRows + wave * kSpecRows;
  if (j0 >= n_lon) return;
  const float* trow[kSpecRows];
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k) trow[k] = tab + (size_t)min(j0 + k, n_lon - 1) * 2 * L;
  double acc[kSpecRows];
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k) acc[k] = 0.0;
  const int cc = min(col, Nd - 1);
  const size_t plane = (size_t)L * n_lat * Nd;
  const double* const g0 = Gs + (size_t)lat * Nd + cc;
  for (int m = 0; m < L; ++m) {
    const double xc = g0[(size_t)m * n_lat * Nd], xs = g0[plane + (size_t)m * n_lat * Nd];
#pragma unroll
    for (int k = 0; k < kSpecRows; ++k) {
      acc[k] = fma((double)trow[k][2 * m], xc, acc[k]);
      acc[k] = fma((double)trow[k][2 * m + 1], xs, acc[k]);
    }
  }
  if (col >= Nd) return;
  const int b = col / c_d, j = col - b * c_d;
  const bool bad = flags[b * nu + ucol[j]] != 0u, complement = comp[band_of[j]] != 0;
  const float* const f = src + (size_t)b * c_src + chan[j];
#pragma unroll
  for (int k = 0; k < kSpecRows; ++k) {
    if (j0 + k >= n_lon) continue;
    const size_t node = (size_t)lat * n_lon + j0 + k;
    float d = complement ? (float)((double)f[node * ((size_t)B * c_src)] - acc[k]) : (float)acc[k];
    if (bad) d = __builtin_nanf("");
    dst[node * Nd + col] = d;
  }
}

static bool spec_grid_ok(int L, int n_lat, int N) {
  return L >= 1 && n_lat >= 1 && N >= 1 && n_lat <= 65535 && (N + 63) / 64 <= 65535 &&
         2 * ((L + kSpecBlockRows - 1) / kSpecBlockRows) <= 65535 && (long long)L * N < (1ll << 31) - 256;
}

// field -> coefficient set (F is the scratch of the Fourier step)
static hipError_t launch_spec_analysis(hipStream_t s, const float* field, const float* tab, const float* Q, int L, int n_lat,
                                       int n_lon, int N, double* F, double* coef, unsigned* flags) {
  if (!spec_grid_ok(L, n_lat, N)) return hipErrorInvalidValue;
  const unsigned cols = (unsigned)((N + 63) / 64);
  hipLaunchKernelGGL(gc_spec_fourier_kernel, dim3(n_lat, (2 * L + kSpecBlockRows - 1) / kSpecBlockRows, cols), dim3(256), 0, s,
                     field, tab, L, n_lat, n_lon, N, F, flags);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gc_spec_legendre_kernel, dim3(L, 2 * ((L + kSpecBlockRows - 1) / kSpecBlockRows), cols), dim3(256), 0, s, Q, F,
                     L, n_lat, N, coef);
  return hipGetLastError();
}

static hipError_t launch_spec_power(hipStream_t s, const double* coef, const unsigned* flags, int L, int N, double* out) {
  hipLaunchKernelGGL(gc_spec_power_kernel, dim3((L * N + 255) / 256), dim3(256), 0, s, coef, flags, L, N, out);
  return hipGetLastError();
}

static hipError_t launch_spec_ens(hipStream_t s, double* sets, size_t set, int M, const unsigned* flags, int L, int N, double* sums,
                                  double* member_power) {
  hipLaunchKernelGGL(gc_spec_mean_kernel, dim3((unsigned)((set + 255) / 256)), dim3(256), 0, s, sets + set, set, M, L, N,
                     sets + (size_t)(M + 1) * set);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gc_spec_ens_kernel, dim3((L * N + 255) / 256), dim3(256), 0, s, sets, set, M, flags, L, N, sums, member_power);
  return hipGetLastError();
}

// the device side of a band plan (gc_ens_band_set) and the scratch of the field in flight
struct BandPlan {
  const double* resp;
  const float *leg, *tab;
  const int *comp, *chan, *band_of, *ucol, *ulist;
  int L, n_lat, n_lon, B, c_src, c_d, nu;
  float* gather;
  double *F, *coef, *Gs;
};

// one field [G][B c_src] -> the band field [G][B c_d]; flags: the [B nu] of this field, zeroed by the caller
static hipError_t launch_band_field(hipStream_t s, const BandPlan& p, const float* atab, const float* Q, const float* src, float* dst,
                                    unsigned* flags) {
  const int Nu = p.B * p.nu, Nd = p.B * p.c_d;
  const size_t G = (size_t)p.n_lat * p.n_lon;
  hipLaunchKernelGGL(gc_band_gather_kernel, dim3((unsigned)((G * Nu + 255) / 256)), dim3(256), 0, s, src, G, p.B, p.c_src, p.nu,
                     p.ulist, p.gather);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if ((e = launch_spec_analysis(s, p.gather, atab, Q, p.L, p.n_lat, p.n_lon, Nu, p.F, p.coef, flags)) != hipSuccess) return e;
  const unsigned cols = (unsigned)((Nd + 63) / 64);
  hipLaunchKernelGGL(gc_band_legendre_kernel, dim3(p.L, 2 * ((p.n_lat + kSpecBlockRows - 1) / kSpecBlockRows), cols), dim3(256), 0, s,
                     p.leg, p.coef, p.resp, p.band_of, p.ucol, p.L, p.n_lat, p.B, p.c_d, p.nu, p.Gs);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(gc_band_fourier_kernel, dim3(p.n_lat, (p.n_lon + kSpecBlockRows - 1) / kSpecBlockRows, cols), dim3(256), 0, s,
                     p.tab, p.Gs, src, flags, p.comp, p.band_of, p.chan, p.ucol, p.L, p.n_lat, p.n_lon, p.B, p.c_src, p.c_d, p.nu,
                     dst);
  return hipGetLastError();
}

}  // namespace gc

using namespace gci;

namespace {

size_t spec_set_len(const gc_handle* h) { return (size_t)2 * h->sp_L * h->sp_L * h->cfg.batch * h->cfg.c_out; }

int spec_ready(gc_handle* h) {
  const int rc = need_graph(h);
  return rc ? rc : need(h, h->sp_L != 0, "no analysis tables (gc_spec_set_tables)");
}

// The buffers sized by the number of coefficient sets a call keeps: made again when a call needs more than there are.
int spec_reserve_sets(gc_handle* h, int sets) {
  if (sets <= h->sp_sets) return GC_OK;
  GC_HIP(h, h->spec_work_allocs.drop(h->stream));
  h->sp_sets = 0;
  const size_t out = (size_t)h->cfg.batch * h->cfg.c_out * h->sp_L;
  if (int rc = alloc_all(h, h->spec_work_allocs, buf(&h->d_sp_coef, (size_t)sets * spec_set_len(h)),
                         buf(&h->d_sp_out, (size_t)(6 + sets) * out)))
    return rc;
  h->sp_sets = sets;
  return GC_OK;
}

// columns with a value that was not finite
int64_t flagged(const std::vector<unsigned>& flags) {
  int64_t bad = 0;
  for (unsigned f : flags) bad += f ? 1 : 0;
  return bad;
}

}  // namespace

extern "C" {

int gc_spec_set_tables(gc_handle* h, int32_t n_lat, int32_t n_lon, int32_t lmax, const float* legendre_analysis,
                       const float* cos_a, const float* sin_a) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (!legendre_analysis || !cos_a || !sin_a) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (n_lat < 2 || n_lon < 2 || (int64_t)n_lat * n_lon != h->hg.G)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "n_lat * n_lon must equal the number of grid nodes");
  if (lmax < 1 || 2 * (int64_t)lmax > n_lon) return fail(h, GC_ERR_INVALID_ARGUMENT, "lmax must be in 1 .. n_lon / 2");
  const int N = h->cfg.batch * h->cfg.c_out;
  if (!gc::spec_grid_ok(lmax, n_lat, N)) return fail(h, GC_ERR_UNSUPPORTED, "grid too large for the spectrum kernels");
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, h->spec_allocs.drop(h->stream));       // nothing reads the old tables any more
  h->spec_work_allocs.free();
  h->band_allocs.free();                           // a band plan is made for the grid and the band limit of the tables: it goes with them
  h->band_work_allocs.free();
  h->band_set = false;
  h->sp_L = h->sp_sets = 0;
  const size_t L = (size_t)lmax;
  std::vector<float> tab(2 * L * n_lon);
  std::copy(cos_a, cos_a + L * n_lon, tab.begin());
  std::copy(sin_a, sin_a + L * n_lon, tab.begin() + L * n_lon);
  if (int rc = alloc_all(h, h->spec_allocs, buf(&h->d_sp_q, L * L * n_lat, legendre_analysis), buf(&h->d_sp_tab, tab),
                         buf(&h->d_sp_F, 2 * L * n_lat * N), buf(&h->d_sp_field, field_len(h)), buf(&h->d_sp_flags, (size_t)N)))
    return rc;
  h->sp_L = lmax; h->sp_lat = n_lat; h->sp_lon = n_lon;
  return GC_OK;
  });
}

int gc_spec_field(gc_handle* h, const float* field, double* power) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = spec_ready(h)) || (rc = need_out(h, power)) ||
      (rc = need(h, field || (h->finalized && h->has_sample), "no sample on the device (gc_sample_resident)")))
    return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if (!field && (rc = resolve_guard(h))) return rc;   // the spectrum is of the CHECKED sample (exact-f32 re-run included)
  if ((rc = spec_reserve_sets(h, 1))) return rc;
  if (field && (rc = staged_upload(h, h->pin_noise, h->d_sp_field, field, field_len(h)))) return rc;
  const int L = h->sp_L, N = h->cfg.batch * h->cfg.c_out;
  hipStream_t s = h->stream;
  const float* src = field ? h->d_sp_field : h->d_sx;
  std::vector<unsigned> flags((size_t)N);
  rc = timed(h, h->spec,
             [&]() -> int {
               GC_HIP(h, hipMemsetAsync(h->d_sp_flags, 0, (size_t)N * sizeof(unsigned), s));
               return launch_each(h,
                   [&] {
                     return gc::launch_spec_analysis(s, src, h->d_sp_tab, h->d_sp_q, L, h->sp_lat, h->sp_lon, N, h->d_sp_F, h->d_sp_coef,
                                                     h->d_sp_flags);
                   },
                   [&] { return gc::launch_spec_power(s, h->d_sp_coef, h->d_sp_flags, L, N, h->d_sp_out); });
             },
             [&]() -> int {
               if ((rc = read_back(h, power, h->d_sp_out, (size_t)N * L)) || (rc = read_back(h, flags.data(), h->d_sp_flags, flags.size())))
                 return rc;
               return GC_OK;
             });
  if (rc) return rc;
  h->spec.invalid = flagged(flags);
  return GC_OK;
  });
}

int gc_ens_spectrum(gc_handle* h, const float* truth, double* sums, double* member_power) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = spec_ready(h)) || (rc = need_store(h)) || (rc = need_out(h, sums)) || (rc = store_complete(h, h))) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_spectrum"))) return rc;
  const int M = h->ens_members;
  const size_t field = field_len(h), set = spec_set_len(h);
  if ((rc = spec_reserve_sets(h, M + 2))) return rc;
  const int L = h->sp_L, N = h->cfg.batch * h->cfg.c_out;
  const size_t plane = (size_t)N * L;
  hipStream_t s = h->stream;
  double* const d_sums = h->d_sp_out;
  double* const d_mp = h->d_sp_out + 6 * plane;
  std::vector<unsigned> flags((size_t)N);
  rc = timed(h, h->spec,
             [&]() -> int {
               GC_HIP(h, hipMemsetAsync(h->d_sp_flags, 0, (size_t)N * sizeof(unsigned), s));
               // one field at a time through the Fourier scratch; set 0 = truth, 1 + i = member i, M + 1 = the mean coefficients
               for (int k = 0; k <= M; ++k) {
                 const float* src = k == 0 ? h->d_ens_truth : h->d_ens + (size_t)(k - 1) * field;
                 if ((rc = launch_each(h, [&] {
                       return gc::launch_spec_analysis(s, src, h->d_sp_tab, h->d_sp_q, L, h->sp_lat, h->sp_lon, N, h->d_sp_F,
                                                       h->d_sp_coef + (size_t)k * set, h->d_sp_flags);
                     })))
                   return rc;
               }
               return launch_each(h, [&] {
                 return gc::launch_spec_ens(s, h->d_sp_coef, set, M, h->d_sp_flags, L, N, d_sums, member_power ? d_mp : nullptr);
               });
             },
             [&]() -> int {
               if ((rc = read_back(h, sums, d_sums, 6 * plane)) ||
                   (member_power && (rc = read_back(h, member_power, d_mp, (size_t)M * plane))) ||
                   (rc = read_back(h, flags.data(), h->d_sp_flags, flags.size())))
                 return rc;
               return GC_OK;
             });
  if (rc) return rc;
  h->spec.invalid = flagged(flags);
  return GC_OK;
  });
}

int gc_ens_band_set(gc_handle* h, int32_t c_src, int32_t n_bands, const double* response, const int32_t* complement,
                    const int32_t* src_channel, const int32_t* band, const float* legendre_synthesis, const float* cos_s,
                    const float* sin_s) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc = spec_ready(h);
  if (rc) return rc;
  if (n_bands < 1 || n_bands > 8) return fail(h, GC_ERR_UNSUPPORTED, "the number of bands must be in 1 .. 8");
  if (!response || !complement || !src_channel || !band || !legendre_synthesis || !cos_s || !sin_s)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (c_src < 1) return fail(h, GC_ERR_INVALID_ARGUMENT, "c_src must be positive");
  const int c_d = h->cfg.c_out, B = h->cfg.batch, K = n_bands;
  const size_t L = (size_t)h->sp_L, n_lat = (size_t)h->sp_lat, n_lon = (size_t)h->sp_lon;
  for (size_t i = 0; i < (size_t)K * L; ++i)
    if (!std::isfinite(response[i])) return fail(h, GC_ERR_INVALID_ARGUMENT, "the response of band " + std::to_string(i / L) + " is not finite at l = " + std::to_string(i % L));
  std::vector<int> ulist;                            // the distinct source channels, ascending
  for (int j = 0; j < c_d; ++j) {
    if (src_channel[j] < 0 || src_channel[j] >= c_src) return fail(h, GC_ERR_INVALID_ARGUMENT, "derived channel " + std::to_string(j) + ": source channel outside [0, c_src)");
    if (band[j] < 0 || band[j] >= K) return fail(h, GC_ERR_INVALID_ARGUMENT, "derived channel " + std::to_string(j) + ": band outside [0, n_bands)");
    ulist.push_back(src_channel[j]);
  }
  std::sort(ulist.begin(), ulist.end());
  ulist.erase(std::unique(ulist.begin(), ulist.end()), ulist.end());
  const int nu = (int)ulist.size();
  if (!gc::spec_grid_ok(h->sp_L, h->sp_lat, B * nu) || !gc::spec_grid_ok(h->sp_L, h->sp_lat, B * c_d))
    return fail(h, GC_ERR_UNSUPPORTED, "grid too large for the spectrum kernels");
  GC_HIP(h, hipSetDevice(h->device));
  // one blob.  doubles: response [K][L]; floats: the Legendre synthesis [L][n_lat][L], then (cos_s, sin_s) [n_lon][L][2];
  // int32: complement [K], src_channel, band, place in the list [c_d], the list [nu]
  const size_t n_d = (size_t)K * L, n_leg = L * n_lat * L, n_f = n_leg + 2 * n_lon * L, n_i = (size_t)K + 3 * (size_t)c_d + nu;
  std::vector<double> blob(n_d + (n_f + 1) / 2 + (n_i + 1) / 2);
  std::copy(response, response + n_d, blob.begin());
  float* const fb = reinterpret_cast<float*>(blob.data() + n_d);
  std::copy(legendre_synthesis, legendre_synthesis + n_leg, fb);
  for (size_t m = 0; m < L; ++m)
    for (size_t j = 0; j < n_lon; ++j) {
      fb[n_leg + (j * L + m) * 2] = cos_s[m * n_lon + j];
      fb[n_leg + (j * L + m) * 2 + 1] = sin_s[m * n_lon + j];
    }
  int32_t* const ib = reinterpret_cast<int32_t*>(blob.data() + n_d + (n_f + 1) / 2);
  for (int k = 0; k < K; ++k) ib[k] = complement[k] ? 1 : 0;
  for (int j = 0; j < c_d; ++j) {
    ib[K + j] = src_channel[j];
    ib[K + c_d + j] = band[j];
    ib[K + 2 * c_d + j] = (int)(std::lower_bound(ulist.begin(), ulist.end(), src_channel[j]) - ulist.begin());
  }
  std::copy(ulist.begin(), ulist.end(), ib + K + 3 * (size_t)c_d);
  GC_HIP(h, h->band_allocs.drop(h->stream));         // nothing reads the old plan any more
  h->band_set = false;
  double* d_blob = nullptr;
  if ((rc = dev_alloc(h, &d_blob, blob.size(), &h->band_allocs))) return rc;
  GC_HIP(h, h->ev_band_src.ensure());
  if ((rc = store_upload(h, d_blob, blob.data(), blob.size() * sizeof(double)))) return rc;
  h->d_band_resp = d_blob;
  h->d_band_leg = reinterpret_cast<float*>(d_blob + n_d);
  h->d_band_tab = h->d_band_leg + n_leg;
  h->d_band_comp = reinterpret_cast<int*>(d_blob + n_d + (n_f + 1) / 2);
  h->d_band_chan = h->d_band_comp + K;
  h->d_band_of = h->d_band_chan + c_d;
  h->d_band_ucol = h->d_band_of + c_d;
  h->d_band_ulist = h->d_band_ucol + c_d;
  h->band_c_src = c_src;
  h->band_K = K;
  h->band_nu = nu;
  h->band_set = true;
  return GC_OK;
  });
}

int gc_ens_band(gc_handle* h, gc_handle* src, const float* truth) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_source(h, src)) || (rc = spec_ready(h)) || (rc = need(h, h->band_set, "no plan (gc_ens_band_set)"))) return rc;
  const int B = h->cfg.batch, c_d = h->cfg.c_out, M = h->ens_members, nu = h->band_nu;
  const size_t L = (size_t)h->sp_L, n_lat = (size_t)h->sp_lat, Nu = (size_t)B * nu, Nd = (size_t)B * c_d;
  const size_t field = field_len(h), sfield = field_len(src);
  rc = fill_open(h, src, h->band_c_src, truth, "gc_ens_band", h->ev_band_src, [&] {   // the scratch of ONE field, and the flags of all
    return sized_for(h, h->band_work_allocs, {Nu, (size_t)M + 1}, buf(&h->d_band_gather, (size_t)h->hg.G * Nu),
                     buf(&h->d_band_F, 2 * L * n_lat * Nu), buf(&h->d_band_coef, 2 * L * L * Nu), buf(&h->d_band_G, 2 * L * n_lat * Nd),
                     buf(&h->d_band_flags, ((size_t)M + 1) * Nu));
  });
  if (rc) return rc;
  hipStream_t s = h->stream;
  const gc::BandPlan p{h->d_band_resp, h->d_band_leg, h->d_band_tab, h->d_band_comp, h->d_band_chan, h->d_band_of, h->d_band_ucol,
                       h->d_band_ulist, h->sp_L, h->sp_lat, h->sp_lon, B, src->cfg.c_out, c_d, nu, h->d_band_gather, h->d_band_F,
                       h->d_band_coef, h->d_band_G};
  std::vector<unsigned> flags(((size_t)M + 1) * Nu);
  rc = timed(h, h->band,
             [&]() -> int {
               GC_HIP(h, hipMemsetAsync(h->d_band_flags, 0, ((size_t)M + 1) * Nu * sizeof(unsigned), s));
               for (int z = 0; z <= M; ++z) {        // the M members, then the truth: one field at a time through the scratch
                 const float* from = z < M ? src->d_ens + (size_t)z * sfield : src->d_ens_truth;
                 float* to = z < M ? h->d_ens + (size_t)z * field : h->d_ens_truth;
                 if ((rc = launch_each(h, [&] {
                       return gc::launch_band_field(s, p, h->d_sp_tab, h->d_sp_q, from, to, h->d_band_flags + (size_t)z * Nu);
                     })))
                   return rc;
               }
               return GC_OK;
             },
             [&] { return read_back(h, flags.data(), h->d_band_flags, flags.size()); });
  if (rc) return rc;
  h->band.invalid = flagged(flags);
  h->band.blocks = (int64_t)(((size_t)h->hg.G * Nu + 255) / 256);   // of the gather, the one pass laid out over the nodes
  fill_close(h);
  return GC_OK;
  });
}

}  // extern "C"
