// The Extreme Forecast Index on the device (include/gencast_hip.h, gc_ens_efi_*): the M members of handle h ranked, point
// by point, in the K climatological samples of a second, graph-only handle.  Kernels and their host code live together
// here; DESIGN.md section 8s has the definitions and what is exact.
//
// Per point (g, b, c), from the float32 members x_0 .. x_{M-1}, the samples c_0 .. c_{K-1} and the truth y:
//   le(v) = #{j : c_j <= v}      lt(v) = #{j : c_j < v}                  comparisons on the float32 values
//   f = (sum_i (a[le(x_i)] + a[lt(x_i)])) / M                            i ascending, in double: the EFI
//   o = a[le(y)] + a[lt(y)]                                              the observed index
// a[0 .. K] is the host's table asin(2 n / K - 1) / pi.  A point counts when y, all M members and all K samples are
// finite; elsewhere both fields are NaN.  Per column (b, c), over the counted nodes, w = node weight of h:
//   S0 = sum w    S1 = sum w f    S2 = sum w o    S3 = sum w f o    S4 = sum w f^2    S5 = sum w o^2
// and, for event t of the truth (dir > 0: lt(y) >= rank, dir < 0: le(y) <= rank) and EFI bin e = min(E - 1, (int)((f + 1) E / 2)):
//   weighted[t][b][c][o_t][e] += wq[g]     counts[t][b][c][o_t][e] += 1
// The six sums have one order (gc_colsum.h); the tables are integers, so their atomics commute.  Two passes, as in
// gc_events.hip: the index pass leaves one 16-bit code per point, the table pass reads the codes and the weights.
#include "gc_colsum.h"
#include "gc_sort.h"
#include "gc_store.h"

// the per-point arithmetic is the definition above, operation for operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace gc {

constexpr int kEfiSums = 6;
constexpr int kEfiMaxEvents = 4, kEfiMaxBins = 32;
constexpr int kEfiTable = 65;                    // a[0 .. 64]; the LDS copy is zero behind K
constexpr size_t kEfiTableLds = 40 * 1024;       // both tables of a workgroup of the table pass (that of gc_events.hip)
constexpr int kEfiMaxWorkgroups = 1024;

struct EfiEvents {
  int T, E;
  int rank[kEfiMaxEvents], dir[kEfiMaxEvents];
};

// le and lt of x in the padded samples: P compare-and-adds each, every register index a compile-time constant.  The +inf
// padding satisfies neither comparison against a finite x; against x = +inf it does (le <= P <= 64: inside the LDS copy,
// and the point is not counted).
template <int P>
__device__ inline void efi_rank(const float (&v)[P], float x, int& le, int& lt) {
  le = 0;
  lt = 0;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    le += v[k] <= x ? 1 : 0;
    lt += v[k] < x ? 1 : 0;
  }
}

// The index pass, on the 256-wide cut of gc_colsum.h.  Per point the K samples are read once into P padded registers
// (load_padded); the M members stream past them (M loads of stride `field`, coalesced across the wave).
// TRUTH: also the observed index, the code and the six sums; else the EFI field alone.
// Out, as plain stores: efi / obs [field], code [field], part[block x][6][W] (double), ipart[block x][tile] (skipped).
template <int P, bool TRUTH>
__global__ __launch_bounds__(256) void gc_ens_efi_kernel(const float* __restrict__ mem, int M, const float* __restrict__ clim,
                                                          int K, size_t field, const float* __restrict__ truth,
                                                          const float* __restrict__ node_w, const double* __restrict__ table,
                                                          const EfiEvents ev, int G, int W, int per, float* __restrict__ efi,
                                                          float* __restrict__ obs, unsigned short* __restrict__ code,
                                                          double* __restrict__ part, unsigned* __restrict__ ipart) {
  __shared__ double tab[kEfiTable];
  __shared__ double lane_sum[256];
  __shared__ unsigned skipped;
  const ColTile ct(256, 256, W, blockIdx.y);
  const int tid = threadIdx.x, col = ct.col;
  if (tid < kEfiTable) tab[tid] = tid <= K ? table[tid] : 0.0;
  if (tid == 0) skipped = 0u;
  __syncthreads();
  double s[kEfiSums];
#pragma unroll
  for (int k = 0; k < kEfiSums; ++k) s[k] = 0.0;
  unsigned inv = 0;
  if (ct.active()) {
    const double dM = (double)M;
    const float nan = __builtin_nanf("");
    const int n_end = ct.n_end(G, per);
    for (int n = ct.n_begin(per); n < n_end; n += ct.q) {
      const size_t i = (size_t)n * W + col;
      float v[P];
      bool fin = load_padded<P>(v, clim, field, i, K);
      float y = 0.f;
      if constexpr (TRUTH) {
        y = truth[i];
        fin = fin && isfinite(y);
      }
      double acc = 0.0;
      if (fin) {                                     // (a point that is out already does not read its members)
#pragma unroll 2
        for (int m = 0; m < M; ++m) {
          const float x = mem[(size_t)m * field + i];
          fin = fin && isfinite(x);
          int le, lt;
          efi_rank<P>(v, x, le, lt);
          acc += tab[le] + tab[lt];
        }
      }
      if (!fin) {
        efi[i] = nan;
        if constexpr (TRUTH) {
          obs[i] = nan;
          code[i] = (unsigned short)0xFFFFu;
          ++inv;
        }
        continue;
      }
      const double f = acc / dM;
      efi[i] = (float)f;
      if constexpr (TRUTH) {
        int le, lt;
        efi_rank<P>(v, y, le, lt);
        const double o = tab[le] + tab[lt];
        obs[i] = (float)o;
        unsigned c = (unsigned)min(ev.E - 1, (int)((f + 1.0) * (0.5 * (double)ev.E)));
#pragma unroll
        for (int t = 0; t < kEfiMaxEvents; ++t)
          if (t < ev.T && (ev.dir[t] > 0 ? lt >= ev.rank[t] : le <= ev.rank[t])) c |= 256u << t;
        code[i] = (unsigned short)c;
        const double w = (double)node_w[n];
        s[0] += w;
        s[1] += w * f;
        s[2] += w * o;
        s[3] += w * (f * o);
        s[4] += w * (f * f);
        s[5] += w * (o * o);
      }
    }
  }
  if constexpr (TRUTH) {
    if (inv) atomicAdd(&skipped, inv);               // (an integer: the order of these does not show)
#pragma unroll
    for (int k = 0; k < kEfiSums; ++k) {
      const double t = col_total(lane_sum, s[k], ct);
      if (tid < ct.wt) part[((size_t)blockIdx.x * kEfiSums + k) * W + col] = t;
    }
    if (tid == 0) ipart[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = skipped;
  }
}

// Column tiles of the table pass, as gc_events.hip cuts them: as few as fit the LDS budget, of equal width, a column's
// 2 E bins padded to the odd stride 2 E + 1 (most points of a column land in the bins of o = 0 around f = 0).
static int efi_stride(int E) { return 2 * E + 1; }
static int efi_tiles(int W, int E) {
  const int fit = std::max(1, std::min(256, (int)(kEfiTableLds / ((size_t)efi_stride(E) * 12))));
  return (W + fit - 1) / fit;
}
static int efi_tile_width(int W, int E) { const int tiles = efi_tiles(W, E); return (W + tiles - 1) / tiles; }

// Table pass.  grid = (node-range blocks, events, column tiles): equal-width tiles of gc_colsum.h, cap = 256.  Dynamic
// LDS: unsigned long long[wt][stride] weighted, then unsigned[wt][stride] counts.  A block's non-zero bins leave by
// integer atomics into the zeroed global tables weighted / counts [T][W][2][E].
__global__ __launch_bounds__(256) void gc_ens_efi_table_kernel(const unsigned short* __restrict__ code,
                                                                const unsigned* __restrict__ wq, int G, int W, int E,
                                                                int tile_w, int per, unsigned long long* __restrict__ weighted,
                                                                unsigned long long* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char efi_lds[];
  const int t = blockIdx.y;
  const ColTile ct(tile_w, 256, W, blockIdx.z);
  const int col0 = ct.col0, wt = ct.wt, cl = ct.cl;
  const int tid = threadIdx.x;
  const int bins = 2 * E, stride = bins + 1;
  unsigned long long* const wtab = reinterpret_cast<unsigned long long*>(efi_lds);
  unsigned* const ctab = reinterpret_cast<unsigned*>(wtab + (size_t)tile_w * stride);
  for (int i = tid; i < wt * stride; i += 256) {
    wtab[i] = 0ull;
    ctab[i] = 0u;
  }
  __syncthreads();
  if (ct.active()) {
    const unsigned short* const my = code + col0 + cl;
    const int n_end = ct.n_end(G, per);
#pragma unroll 4
    for (int n = ct.n_begin(per); n < n_end; n += ct.q) {
      const unsigned c = my[(size_t)n * W];
      if (c == 0xFFFFu) continue;
      const int bin = cl * stride + (int)((c >> (8 + t)) & 1u) * E + (int)(c & 31u);
      atomicAdd(&wtab[bin], (unsigned long long)wq[n]);
      atomicAdd(&ctab[bin], 1u);
    }
  }
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
}

// The ascending block finish: e < 6 W: sum j = e / W of column e % W, as the partials lie -> out [W][6]; the skipped
// points -> outc[0].
struct EfiFinishMap {
  const double* part;
  int W;
  SkippedSum skipped;
  __host__ __device__ int sums() const { return kEfiSums * W; }
  __host__ __device__ int counts() const { return 0; }
  __device__ BlockSum<double> sum(int e) const {
    const int j = e / W, col = e - j * W;
    return {part + e, (size_t)kEfiSums * W, (size_t)col * kEfiSums + j};
  }
  __device__ BlockSum<unsigned> count(int) const { return {nullptr, 0, 0}; }
};

// the padded size is that of K alone: the members are never held
template <bool TRUTH>
static hipError_t launch_ens_efi(hipStream_t s, const float* mem, int M, const float* clim, int K, size_t field,
                                 const float* truth, const float* node_w, const double* table, const EfiEvents& ev, int G, int B,
                                 int c_out, float* efi, float* obs, unsigned short* code, double* part, unsigned* ipart) {
  const int W = B * c_out;
  const int blocks = loss_reduce_blocks(G, B, c_out);
  const int per = (G + blocks - 1) / blocks;
  const dim3 grid(blocks, (W + 255) / 256);
  return pad_dispatch(K, [&](auto p) {
    hipLaunchKernelGGL((gc_ens_efi_kernel<decltype(p)::value, TRUTH>), grid, dim3(256), 0, s, mem, M, clim, K, field, truth, node_w,
                       table, ev, G, W, per, efi, obs, code, part, ipart);
    return hipGetLastError();
  });
}

// node-range blocks of the table pass: within kEfiMaxWorkgroups for the whole grid
static int efi_table_blocks(int G, int W, int T, int E) {
  return node_blocks(G, 256 / efi_tile_width(W, E), kEfiMaxWorkgroups / (T * efi_tiles(W, E)));
}

static hipError_t launch_ens_efi_table(hipStream_t s, const unsigned short* code, const unsigned* wq, int G, int W, int T, int E,
                                       unsigned long long* weighted, unsigned long long* counts) {
  const int tiles = efi_tiles(W, E), tile_w = efi_tile_width(W, E);
  const int blocks = efi_table_blocks(G, W, T, E);
  const int per = (G + blocks - 1) / blocks;
  const size_t lds = (size_t)tile_w * efi_stride(E) * (sizeof(unsigned long long) + sizeof(unsigned));
  hipLaunchKernelGGL(gc_ens_efi_table_kernel, dim3(blocks, T, tiles), dim3(256), lds, s, code, wq, G, W, E, tile_w, per, weighted,
                     counts);
  return hipGetLastError();
}

static hipError_t launch_ens_efi_finish(hipStream_t s, const double* part, const unsigned* ipart, int blocks, int tiles, int W,
                                        double* out, unsigned long long* outc) {
  return launch_block_finish(s, EfiFinishMap{part, W, {ipart, tiles, 0}}, blocks, out, outc);
}

}  // namespace gc

using namespace gci;

namespace {

// what both passes ask of the two handles, in the order gc_ens_clim_score reports it; the truth and the weights follow
int efi_stores(gc_handle* h, gc_handle* clim, const double* table) {
  if (!clim || clim == h) return fail(h, GC_ERR_INVALID_ARGUMENT, "the climatology must be another handle");
  int rc;
  if ((rc = need_out(h, table)) || (rc = need_graph(h)) || (rc = check_peer(h, clim, "climatology", false, h->cfg.c_out)) ||
      (rc = need_store(h)) || (rc = need(h, clim->ens_members != 0, "no member store on the climatology handle (gc_ens_reserve)")) ||
      (rc = store_complete(h, h)) || (rc = store_complete(h, clim, "climatology ")))
    return rc;
  // a[K - n] == -a[n] to the bit (so a[K / 2] == 0 for even K) and a non-decreasing: what makes the index antisymmetric
  // and monotone; a NaN fails the first test
  const int K = clim->ens_members;
  for (int n = 0; n <= K; ++n)
    if (!(table[K - n] == -table[n]) || (n > 0 && table[n] < table[n - 1]))
      return fail(h, GC_ERR_INVALID_ARGUMENT, "the table is not antisymmetric and non-decreasing over 0 .. K");
  return GC_OK;
}

// the buffers sized by G, B and c_out alone (made once), then the table of this call behind whatever still reads the last
int efi_buffers(gc_handle* h, const double* table, int K, int blocks, int tiles) {
  int rc;
  if (!h->d_efi_field) {
    const size_t field = field_len(h), W = (size_t)h->cfg.batch * h->cfg.c_out;
    if ((rc = alloc_all(h, h->efi_allocs, buf(&h->d_efi_field, 2 * field), buf(&h->d_efi_code, field),
                        buf(&h->d_efi_tab, (size_t)gc::kEfiTable), buf(&h->d_efi_part, (size_t)blocks * gc::kEfiSums * W),
                        buf(&h->d_efi_ipart, (size_t)blocks * tiles), buf(&h->d_efi_out, (size_t)gc::kEfiSums * W),
                        buf(&h->d_efi_outc, (size_t)1)))) {
      h->d_efi_field = nullptr;
      return rc;
    }
    GC_HIP(h, h->ev_efi_src.ensure());
  }
  return store_upload(h, h->d_efi_tab, table, (size_t)(K + 1) * sizeof(double));
}

}  // namespace

extern "C" {

int gc_ens_efi_set(gc_handle* h, int32_t n_events, const int32_t* rank, const int32_t* direction, int32_t n_bins,
                   const uint32_t* wq) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (n_events < 0 || n_events > gc::kEfiMaxEvents) return fail(h, GC_ERR_INVALID_ARGUMENT, "n_events must be in 0..4");
  if (n_bins < 2 || n_bins > gc::kEfiMaxBins) return fail(h, GC_ERR_INVALID_ARGUMENT, "n_bins must be in 2..32");
  if (n_events > 0 && (!rank || !direction || !wq)) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  for (int t = 0; t < n_events; ++t)
    if (direction[t] == 0) return fail(h, GC_ERR_INVALID_ARGUMENT, "direction " + std::to_string(t) + " is zero");
  GC_HIP(h, hipSetDevice(h->device));
  int rc;
  if (n_events > 0) {
    if (!h->d_efi_wq && (rc = dev_alloc(h, &h->d_efi_wq, (size_t)h->hg.G))) return rc;
    // on the handle's stream, behind whatever still reads the old values; the caller's array is free on return
    if ((rc = store_upload(h, h->d_efi_wq, wq, (size_t)h->hg.G * sizeof(uint32_t)))) return rc;
  }
  for (int t = 0; t < gc::kEfiMaxEvents; ++t) {
    h->efi_rank[t] = t < n_events ? rank[t] : 0;
    h->efi_dir[t] = t < n_events ? (direction[t] > 0 ? 1 : -1) : 0;
  }
  h->efi_T = n_events;
  h->efi_E = n_bins;
  h->efi_set = true;
  return GC_OK;
  });
}

int gc_ens_efi_score(gc_handle* h, gc_handle* clim, const double* table, const float* truth, double* sums, uint64_t* weighted,
                     uint64_t* counts, uint64_t* invalid) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = efi_stores(h, clim, table)) || (rc = need(h, h->efi_set, "no events and bins (gc_ens_efi_set)")) ||
      (rc = need_out(h, sums && (weighted || h->efi_T == 0))) || (rc = need_weights(h)))
    return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_efi_score"))) return rc;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, B = c.batch, W = B * c.c_out, M = h->ens_members, K = clim->ens_members;
  const int T = h->efi_T, E = h->efi_E;
  const int blocks = gc::loss_reduce_blocks(G, B, c.c_out), tiles = (W + 255) / 256;
  const size_t field = field_len(h), len = (size_t)T * W * 2 * E;
  if ((rc = efi_buffers(h, table, K, blocks, tiles)) ||
      (rc = sized_for(h, h->efi_table_allocs, {(size_t)T + 1, (size_t)E}, buf(&h->d_efi_table, 2 * len))))
    return rc;
  hipStream_t s = h->stream;
  // the climatology's store is complete on ITS stream: this handle's stream goes on behind it
  if ((rc = order_behind(h, h->ev_efi_src, clim->stream, s))) return rc;
  gc::EfiEvents ev{T, E, {}, {}};
  for (int t = 0; t < gc::kEfiMaxEvents; ++t) {
    ev.rank[t] = h->efi_rank[t];
    ev.dir[t] = h->efi_dir[t];
  }
  unsigned long long* const d_w = h->d_efi_table;
  unsigned long long* const d_c = d_w + len;
  uint64_t inv = 0;
  h->efi_fields = 0;
  rc = timed(h, h->efi,
             [&]() -> int {
               if (T > 0) GC_HIP(h, hipMemsetAsync(d_w, 0, 2 * len * sizeof(unsigned long long), s));
               int r = launch_each(h,
                   [&] {
                     return gc::launch_ens_efi<true>(s, h->d_ens, M, clim->d_ens, K, field, h->d_ens_truth, h->d_ens_w, h->d_efi_tab,
                                                     ev, G, B, c.c_out, h->d_efi_field, h->d_efi_field + field, h->d_efi_code,
                                                     h->d_efi_part, h->d_efi_ipart);
                   },
                   [&] {
                     return gc::launch_ens_efi_finish(s, h->d_efi_part, h->d_efi_ipart, blocks, tiles, W, h->d_efi_out, h->d_efi_outc);
                   });
               if (r || T == 0) return r;
               return launch_each(h, [&] { return gc::launch_ens_efi_table(s, h->d_efi_code, h->d_efi_wq, G, W, T, E, d_w, d_c); });
             },
             [&]() -> int {
               if ((rc = read_back(h, sums, h->d_efi_out, (size_t)gc::kEfiSums * W)) || (rc = read_back(h, &inv, h->d_efi_outc, 1)) ||
                   (T > 0 && (rc = read_back(h, weighted, d_w, len))) || (T > 0 && counts && (rc = read_back(h, counts, d_c, len))))
                 return rc;
               return GC_OK;
             });
  if (rc) return rc;
  h->efi.invalid = (int64_t)inv;
  h->efi.blocks = T > 0 ? gc::efi_table_blocks(G, W, T, E) : blocks;
  h->efi_fields = 2;
  if (invalid) invalid[0] = inv;
  return GC_OK;
  });
}

int gc_ens_efi_fields(gc_handle* h, gc_handle* clim, const double* table) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = efi_stores(h, clim, table))) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  const gc_config& c = h->cfg;
  const int G = h->hg.G, B = c.batch, W = B * c.c_out, M = h->ens_members, K = clim->ens_members;
  const int blocks = gc::loss_reduce_blocks(G, B, c.c_out), tiles = (W + 255) / 256;
  if ((rc = efi_buffers(h, table, K, blocks, tiles))) return rc;
  hipStream_t s = h->stream;
  if ((rc = order_behind(h, h->ev_efi_src, clim->stream, s))) return rc;
  h->efi_fields = 0;
  rc = timed(h, h->efi,
             [&] {
               return launch_each(h, [&] {
                 return gc::launch_ens_efi<false>(s, h->d_ens, M, clim->d_ens, K, field_len(h), nullptr, nullptr, h->d_efi_tab,
                                                  gc::EfiEvents{}, G, B, c.c_out, h->d_efi_field, nullptr, nullptr, nullptr, nullptr);
               });
             },
             no_readbacks);
  if (rc) return rc;
  h->efi.blocks = blocks;
  h->efi_fields = 1;
  return GC_OK;
  });
}

int gc_ens_efi_download(gc_handle* h, int32_t which, float* field) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (!field) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (which < 0 || which > 1) return fail(h, GC_ERR_INVALID_ARGUMENT, "which must be 0 (the EFI) or 1 (the observed index)");
  if (h->efi_fields == 0) return fail(h, GC_ERR_STATE, "no index fields on the device (gc_ens_efi_score / gc_ens_efi_fields)");
  if (which == 1 && h->efi_fields < 2)
    return fail(h, GC_ERR_STATE, "no observed index on the device: the last call read no truth (gc_ens_efi_score)");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t n = field_len(h);
  GC_HIP(h, hipMemcpyAsync(field, h->d_efi_field + (size_t)which * n, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
  });
}

}  // extern "C"
