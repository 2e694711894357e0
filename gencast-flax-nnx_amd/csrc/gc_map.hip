// Score maps on the device (include/gencast_hip.h, gc_ens_map_*): the marginal scores of the gc_ens_* store kept PER GRID
// POINT and added up over dates, one set of planes per slot (a slot is a lead time).  Kernels and their host code live
// together here; DESIGN.md section 8u has the definitions and what is exact.
//
// Members x_0 .. x_{M-1} (2 <= M <= 64) and truth y are [G, B, c_out] float32 in the sample layout.  A point counts when y
// and all M members are finite there.  No node weight is read: a map is per point.  The plan selects C' channels
// (ascending, distinct), L slots and T event thresholds.
// Per counted point, in double from the float32 values, every operation rounded once and nothing contracted:
//   m  = (sum_i x_i) / M                                          i ascending (slot order)
//   s2 = (sum_i (x_i - m) (x_i - m)) / (M - 1)                    the same order
//   e  = m - y
//   with the members sorted ascending x_(0) <= .. <= x_(M-1):
//   ae = (sum_k |x_(k) - y|) / M                                  k ascending
//   d  = (sum_{k=1}^{M-1} (double)(k (M - k)) (x_(k) - x_(k-1))) / (M (M - 1) / 2)     k ascending: the gap form of section 8l
//   c  = ae - 0.5 d                                               the fair CRPS of the point
//   r  = #{i : x_i < y}                                           a member equal to y is not below it
// The planes of slot l, per point (g, b, c'), each date added to what the dates before left (a left fold in call order):
//   P0 += e   P1 += e e   P2 += s2   P3 += ae   P4 += d   P5 += c c          double
//   N0 += 1   N1 += [r == 0]   N2 += [r == M]                                 uint32
// A point that does not count on a date adds nothing.  Event planes, from the byte gc_ens_event_score leaves per point and
// threshold (code = k | o << 7, 255 = not counted), uint32:
//   E0 += 1   E1 += k   E2 += k k   E3 += k o   E4 += o
// Every point has exactly one owner thread: nothing is reduced, nothing is atomic, and the bytes of a plane are those of
// the NumPy definition (tests/map_reference.py).  Layout: [slot][plane][G][B][C'], so a wave's accesses to one plane are
// contiguous.
#include "gc_colsum.h"
#include "gc_sort.h"
#include "gc_store.h"

// the per-point arithmetic is the definition above, operation for operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace gc {

constexpr int kMapSums = 6, kMapCounts = 3, kMapEventPlanes = 5;
constexpr int kMapMaxSlots = 128, kMapMaxThresholds = 8;
constexpr int kMapMaxBlocks = 1024;              // node-range workgroups of the field pass (grid.x); above it they stride
constexpr int kMapEventMaxBlocks = 2048;

// selected column s = b C' + j of a node -> its column b c_out + chan[j] in the sample layout (chan == nullptr: all)
__device__ inline int map_source_column(int s, int Cs, int c_out, const int* __restrict__ chan) {
  const int b = s / Cs, j = s - b * Cs;
  return b * c_out + (chan ? chan[j] : j);
}

// The field pass, on the 256-wide cut of gc_colsum.h over the Ws = B C' SELECTED columns: thread t owns selected column
// t % wt of node lane t / wt; workgroup x starts at node x q + lane and strides by gridDim.x q, so below kMapMaxBlocks
// every thread has one point.  A point whose truth is not finite reads no member; a point that does not count never
// touches its accumulators.  sums [6][N], counts [3][N] are the planes of the call's slot, N = G Ws.
// Out beside them, as a plain store: ipart[block x][tile] (selected points skipped).
template <int P>
__global__ __launch_bounds__(256) void gc_ens_map_kernel(const float* __restrict__ mem, size_t field, int M,
                                                          const float* __restrict__ truth, const int* __restrict__ chan,
                                                          int G, int c_out, int W, int Cs, int Ws, size_t N,
                                                          double* __restrict__ sums, unsigned* __restrict__ counts,
                                                          unsigned* __restrict__ ipart) {
  __shared__ unsigned skipped;
  const ColTile ct(256, 256, Ws, blockIdx.y);
  if (threadIdx.x == 0) skipped = 0u;
  __syncthreads();
  unsigned inv = 0;
  if (ct.active()) {
    const int src = map_source_column(ct.col, Cs, c_out, chan);
    const double dM = (double)M, pairs = (double)(M * (M - 1) / 2);
    for (size_t n = (size_t)blockIdx.x * ct.q + ct.lane; n < (size_t)G; n += (size_t)gridDim.x * ct.q) {
      const size_t i = n * W + src;
      const float y = truth[i];
      if (!isfinite(y)) {
        ++inv;
        continue;
      }
      float v[P];
      double sum = 0.0;
      const bool fin = load_padded<P>(v, mem, field, i, M, [&](float x) { sum += (double)x; });
      if (!fin) {
        ++inv;
        continue;
      }
      const double yd = (double)y;
      const double m = sum / dM;
      double s2 = 0.0;
#pragma unroll
      for (int k = 0; k < P; ++k) {                 // slot order: before the sort
        if (k < M) {
          const double dx = (double)v[k] - m;
          s2 += dx * dx;
        }
      }
      s2 /= dM - 1.0;
      ord_sort<P>(v);
      double ae = 0.0, pd = 0.0;
      int r = 0;
#pragma unroll
      for (int k = 0; k < P; ++k) {                 // guarded on M, not on P
        if (k < M) {
          ae += fabs((double)v[k] - yd);
          if (k > 0) pd += (double)(k * (M - k)) * ((double)v[k] - (double)v[k - 1]);
          r += v[k] < y ? 1 : 0;
        }
      }
      ae /= dM;
      const double d = pd / pairs;
      const double c = ae - 0.5 * d;
      const double e = m - yd;
      const size_t a = n * Ws + ct.col;
      sums[a] += e;
      sums[N + a] += e * e;
      sums[2 * N + a] += s2;
      sums[3 * N + a] += ae;
      sums[4 * N + a] += d;
      sums[5 * N + a] += c * c;
      counts[a] += 1u;
      if (r == 0) counts[N + a] += 1u;
      if (r == M) counts[2 * N + a] += 1u;
    }
  }
  if (inv) atomicAdd(&skipped, inv);               // (an integer in LDS: the order of these does not show)
  __syncthreads();
  if (threadIdx.x == 0) ipart[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = skipped;
}

// The event pass: one thread per selected point (grid-stride) and threshold t = blockIdx.y.  code [T][G, B, c_out];
// events [T][5][N] are the event planes of the call's slot.
__global__ __launch_bounds__(256) void gc_ens_map_event_kernel(const unsigned char* __restrict__ code, size_t field,
                                                                const int* __restrict__ chan, int c_out, int W, int Cs, int Ws,
                                                                size_t N, unsigned* __restrict__ events) {
  const int t = blockIdx.y;
  const unsigned char* const my = code + (size_t)t * field;
  unsigned* const ev = events + (size_t)t * kMapEventPlanes * N;
  for (size_t a = (size_t)blockIdx.x * 256 + threadIdx.x; a < N; a += (size_t)gridDim.x * 256) {
    const size_t n = a / (size_t)Ws;
    const int s = (int)(a - n * (size_t)Ws);
    const unsigned cd = my[n * W + map_source_column(s, Cs, c_out, chan)];
    if (cd == 255u) continue;
    const unsigned k = cd & 127u, o = cd >> 7;
    ev[a] += 1u;
    ev[N + a] += k;
    ev[2 * N + a] += k * k;
    ev[3 * N + a] += k * o;
    ev[4 * N + a] += o;
  }
}

static int map_tiles(int Ws) { return (Ws + 255) / 256; }
// one point per thread up to the cap
static int map_blocks(int G, int Ws) {
  const int q = 256 / std::min(256, Ws);
  return std::max(1, std::min(kMapMaxBlocks, (G + q - 1) / q));
}
static int map_event_blocks(size_t N) { return (int)std::max<size_t>(1, std::min<size_t>(kMapEventMaxBlocks, (N + 255) / 256)); }

static hipError_t launch_ens_map(hipStream_t s, const float* mem, size_t field, int M, const float* truth, const int* chan, int G,
                                 int B, int c_out, int Cs, double* sums, unsigned* counts, unsigned* ipart) {
  const int Ws = B * Cs;
  const dim3 grid(map_blocks(G, Ws), map_tiles(Ws));
  return pad_dispatch(M, [&](auto p) {
    hipLaunchKernelGGL((gc_ens_map_kernel<decltype(p)::value>), grid, dim3(256), 0, s, mem, field, M, truth, chan, G, c_out,
                       B * c_out, Cs, Ws, (size_t)G * Ws, sums, counts, ipart);
    return hipGetLastError();
  });
}

static hipError_t launch_ens_map_events(hipStream_t s, const unsigned char* code, size_t field, const int* chan, int G, int B,
                                        int c_out, int Cs, int T, unsigned* events) {
  const int Ws = B * Cs;
  const size_t N = (size_t)G * Ws;
  hipLaunchKernelGGL(gc_ens_map_event_kernel, dim3(map_event_blocks(N), T), dim3(256), 0, s, code, field, chan, c_out, B * c_out,
                     Cs, Ws, N, events);
  return hipGetLastError();
}

}  // namespace gc

using namespace gci;

namespace {

// selected points of the plan: one plane holds so many values
size_t map_points(const gc_handle* h) { return (size_t)h->hg.G * h->cfg.batch * h->map_C; }

int map_plan(gc_handle* h) { return need(h, h->map_set, "no map plan (gc_ens_map_set)"); }

int map_slot(gc_handle* h, int32_t slot, int lowest) {
  if (slot < lowest || slot >= h->map_L) return fail(h, GC_ERR_INVALID_ARGUMENT, "slot outside [0, n_slots)");
  return GC_OK;
}

// a slot holds dates of one M
int map_same_members(gc_handle* h, int32_t slot) {
  const int had = h->map_M[(size_t)slot];
  if (had == 0 || had == h->ens_members) return GC_OK;
  return fail(h, GC_ERR_STATE, "slot " + std::to_string(slot) + " holds dates of " + std::to_string(had) + " members, the store has " +
                                   std::to_string(h->ens_members) + ": reset the slot first (gc_ens_map_reset)");
}

const int* map_channels(const gc_handle* h) { return h->map_all ? nullptr : h->d_map_chan; }

}  // namespace

extern "C" {

int gc_ens_map_set(gc_handle* h, int32_t n_channels, const int32_t* channel, int32_t n_slots, int32_t n_event_thresholds) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  const int c_out = h->cfg.c_out;
  if (n_slots < 1 || n_slots > gc::kMapMaxSlots) return fail(h, GC_ERR_UNSUPPORTED, "n_slots must be in 1..128");
  if (n_event_thresholds < 0 || n_event_thresholds > gc::kMapMaxThresholds)
    return fail(h, GC_ERR_UNSUPPORTED, "n_event_thresholds must be in 0..8");
  if (!channel) n_channels = c_out;
  if (n_channels < 1 || n_channels > c_out) return fail(h, GC_ERR_INVALID_ARGUMENT, "n_channels must be in 1..c_out");
  std::vector<int> chan((size_t)n_channels);
  for (int j = 0; j < n_channels; ++j) {
    const int c = channel ? channel[j] : j;
    if (c < 0 || c >= c_out) return fail(h, GC_ERR_INVALID_ARGUMENT, "channel " + std::to_string(j) + " is outside [0, c_out)");
    if (j > 0 && c <= chan[(size_t)j - 1])
      return fail(h, GC_ERR_INVALID_ARGUMENT, "channel " + std::to_string(j) + " is not above the one before it (ascending, distinct)");
    chan[(size_t)j] = c;
  }
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, h->map_allocs.drop(h->stream));          // nothing adds into the old planes any more
  h->map_set = false;
  const int L = n_slots, T = n_event_thresholds, B = h->cfg.batch, G = h->hg.G;
  const size_t N = (size_t)G * B * n_channels;
  const size_t n_sums = (size_t)L * gc::kMapSums * N, n_counts = (size_t)L * gc::kMapCounts * N;
  const size_t n_events = (size_t)L * T * gc::kMapEventPlanes * N;
  const size_t n_ipart = (size_t)gc::kMapMaxBlocks * gc::map_tiles(B * n_channels);
  int rc;
  if ((rc = alloc_all(h, h->map_allocs, buf(&h->d_map_sums, n_sums), buf(&h->d_map_counts, n_counts),
                      buf(&h->d_map_events, n_events), buf(&h->d_map_ipart, n_ipart), buf(&h->d_map_chan, chan))))
    return rc;
  hipStream_t s = h->stream;
  GC_HIP(h, hipMemsetAsync(h->d_map_sums, 0, n_sums * sizeof(double), s));
  GC_HIP(h, hipMemsetAsync(h->d_map_counts, 0, n_counts * sizeof(unsigned), s));
  if (n_events) GC_HIP(h, hipMemsetAsync(h->d_map_events, 0, n_events * sizeof(unsigned), s));
  h->map_C = n_channels;
  h->map_L = L;
  h->map_T = T;
  h->map_all = n_channels == c_out;
  h->map_M.assign((size_t)L, 0);
  h->map_dates.assign((size_t)2 * L, 0);
  h->map_bytes = (int64_t)(n_sums * sizeof(double) + (n_counts + n_events) * sizeof(unsigned));
  h->map_set = true;
  return GC_OK;
  });
}

int gc_ens_map_accumulate(gc_handle* h, int32_t slot, const float* truth) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_graph(h)) || (rc = map_plan(h)) || (rc = map_slot(h, slot, 0)) || (rc = need_store(h)) ||
      (rc = store_complete(h, h)) ||
      (rc = need(h, truth || h->has_ens_truth, "no truth on the device (pass one to gc_ens_map_accumulate)")) ||
      (rc = map_same_members(h, slot)))
    return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_map_accumulate"))) return rc;
  const gc_config& c = h->cfg;
  const int G = h->hg.G, B = c.batch, M = h->ens_members, Cs = h->map_C, Ws = B * Cs;
  const size_t N = map_points(h);
  const int blocks = gc::map_blocks(G, Ws), tiles = gc::map_tiles(Ws);
  std::vector<unsigned> skipped((size_t)blocks * tiles);
  hipStream_t s = h->stream;
  rc = timed(h, h->map,
             [&] {
               return launch_each(h, [&] {
                 return gc::launch_ens_map(s, h->d_ens, field_len(h), M, h->d_ens_truth, map_channels(h), G, B, c.c_out, Cs,
                                           h->d_map_sums + (size_t)slot * gc::kMapSums * N,
                                           h->d_map_counts + (size_t)slot * gc::kMapCounts * N, h->d_map_ipart);
               });
             },
             [&] { return read_back(h, skipped.data(), h->d_map_ipart, skipped.size()); });
  if (rc) return rc;
  int64_t inv = 0;
  for (unsigned v : skipped) inv += (int64_t)v;
  h->map.invalid = inv;
  h->map.blocks = blocks;
  h->map_M[(size_t)slot] = M;
  ++h->map_dates[(size_t)2 * slot];
  return GC_OK;
  });
}

int gc_ens_map_accumulate_events(gc_handle* h, int32_t slot) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_graph(h)) || (rc = map_plan(h)) || (rc = need(h, h->map_T != 0, "the map plan has no event planes (gc_ens_map_set)")) ||
      (rc = map_slot(h, slot, 0)) || (rc = need_store(h)) ||
      (rc = need(h, h->evt_T == h->map_T, "the event thresholds are not as many as the map plan's (gc_ens_event_set, gc_ens_map_set)")) ||
      (rc = need(h, h->evt_scored, "no event codes on the device (gc_ens_event_score)")) || (rc = map_same_members(h, slot)))
    return rc;
  GC_HIP(h, hipSetDevice(h->device));
  const gc_config& c = h->cfg;
  const int G = h->hg.G, B = c.batch, Cs = h->map_C, T = h->map_T;
  const size_t N = map_points(h);
  hipStream_t s = h->stream;
  rc = timed(h, h->map,
             [&] {
               return launch_each(h, [&] {
                 return gc::launch_ens_map_events(s, h->d_evt_code, field_len(h), map_channels(h), G, B, c.c_out, Cs, T,
                                                  h->d_map_events + (size_t)slot * T * gc::kMapEventPlanes * N);
               });
             },
             no_readbacks);
  if (rc) return rc;
  h->map.blocks = gc::map_event_blocks(N);
  h->map_M[(size_t)slot] = h->ens_members;
  ++h->map_dates[(size_t)2 * slot + 1];
  return GC_OK;
  });
}

int gc_ens_map_download(gc_handle* h, int32_t slot, double* sums, uint32_t* counts, uint32_t* events, int64_t* dates) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_graph(h)) || (rc = map_plan(h)) || (rc = map_slot(h, slot, 0)) || (rc = need_out(h, sums && counts))) return rc;
  if (events && h->map_T == 0) return fail(h, GC_ERR_INVALID_ARGUMENT, "the map plan has no event planes (gc_ens_map_set)");
  GC_HIP(h, hipSetDevice(h->device));
  const size_t N = map_points(h), T = (size_t)h->map_T;
  static_assert(sizeof(unsigned) == sizeof(uint32_t), "the counts are copied out as they lie");
  if ((rc = read_back(h, sums, h->d_map_sums + (size_t)slot * gc::kMapSums * N, gc::kMapSums * N)) ||
      (rc = read_back(h, reinterpret_cast<unsigned*>(counts), h->d_map_counts + (size_t)slot * gc::kMapCounts * N, gc::kMapCounts * N)) ||
      (events && (rc = read_back(h, reinterpret_cast<unsigned*>(events), h->d_map_events + (size_t)slot * T * gc::kMapEventPlanes * N,
                                 T * gc::kMapEventPlanes * N))))
    return rc;
  GC_HIP(h, hipStreamSynchronize(h->stream));
  if (dates) {
    dates[0] = h->map_dates[(size_t)2 * slot];
    dates[1] = h->map_dates[(size_t)2 * slot + 1];
  }
  return GC_OK;
  });
}

int gc_ens_map_reset(gc_handle* h, int32_t slot) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_graph(h)) || (rc = map_plan(h)) || (rc = map_slot(h, slot, -1))) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  const size_t N = map_points(h), T = (size_t)h->map_T;
  const size_t first = slot < 0 ? 0 : (size_t)slot, n = slot < 0 ? (size_t)h->map_L : 1;
  hipStream_t s = h->stream;                       // behind every accumulate enqueued so far
  GC_HIP(h, hipMemsetAsync(h->d_map_sums + first * gc::kMapSums * N, 0, n * gc::kMapSums * N * sizeof(double), s));
  GC_HIP(h, hipMemsetAsync(h->d_map_counts + first * gc::kMapCounts * N, 0, n * gc::kMapCounts * N * sizeof(unsigned), s));
  if (T)
    GC_HIP(h, hipMemsetAsync(h->d_map_events + first * T * gc::kMapEventPlanes * N, 0,
                             n * T * gc::kMapEventPlanes * N * sizeof(unsigned), s));
  for (size_t l = first; l < first + n; ++l) {
    h->map_M[l] = 0;
    h->map_dates[2 * l] = h->map_dates[2 * l + 1] = 0;
  }
  return GC_OK;
  });
}

}  // extern "C"
