// Regional ensemble scores on the device (include/gencast_hip.h, gc_ens_region_*): the sums of gc_ens_score for R regions
// of grid nodes from ONE scoring pass over the nodes that belong to any region.  Kernels and their host code live together
// here; DESIGN.md section 8m has the plan, the kernels and the error bound.
//
// node_bits[g] (uint32, bit r set = node g belongs to region r, r < R <= 32) says where a node belongs; regions may overlap,
// and a node with node_bits == 0 belongs to nothing: it is never read and counted nowhere.
// Per region r, over the nodes with bit r set, the sums S0..S5, the rank histogram and the skipped points are those of
// gc_ensemble.hip, with the handle's node weights.  Per point (g, b, c), in double:
//   m  = (sum_i x_i) / M                       ascending slot order
//   s2 = sum_i (x_i - m)^2 / (M - 1)           two passes, ascending slot order
//   ae = (sum_i |x_i - y|) / M
//   d  = sum_{i<j} |x_i - x_j| / (M (M-1) / 2)
//   r  = #{i : x_i < y}                        a member equal to y is not below it
// A point counts when y and all M members are finite.
//
// The plan (gc_ens_region_set, host code).  An ATOM is a distinct non-zero value of node_bits: the nodes of an atom belong
// to the same regions.  order[] lists the nodes with node_bits != 0 grouped by atom (ascending atom value), ascending in
// node index inside an atom.  The block table cuts order[] into ranges {begin, end} that each lie inside ONE atom: an atom
// of n_a nodes gets ceil(n_a / per) blocks, per = ceil(n / base) with base = loss_reduce_blocks(n, B, c_out) for the n listed
// nodes, so blocks <= base + atoms <= base + 256.  A block's partial sums are sums over nodes of one atom; region r is the sum
// of the blocks whose atom has bit r.  The per-point work is done once per listed point, whatever R is.
// No atomics on floats: every partial has one writer and every sum a fixed order (a thread's nodes in order[] order, the
// node lanes of a column in lane order, the blocks in index order), so the same call twice returns identical bytes.  The
// rank counts are integers; their LDS atomics commute.
#include <map>

#include "gc_colsum.h"
#include "gc_store.h"

// the per-point arithmetic is the definition above, operation for operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace gc {

constexpr int kRegionMax = 32, kRegionMaxAtoms = 256;
constexpr int kRegionMaxBlocks = kLossMaxBlocks + kRegionMaxAtoms;   // base + one ragged block per atom at the most

// The scoring pass, on the 256-wide cut of gc_colsum.h, but block x walks order[begin, end) of its table entry blk[2 x],
// blk[2 x + 1] in steps of q instead of a contiguous node range.  Dynamic LDS:
// ens_score_lds (nothing scales with R).  Out, as plain stores: part[block x][6][W] (double), hpart[block x][W][M + 1],
// ipart[block x][tile] (points skipped).
__global__ __launch_bounds__(256) void gc_ens_region_kernel(const float* __restrict__ mem, size_t field, int M,
                                                             const float* __restrict__ truth,
                                                             const float* __restrict__ node_w,
                                                             const int* __restrict__ order, const int* __restrict__ blk,
                                                             int W, double* __restrict__ part,
                                                             unsigned* __restrict__ hpart, unsigned* __restrict__ ipart) {
  extern __shared__ __attribute__((aligned(16))) unsigned char reg_lds[];
  __shared__ double lane_sum[256];
  __shared__ unsigned skipped;
  float* const tile = reinterpret_cast<float*>(reg_lds);
  unsigned* const hist = reinterpret_cast<unsigned*>(tile + (size_t)M * 256);
  const ColTile ct(256, 256, W, blockIdx.y);
  const int tid = threadIdx.x;
  const int bins = M + 1;
  for (int i = tid; i < ct.wt * bins; i += 256) hist[i] = 0u;
  if (tid == 0) skipped = 0u;
  __syncthreads();
  double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned inv = 0;
  if (ct.active()) {
    float* const my = tile + tid;                  // x_k at my[k * 256]
    const double dM = (double)M, pairs = 0.5 * dM * (dM - 1.0);
    const int p_end = blk[2 * blockIdx.x + 1];
    for (int p = blk[2 * blockIdx.x] + ct.lane; p < p_end; p += ct.q) {
      const int n = order[p];
      const size_t i = (size_t)n * W + ct.col;
      const float y = truth[i];
      bool xfin = true;
      double sum = 0.0;
#pragma unroll 4
      for (int k = 0; k < M; ++k) {
        const float x = mem[(size_t)k * field + i];
        my[k * 256] = x;
        xfin = xfin && isfinite(x);
        sum += (double)x;
      }
      if (!(xfin && isfinite(y))) {
        ++inv;
        continue;
      }
      const double m = sum / dM, yd = (double)y;
      double s2 = 0.0, ae = 0.0;
      int r = 0;
#pragma unroll 4
      for (int k = 0; k < M; ++k) {                // the second pass
        const float x = my[k * 256];
        const double dx = (double)x - m;
        s2 += dx * dx;
        ae += fabs((double)x - yd);
        r += x < y ? 1 : 0;
      }
      s2 /= dM - 1.0;
      double d0 = 0.0, d1 = 0.0;                    // two chains: the pair sum has no prescribed order
      for (int a = 0; a + 1 < M; ++a) {
        const double xa = (double)my[a * 256];
        int b = a + 1;
        for (; b + 1 < M; b += 2) {
          d0 += fabs(xa - (double)my[b * 256]);
          d1 += fabs(xa - (double)my[(b + 1) * 256]);
        }
        if (b < M) d0 += fabs(xa - (double)my[b * 256]);
      }
      const double w = (double)node_w[n], e = m - yd;
      s[0] += w;
      s[1] += w * e;
      s[2] += w * (e * e);
      s[3] += w * s2;
      s[4] += w * (ae / dM);
      s[5] += w * ((d0 + d1) / pairs);
      atomicAdd(&hist[ct.cl * bins + r], 1u);
    }
  }
  if (inv) atomicAdd(&skipped, inv);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double t = col_total(lane_sum, s[k], ct);
    if (tid < ct.wt) part[((size_t)blockIdx.x * 6 + k) * W + ct.col] = t;
  }
  unsigned* const hp = hpart + ((size_t)blockIdx.x * W + ct.col0) * bins;
  for (int i = tid; i < ct.wt * bins; i += 256) hp[i] = hist[i];
  if (tid == 0) ipart[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = skipped;
}

// One workgroup per (column tile, region r).  The blocks whose atom bits[b] has bit r are listed in LDS in ascending order
// (blocks <= kRegionMaxBlocks); the six sums of a column are the lane-split block sum (gc_colsum.h) over that list.
// sums [R][6][W]; hist [R][W][M + 1], then [R] words: the points of each region the call skipped.
__global__ __launch_bounds__(256) void gc_ens_region_finish_kernel(const double* __restrict__ part,
                                                                    const unsigned* __restrict__ hpart,
                                                                    const unsigned* __restrict__ ipart,
                                                                    const unsigned* __restrict__ bits, int blocks, int W,
                                                                    int M, double* __restrict__ sums,
                                                                    unsigned long long* __restrict__ hist) {
  __shared__ double lane_sum[256];
  __shared__ unsigned long long skipped;
  __shared__ int sel[kRegionMaxBlocks];              // the blocks of region r, ascending
  __shared__ int sel_at[257];
  const int r = blockIdx.y, R = gridDim.y, tiles = gridDim.x;
  const unsigned bit = 1u << r;
  const ColTile ct(256, 256, W, blockIdx.x);
  const int col0 = ct.col0, wt = ct.wt, col = ct.col;
  const int tid = threadIdx.x;
  const int bins = M + 1;
  // The list first, so that the sums below are loops of independent loads: thread t looks at the contiguous blocks
  // [t chunk, (t + 1) chunk), the counts are added up in thread order, and every thread writes its own at its offset.
  const int chunk = (blocks + 255) / 256;
  const int c_begin = min(blocks, tid * chunk), c_end = min(blocks, (tid + 1) * chunk);
  int mine = 0;
  for (int b = c_begin; b < c_end; ++b) mine += (bits[b] & bit) ? 1 : 0;
  sel_at[tid + 1] = mine;
  if (tid == 0) {
    skipped = 0ull;
    sel_at[0] = 0;
  }
  __syncthreads();
  if (tid == 0)
    for (int t = 1; t <= 256; ++t) sel_at[t] += sel_at[t - 1];
  __syncthreads();
  for (int b = c_begin, at = sel_at[tid]; b < c_end; ++b)
    if (bits[b] & bit) sel[at++] = b;
  __syncthreads();
  const int n_sel = sel_at[256];
  for (int k = 0; k < 6; ++k) {
    const double tot = lane_split_block_sum(lane_sum, ct, part + (size_t)k * W + col, (size_t)6 * W, n_sel, ListedBlocks{sel});
    if (tid < wt) sums[((size_t)r * 6 + k) * W + col] = tot;
  }
  for (int e = tid; e < wt * bins; e += 256) {
    unsigned long long t = 0ull;
#pragma unroll 8
    for (int i = 0; i < n_sel; ++i) t += hpart[((size_t)sel[i] * W + col0) * bins + e];
    hist[((size_t)r * W + col0) * bins + e] = t;
  }
  if (blockIdx.x == 0) {
    unsigned long long t = 0ull;
    for (int i = tid; i < n_sel * tiles; i += 256) t += ipart[(size_t)sel[i / tiles] * tiles + i % tiles];
    if (t) atomicAdd(&skipped, t);
    __syncthreads();
    if (tid == 0) hist[(size_t)R * W * bins + r] = skipped;
  }
}

static hipError_t launch_ens_region(hipStream_t s, const float* mem, size_t field, int M, const float* truth, const float* node_w,
                                    const int* order, const int* blk, int blocks, int W, double* part, unsigned* hpart,
                                    unsigned* ipart) {
  const size_t lds = ens_score_lds(M, W);
  if (lds > 64 * 1024) {                           // (a per-device property of the kernel; setting it again is harmless)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gc_ens_region_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(gc_ens_region_kernel, dim3(blocks, (W + 255) / 256), dim3(256), lds, s, mem, field, M, truth, node_w, order,
                     blk, W, part, hpart, ipart);
  return hipGetLastError();
}

static hipError_t launch_ens_region_finish(hipStream_t s, const double* part, const unsigned* hpart, const unsigned* ipart,
                                           const unsigned* bits, int blocks, int R, int W, int M, double* sums,
                                           unsigned long long* hist) {
  hipLaunchKernelGGL(gc_ens_region_finish_kernel, dim3((W + 255) / 256, R), dim3(256), 0, s, part, hpart, ipart, bits, blocks,
                     W, M, sums, hist);
  return hipGetLastError();
}

}  // namespace gc

using namespace gci;

namespace {

// The device side of the plan and everything sized by it and by M, one BufferGroup: replaced as a whole.  The plan itself
// stays on the host (h->reg_plan), so a store of another M gets its buffers without a new gc_ens_region_set.
int region_buffers(gc_handle* h, int M) {
  GC_HIP(h, h->reg_allocs.drop(h->stream));          // nothing reads the old ones any more
  const int W = h->cfg.batch * h->cfg.c_out, R = h->reg_R;
  const size_t blocks = (size_t)h->reg_blocks, tiles = (size_t)(W + 255) / 256, bins = (size_t)M + 1;
  int rc;
  if ((rc = alloc_all(h, h->reg_allocs, buf(&h->d_reg_plan, h->reg_plan.size()), buf(&h->d_reg_part, blocks * 6 * W),
                      buf(&h->d_reg_hpart, blocks * W * bins + blocks * tiles), buf(&h->d_reg_sums, (size_t)R * 6 * W),
                      buf(&h->d_reg_hist, (size_t)R * W * bins + R))))
    return rc;
  if (!h->reg_plan.empty()) {
    GC_HIP(h, hipMemcpyAsync(h->d_reg_plan, h->reg_plan.data(), h->reg_plan.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    GC_HIP(h, hipStreamSynchronize(h->stream));
  }
  h->reg_allocs.key = {(size_t)M};                   // (only now: a failed upload leaves buffers the next call replaces)
  return GC_OK;
}

}  // namespace

extern "C" {

int gc_ens_region_set(gc_handle* h, int32_t n_regions, const uint32_t* node_bits) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (!node_bits) return fail(h, GC_ERR_INVALID_ARGUMENT, "null argument");
  if (n_regions < 1 || n_regions > gc::kRegionMax) return fail(h, GC_ERR_UNSUPPORTED, "n_regions must be in 1..32");
  const int G = h->hg.G, R = n_regions;
  const uint32_t beyond = R == 32 ? 0u : ~0u << R;
  std::map<uint32_t, std::vector<int>> atoms;        // ascending atom value; the nodes of an atom ascending
  size_t listed = 0;
  for (int g = 0; g < G; ++g) {
    if (node_bits[g] & beyond) return fail(h, GC_ERR_INVALID_ARGUMENT, "node " + std::to_string(g) + " has a bit at or above n_regions");
    if (node_bits[g] == 0u) continue;
    atoms[node_bits[g]].push_back(g);
    ++listed;
    if (atoms.size() > (size_t)gc::kRegionMaxAtoms)
      return fail(h, GC_ERR_UNSUPPORTED, "more than 256 atoms (distinct non-zero values of node_bits)");
  }
  // the plan, as it lies on the device: order [listed], then {begin, end} [blocks], then the atom of every block [blocks]
  std::vector<int> order, table, bits;
  order.reserve(listed);
  if (listed) {
    const int base = gc::loss_reduce_blocks((int)listed, h->cfg.batch, h->cfg.c_out);
    const int per = ((int)listed + base - 1) / base;
    for (const auto& a : atoms) {
      const int begin = (int)order.size(), n_a = (int)a.second.size();
      order.insert(order.end(), a.second.begin(), a.second.end());
      for (int b = begin; b < begin + n_a; b += per) {
        table.push_back(b);
        table.push_back(std::min(b + per, begin + n_a));
        bits.push_back((int)a.first);
      }
    }
  }
  if (bits.size() > (size_t)gc::kRegionMaxBlocks) return fail(h, GC_ERR_INTERNAL, "the block table is longer than base + atoms");
  GC_HIP(h, hipSetDevice(h->device));
  GC_HIP(h, h->reg_allocs.drop(h->stream));          // the old plan is in force until here
  h->reg_R = R;
  h->reg_listed = (int)listed;
  h->reg_blocks = (int)bits.size();
  h->reg_plan = std::move(order);
  h->reg_plan.insert(h->reg_plan.end(), table.begin(), table.end());
  h->reg_plan.insert(h->reg_plan.end(), bits.begin(), bits.end());
  // with a store the buffers are made now, so that a set / reserve / set sequence holds the same number throughout
  return h->ens_members ? region_buffers(h, h->ens_members) : GC_OK;
  });
}

int gc_ens_region_score(gc_handle* h, const float* truth, double* sums, uint64_t* hist, uint64_t* invalid) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_graph(h)) || (rc = need(h, h->reg_R != 0, "no regions (gc_ens_region_set)")) || (rc = need_store(h)) ||
      (rc = need_out(h, sums)) || (rc = store_complete(h, h)) || (rc = need_weights(h)))
    return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, h, truth, "gc_ens_region_score"))) return rc;
  const gc_config& c = h->cfg;
  const int W = c.batch * c.c_out, M = h->ens_members, R = h->reg_R, blocks = h->reg_blocks;
  if (h->reg_allocs.differs({(size_t)M}) && (rc = region_buffers(h, M))) return rc;   // a store of another M since the plan was set
  const int* const order = h->d_reg_plan;
  const int* const table = order + h->reg_listed;
  const unsigned* const bits = reinterpret_cast<const unsigned*>(table + 2 * (size_t)blocks);
  unsigned* const ipart = h->d_reg_hpart + (size_t)blocks * W * (M + 1);
  hipStream_t s = h->stream;
  const size_t n_hist = (size_t)R * W * (M + 1);
  std::vector<uint64_t> out(n_hist + R);
  rc = timed(h, h->reg,
             [&]() -> int {
               if (blocks > 0 && (rc = launch_each(h, [&] {
                     return gc::launch_ens_region(s, h->d_ens, field_len(h), M, h->d_ens_truth, h->d_ens_w, order, table, blocks, W,
                                                  h->d_reg_part, h->d_reg_hpart, ipart);
                   })))
                 return rc;
               return launch_each(h, [&] {
                 return gc::launch_ens_region_finish(s, h->d_reg_part, h->d_reg_hpart, ipart, bits, blocks, R, W, M, h->d_reg_sums,
                                                     h->d_reg_hist);
               });
             },
             [&]() -> int {
               if ((rc = read_back(h, sums, h->d_reg_sums, (size_t)R * 6 * W)) || (rc = read_back(h, out.data(), h->d_reg_hist, out.size())))
                 return rc;
               return GC_OK;
             });
  if (rc) return rc;
  int64_t total = 0;
  for (int r = 0; r < R; ++r) {
    total += (int64_t)out[n_hist + r];
    if (invalid) invalid[r] = out[n_hist + r];
  }
  h->reg.invalid = total;
  h->reg.blocks = blocks;                            // (the entries of the block table: one workgroup row each)
  if (hist)
    for (size_t i = 0; i < n_hist; ++i) hist[i] = out[i];
  return GC_OK;
  });
}

}  // extern "C"
