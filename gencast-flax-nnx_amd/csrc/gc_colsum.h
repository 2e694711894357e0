// Column sums of the ensemble scorers (gc_ensemble.hip, gc_region.hip, gc_clim.hip, gc_efi.hip, gc_order.hip, gc_tail.hip,
// gc_multivar.hip, gc_fss.hip, gc_events.hip): the thread layout over column tiles, the fold of a column's node lanes,
// the two sums over the per-block partials, and the host helpers that size the grids.  DESIGN.md section 8r.  Every sum formed here has ONE order, so the same call twice returns identical bytes.
//
// Thread layout (that of gc_loss_reduce_kernel, gc_kernels.hip).  A grid node's B rows are W = B c_out consecutive floats.
// W is cut into column tiles of tile_w columns, the last one narrower: tile_w = 256 (the 256-wide cut), or the equal
// width ceil(W / tiles) of a unit that chooses its number of tiles.  A workgroup has 256 threads, of which `cap` <= 256
// may own an accumulator set.  Inside a tile of wt columns thread t owns column t % wt (ONE accumulator set) of node lane
// t / wt; there are q = cap / wt lanes, and the threads of lane >= q idle.  Block x walks the contiguous node range
// [x per, (x + 1) per) in steps of q, so the threads of a wave read consecutive floats.  A column's total is then formed
// in three fixed steps: a thread's nodes ascending, the q lanes in lane order, the blocks by one of the two block sums.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

// (the pragma leaks to the end of the including file: every includer with floating-point arithmetic sets it anyway)
#pragma clang fp contract(off)

namespace gc {

struct ColTile {
  int col0, wt, q, lane, cl, col;
  // tile: blockIdx.y in the passes, blockIdx.x in a finish kernel that has one workgroup per tile
  __device__ ColTile(int tile_w, int cap, int W, int tile) {
    col0 = tile * tile_w;
    wt = min(tile_w, W - col0);
    q = cap / wt;
    lane = (int)threadIdx.x / wt;
    cl = (int)threadIdx.x - lane * wt;
    col = col0 + cl;
  }
  __device__ bool active() const { return lane < q; }
  // the node walk of block x over (G, per): for (n = n_begin(per); n < n_end(G, per); n += q)
  __device__ int n_begin(int per) const { return (int)blockIdx.x * per + lane; }
  __device__ int n_end(int G, int per) const { return min(G, (int)(blockIdx.x + 1) * per); }
};

// The q lane values of column c, added in lane order l = 0, 1, ..: lane l's value lies at a[l wt + c].  In place on
// whatever LDS row holds them (a staging array, or the row of one accumulator); no barrier in here: the caller has one
// between the writes of `a` and this call.
template <typename T>
__device__ inline T lane_fold(const T* a, int c, int wt, int q) {
  T t = a[c];
  for (int l = 1; l < q; ++l) t += a[l * wt + c];
  return t;
}

// The column total of a value every thread holds in a register: staged in stage[256], then lane_fold.  The total comes
// back on the threads tid < wt (the others get 0).  Barrier contract: EVERY thread of the workgroup calls this, under
// uniform control flow (idle threads pass zeros nobody reads); it has a barrier behind the staging and one behind the
// fold, so `stage` is free again on return and LDS writes made before the call are visible after it.
template <typename T>
__device__ inline T col_total(T* stage, T v, const ColTile& ct) {
  const int tid = threadIdx.x;
  stage[tid] = v;
  __syncthreads();
  const T t = tid < ct.wt ? lane_fold(stage, tid, ct.wt, ct.q) : T(0);
  __syncthreads();
  return t;
}

// ---- the two sums over the blocks: different roundings, both fixed ------------------------------------------------------

// Lane-split block sum (one workgroup per column tile): lane l adds its contiguous range [l bper, (l + 1) bper) of a
// list of n blocks, bper = ceil(n / q), ascending from 0.0; the lanes are then folded in lane order.  The partial of list
// entry i lies at from[list(i) * stride].  Barrier contract and result as col_total.
struct AllBlocks {                               // the list 0, 1, .., n - 1 (what gc_ens_finish_kernel's own text sums)
  __device__ int operator()(int i) const { return i; }
};
struct ListedBlocks {                            // an index list, ascending (a region's blocks)
  const int* sel;
  __device__ int operator()(int i) const { return sel[i]; }
};
template <class List>
__device__ inline double lane_split_block_sum(double* stage, const ColTile& ct, const double* __restrict__ from,
                                              size_t stride, int n, List list) {
  const int bper = (n + ct.q - 1) / ct.q;
  double t = 0.0;
  if (ct.active()) {
    const int i_end = min(n, (ct.lane + 1) * bper);
#pragma unroll 8
    for (int i = ct.lane * bper; i < i_end; ++i) t += from[(size_t)list(i) * stride];
  }
  return col_total(stage, t, ct);
}

// Ascending block finish: one thread per result adds the blocks of a sum from 0, b = 0, 1, ...  A unit gives a map, by
// value: sums() doubles, then counts() counts (unsigned partials, unsigned long long results); sum(e) / count(e) say
// where the partials of result e lie (from[b * stride]) and where the total goes (out[to] / outc[to]); from == nullptr:
// the index stands for no result (a column past W).  Where skipped.ipart is set, one more thread adds those
// skipped.per_block words of every block into outc[skipped.to].
template <typename T>
struct BlockSum {
  const T* from;
  size_t stride, to;
};
struct SkippedSum {
  const unsigned* ipart = nullptr;
  int per_block = 0;
  size_t to = 0;
};

template <class Map>
__global__ __launch_bounds__(256) void gc_block_finish_kernel(const Map map, int blocks, double* __restrict__ out,
                                                               unsigned long long* __restrict__ outc) {
  const int nd = map.sums(), nc = map.counts();
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < nd) {
    const BlockSum<double> r = map.sum(e);
    if (!r.from) return;
    double t = 0.0;
#pragma unroll 8
    for (int b = 0; b < blocks; ++b) t += r.from[(size_t)b * r.stride];
    out[r.to] = t;
  } else if (e < nd + nc) {
    const BlockSum<unsigned> r = map.count(e - nd);
    unsigned long long t = 0ull;
#pragma unroll 8
    for (int b = 0; b < blocks; ++b) t += r.from[(size_t)b * r.stride];
    outc[r.to] = t;
  } else if (e == nd + nc && map.skipped.ipart) {
    unsigned long long t = 0ull;
    for (int i = 0; i < blocks * map.skipped.per_block; ++i) t += map.skipped.ipart[i];
    outc[map.skipped.to] = t;
  }
}

template <class Map>
static hipError_t launch_block_finish(hipStream_t s, const Map& map, int blocks, double* out, unsigned long long* outc) {
  const int total = map.sums() + map.counts() + (map.skipped.ipart ? 1 : 0);
  hipLaunchKernelGGL(gc_block_finish_kernel<Map>, dim3((total + 255) / 256), dim3(256), 0, s, map, blocks, out, outc);
  return hipGetLastError();
}

// node-range blocks of a pass with q node lanes: 8 nodes per thread or more, at most cap_blocks
static int node_blocks(int G, int q, int cap_blocks) { return std::max(1, std::min((G + 8 * q - 1) / (8 * q), cap_blocks)); }

// dynamic LDS of the ensemble and the region pass: float[M][256], a point's members in the thread's own column (a bank of
// its own for every lane), then unsigned[wt][M + 1] rank counts
static size_t ens_score_lds(int M, int W) { return (size_t)M * 256 * sizeof(float) + (size_t)std::min(256, W) * (M + 1) * sizeof(unsigned); }

}  // namespace gc
