// Declarations of the kernel launchers, included by gc_kernels.h once per namespace (no include guard):
//   gc      -- the kernels as compiled from gc_kernels.hip (3 fp16 MFMAs per product),
//   gc_a16  -- the SAME source compiled with -DGC_TU_A16: the weight-streaming GEMM / MLP / FFW / out-projection
//              kernels instantiated with A16 = true (activation operand exact fp16, "fp16 node features":
//              2 MFMAs per product, identical bits).  A second translation unit, compiled beside the first,
//              instead of twice the instantiations in one (which took the build from 75 s to 3 minutes).
namespace GC_KERNELS_NS {

// Kernel classes, used for per-class profiling and as kernel-name prefixes.
enum KernelClass : int {
  KC_COND = 0,      // noise-level encoder + all conditioning vectors
  KC_PACK,          // grid input packing / sampler elementwise
  KC_MLP,           // fused GNN MLP (+LN +cond +residual)
  KC_SEGSUM,        // CSR segment sum
  KC_ROWOP,         // residual add (+ split-K slab sum) + LayerNorm + cond of the mesh rows
  KC_GEMM_QKV,      // QKV projection
  KC_ATTN,          // k-hop sparse attention
  KC_ATTN_COMBINE,  // (no kernel is filed under it: the out-projection's loader merges the key splits; kept for the ABI)
  KC_GEMM_OUT,      // attention out-projection (slab)
  KC_GEMM_FFW1,     // FFW layer 1 + gelu
  KC_GEMM_FFW2,     // FFW layer 2 (split-K slabs)
  KC_GEMM_NODE,     // per-node halves of the edge MLPs' first layer
  KC_NOISE,         // spherical white noise: Philox normals + Legendre / Fourier synthesis
  KC_COUNT
};

constexpr int kTileM = 32;          // rows per block tile (one 32x32 MFMA tile high)
constexpr int kCondDim = 16;

// One source of input columns for the fused MLP (concatenated along K).
struct Segment {
  const float* ptr;    // source rows
  const int* index;    // per-item gather index, or nullptr (identity)
  const float* affine; // per-batch [scale(width) | offset(width)] applied on load, or nullptr
  int width;           // columns, multiple of 32
  int ld;              // source row stride (floats)
  int bcast;           // 1: source has no batch axis (row = item), 0: row = item*B + b
};

// A per-node product gathered per row and added to the first layer's pre-activation.
// The three of a first layer without a product (MlpArgs::nseg == 0) are added in float32 in this order: add[0] (the
// per-noise-level edge term T), add[1] (sender), add[2] (receiver), then b1.
struct AddTerm {
  const float* ptr;    // [nodes * B][hidden] float32
  const int* index;    // per-item node index; nullptr: the item itself (a per-ROW term, e.g. the cached static part of the grid embedding)
};

struct MlpArgs {
  Segment seg[3];
  int nseg;            // 0 (weight-streaming form, f16x3, hidden 256): no first-layer product, pre-activation = add terms + b1
  AddTerm add[3];
  int nadd;
  int rows;            // items * B
  int B;
  int hidden;          // 128 / 256 / 512
  const float* w1t;    // [hidden][ldw1]  (transposed, K padded)
  int ldw1;
  const float* b1;     // [hidden]
  const float* w2t;    // [n_out_pad][hidden]
  const float* b2;     // [n_out_pad]
  int n_out;           // real output columns
  int n_out_pad;       // multiple of 128
  int do_ln;
  const float* cond;   // per-batch [scale(n_out) | offset(n_out)], or nullptr
  int cond_stride;     // floats between batch elements in cond / affine buffers
  const float* residual; // [rows][n_out] or nullptr
  float* out;          // [rows][ldo]
  int ldo;
  int f16;             // 1: w1t / w2t are S16-encoded; inputs are split on the fly (f16x3 products)
  // weight-streaming form (f16x3 only; used when w1f != nullptr; with add terms w1f is the edge block's image, K = k1f):
  const float* w1f;    // WF16 fragment-order image of W1^T, K zero-padded to k1f
  int k1f;             // padded K of w1f, multiple of 64, >= sum of segment widths
  const float* w2f;    // WF16 image of W2^T [n_out_pad][hidden]
  const float* ones;   // >= 512 ones / zeros: the identity affine of segments without one
  const float* zeros;
  // "fp16 node features" mode (gc_set_option features=f16; rounding points: DESIGN.md section 3b):
  int round16;         // 1: staged inputs, the hidden activation and the second Linear's output are rounded to fp16
  int round_out;       // 1: the LayerNorm + conditioning output and the residual sum are rounded to fp16
  int a16;             // 1 (only with round16): staged inputs and hidden tile are exact fp16 -- the CALLER then launches
                       // the gc_a16 build of the kernel (2 MFMAs per product: the lo planes are zero); identical bits
  // gc_a16 build only (physical fp16 activation storage): segment sources, `residual` and `out` are _Float16
  // arrays behind the float* fields (same element strides), except where these say otherwise:
  int seg0_f32;        // 1: segment 0 is a float32 source (packed grid input, statically embedded latents, structural features)
  int out_f32;         // 1: `out` is float32 (static embeddings, the decoder's network output)
  int f32w;            // 1 (with f16 == 0): exact-f32 family on the weight-streaming form -- w1f / w2f are WF32 images
  // weight-streaming form only: rows come as triples (item 3 g + s, s = 0..2, of unit u = g * B + b; rows = 3 x units) and
  // the epilogue stores out[u] = the float32 sum, in ascending s, of the triple's LayerNorm + conditioning results (each
  // rounded to fp16 first when round_out) -- the mesh2grid edge update with jraph.segment_sum folded in (no residual)
  int tri;
};
// true when launch_mlp runs `a` on the weight-streaming kernel (the only one with the triple epilogue, MlpArgs::tri);
// launch_mlp and mlp_pair_supported decide by it
bool mlp_runs_weight_streaming(const MlpArgs& a);

hipError_t launch_cond(hipStream_t s, const float* sigma_dev, float sigma_scalar, int B,
                       const float* w0t, const float* b0, const float* w1t, const float* b1,
                       int nfreq, int nhid, float base_period,
                       const float* wc_all, const float* bc_all, int total, float* cond_vec,
                       float* cond_out);

// Conditioning of up to kMaxSigmaList denoiser calls in one launch (sampler): cond_out[call][b][total]
constexpr int kMaxSigmaList = 96;
struct SigmaList { float v[kMaxSigmaList]; };
hipError_t launch_cond_multi(hipStream_t s, const SigmaList& sl, int ncalls, int B, const float* w0t,
                             const float* b0, const float* w1t, const float* b1, int nfreq, int nhid,
                             float base_period, const float* wc_all, const float* bc_all, int total,
                             float* cond_out);

hipError_t launch_mlp(hipStream_t s, const MlpArgs& a);
// Two independent MLPs in ONE launch (workgroups [0, tiles(a)) run a, the rest b), when both take the same kernel form
// (mlp_pair_supported: 8-wave weight-streaming form -- hidden 256 below 24 000 rows, or hidden 512 --, one precision
// family, no triple epilogue)
bool mlp_pair_supported(const MlpArgs& a, const MlpArgs& b);
hipError_t launch_mlp_pair(hipStream_t s, const MlpArgs& a, const MlpArgs& b);

hipError_t launch_segsum(hipStream_t s, const float* src, const int* rowptr, const int* eids,
                         int n_items, int n_edges, int B, int width, float* out, bool round16 = false,
                         bool h16 = false /* src and out are _Float16 arrays (implies rounding) */,
                         float norm = 0.f /* != 0: the float32 sum is divided by it before it is stored */);

struct GemmArgs {
  const float* a;      // [rows][lda]
  int lda;
  int a_f32;           // f16 mode only: 1 = A holds plain float32 and is split to S16 while staging
  // att_S > 0: A is the attention output merged on the fly from att_S key-split partials
  // (launch_attention's part_o / part_ml); `a` is then unused.  Only with 32-row tiles, epi 1.
  const float* att_po;
  const float* att_pml;
  int att_S, att_B, att_H, att_DH;
  // gc_gemm_rowop only, with att_S == 0: per attention tile (first partial slot, number of partial pieces); a tile with
  // pieces > 0 was cut into key-range pieces by the attention launch's work-item list and its rows of A are merged
  // from att_po / att_pml instead of read from `a`.  nullptr: every row comes from `a`.
  const int* att_tiles;
  const float* wt;     // W^T: [n][ldw]
  int ldw;
  int rows, n;
  int k_slice;         // K handled by one split (multiple of 32); split z covers [z*k_slice, (z+1)*k_slice)
  int splits;          // filled in by launch_gemm
  const float* bias;   // [n] or nullptr (epi 0)
  int act;             // 1: gelu(tanh) (epi 0)
  float* out;          // epi 0: [rows][ldo]; epi 1: slabs [splits][rows][ldo]
  int ldo;
  int round16;         // fp16-feature mode: epi 0 outputs and the merged attention output are rounded to fp16
  int a16;             // weight-streaming forms: A holds exact fp16 values (every producer rounds in fp16-feature mode) --
                       // the CALLER then launches the gc_a16 build, which leaves out the A-lo x W-hi MFMA; identical bits
  // epi 3 (QKV projection, weight-streaming form): besides out [rows][3d] f32, K and V are written
  // ALREADY SPLIT as fp16 planes for the attention kernel: kv16[row] = [K_hi(d) | K_lo(d) | V_hi(d) | V_lo(d)]
  void* kv16;
  int kv_d;            // d_model (n == 3 * kv_d)
  int out_f32;         // gc_a16 build, epi 0: `out` is float32 (the per-node pre-activation terms of a split edge MLP)
  int f32w;            // weight-streaming forms: 1 = exact-f32 family -- wt is a WF32 image, products on v_mfma_f32_32x32x2_f32
};
// LDS-staged form: 32x128 tiles (256 threads);
// epi 0: bias/act f32 store, 1: raw split-K slabs (f32),
// 2: bias/act store in S16 split-fp16 layout (f16 only).  f16: A and W^T are S16-encoded and the
// product runs as 3 fp16 MFMAs per k-step (f32-equivalent accuracy, see gc_kernels.hip).
hipError_t launch_gemm(hipStream_t s, int cls, const GemmArgs& g, int splits, int epi, bool f16);
// Weight-streaming f16x3 form: g.wt is the WF16 fragment-order image of W^T (gc_weights.hip
// encode_wf16), g.ldw the full contraction length K; a is plain float32 (or attention partials).
// Tile (32*mt) x 128, mt 1 or 2; needs n % 128 == 0 and k_slice a multiple of 128.  epi 0 | 1 as launch_gemm;
// epi 3 = QKV projection with pre-split K / V planes (g.kv16, g.kv_d).
hipError_t launch_gemm_ws(hipStream_t s, int cls, const GemmArgs& g, int mt, int splits, int epi);
#ifdef GC_STAMPS
hipError_t set_gemm_ws_stamp_buffer(unsigned long long* p);     // diagnostic builds: 10 words per wave
#endif

// Both feed-forward layers in one launch (gc_ffw_fused): slab[z] = gelu(a @ W1[:, Fz] + b1[Fz]) @ W2[Fz, :]
// for hidden slices Fz of 256 columns; the hidden activations never leave LDS.  f16x3, WF16 weights.
struct FfwArgs {
  const float* a;      // [rows][d] float32 (the normed + conditioned residual stream)
  int rows, d, f;      // d = 128 or 256, f % 256 == 0
  const float* w1f;    // WF16 image of W1^T [f][d]
  const float* b1;     // [f]
  const float* w2f;    // WF16 image of W2^T [d][f]
  float* out;          // [f/256][rows][d] partial sums, one slab per hidden slice
  int round16;         // fp16-feature mode: the hidden activation is rounded to fp16
  int a16;             // 1 (only with round16): a and the hidden tile are exact fp16 -- the caller launches the gc_a16 build
  // diagnostic builds only (-DGC_STAMPS, tools/stamp_ffw.cpp): 8 s_memtime stamps per wave, or nullptr
  unsigned long long* stamps;
  int f32w;            // 1: exact-f32 family -- w1f / w2f are WF32 images (gc_weights.hip encode_wf32), products on v_mfma_f32_32x32x2_f32
};
hipError_t launch_ffw_fused(hipStream_t s, const FfwArgs& g);

// Row pass fused behind a full-width projection (gc_gemm_rowop): after y = A @ W (n == K == d_model,
// no K split), x <- x + bias + y and h <- cond(LayerNorm(x)), i.e. gc_rowop with one slab.
struct RowFuse {
  float* x;            // [rows][n] residual stream, updated in place
  const float* bias;   // [n] or nullptr
  const float* cond;   // per-batch [scale(n) | offset(n)]
  int cond_stride;
  int B;
  float* h;            // [rows][n]
  int round16;         // fp16-feature mode: x and h are rounded to fp16 when stored
};
// g as for launch_gemm_ws (WF16 weights; optional attention partials as A); g.out is unused.
hipError_t launch_gemm_rowop(hipStream_t s, int cls, const GemmArgs& g, const RowFuse& f);
#ifdef GC_STAMPS
hipError_t set_gemm_rowop_stamp_buffer(unsigned long long* p);   // diagnostic builds: 8 words per wave
#endif

// x += bias + sum of slabs (in place; skipped when both absent); h = cond(LN(x)) when h != nullptr
hipError_t launch_rowop(hipStream_t s, float* x, const float* bias, const float* partials, int n_slabs,
                        int rows, int d, int B, const float* cond, int cond_stride, float* h,
                        int h_s16 /* 0: [rows][d]; 1: S16 */,
                        bool round16 = false, bool h16 = false /* x and h are _Float16 arrays (implies rounding) */);

// Exact-f32 attention.  S == 1: writes o directly; S > 1: writes partial (m, l, O) per key split, merged by the
// out-projection's A loader (GemmArgs::att_S)
hipError_t launch_attention(hipStream_t s, const float* qkv, float* o, float* part_o, float* part_ml,
                            int M, int B, int D, int H, int S, bool out_s16,
                            const int* tile_chunk_start, const int* union_idx, const unsigned* mask_bits,
                            int n_tiles, bool feat16 = false,
                            const int* items = nullptr /* work-item list, as launch_attention_v2 (S == 1) */, int n_items = 0);
// Attention on pre-split K / V planes (kv16 as written by launch_gemm_ws epi 3); q from qkv (f32).
// Always writes per-split partials when S > 1, o when S == 1 (as launch_attention).
hipError_t launch_attention_v2(hipStream_t s, const float* qkv, const void* kv16, float* o, float* part_o,
                               float* part_ml, int M, int B, int D, int H, int S, const int* tile_chunk_start,
                               const int* union_idx, const unsigned* mask_bits, int n_tiles,
                               int max_chunks_per_tile, bool feat16,
                               bool h16 = false /* with feat16: q is a _Float16 array [M*B][D], o a _Float16 array */,
                               const int* items = nullptr /* work-item list [n_items][4] = (tile, first chunk, end chunk, partial
                                                             slot or -1 = whole tile, output final); tile < 0: padding */,
                               int n_items = 0);
#ifdef GC_STAMPS
hipError_t set_attention_stamp_buffer(unsigned long long* p);   // diagnostic builds: 12 words per wave
#endif

// grid input packing: xp[rows][kp] = [struct(3) | feats(c_in) | 0...]
hipError_t launch_pack_full(hipStream_t s, const float* grid_struct, const float* feats, int G, int B,
                            int c_in, int kp, float* xp);
// xp[row][3 + slot[c]] = scale * x[row][c]
hipError_t launch_write_noisy(hipStream_t s, const float* x, const int* slots, int rows, int c_out,
                              int kp, float scale, float* xp);
// xn[row][c] = scale * x[row][c] (compact form, row stride ldn)
hipError_t launch_write_noisy_compact(hipStream_t s, const float* x, int rows, int c_out, int ldn, float scale, float* xn);
// xp[row][3 + slot[c]] = 0: the noisy-target columns of the packed input carry nothing once the noisy channels travel in
// the compact array (whatever the caller left there must not meet the zero weights as NaN / Inf)
hipError_t launch_zero_slots(hipStream_t s, const int* slots, int rows, int c_out, int kp, float* xp);
// out[item*B+b][c] = src[item][c] * scale[b][c] + offset[b][c]   (statically embedded latents)
hipError_t launch_affine_rows(hipStream_t s, const float* src, const float* cond, int cond_stride,
                              int items, int B, int w, float* out, bool round16 = false,
                              bool h16 = false /* out is a _Float16 array */);
// f16x3 domain guard: *counter += (number of workgroups that saw a NaN / Inf in p[0..n)); p 16-byte aligned
hipError_t launch_finite_check(hipStream_t s, const float* p, size_t n, unsigned* counter);
// Optional second output of the three sampler-state kernels below: the value also goes, times `scale` (the NEXT denoiser
// call's c_in), into the noisy-target slots of the packed grid input -- xp[row][3 + slots[c]] = scale * v, what
// launch_write_noisy does as a launch of its own.  xp == nullptr: off.
constexpr int kItemPieces = 4;   // most key-range pieces an attention tile is cut into by a work-item list (gc_forward.hip build_attention_items)
struct NoisyWrite {
  const int* slots = nullptr;
  int c_out = 1, kp = 0;
  float scale = 0.f;
  float* xp = nullptr;
  // compact form (the sampler with the cached static grid embedding): xn[row][c] = scale * v, row stride ldn -- the noisy
  // channels side by side in slot order instead of scattered over the packed input's columns
  float* xn = nullptr;
  int ldn = 0;
  bool active() const { return xp != nullptr || xn != nullptr; }
};
// dst = a * src
hipError_t launch_scale(hipStream_t s, const float* src, float a, size_t n, float* dst, const NoisyWrite& nw = NoisyWrite());
// Per-channel context update of the packed conditioning (gc_rollout_advance; kinds in gencast_hip.h).
hipError_t launch_rollout_advance(hipStream_t s, const float* old_feats, const float* sample, const float* forcings,
                                  const int* kind, const int* src, const int* sidx, const float* a, const float* b,
                                  int rows, int c_in, int c_out, int n_forcing, float* new_feats);
// den = c_out*y + c_skip*x ; mid = a_mid*x + (1-a_mid)*den
hipError_t launch_dpm_first(hipStream_t s, const float* y, const float* x, float c_out, float c_skip,
                            float a_mid, size_t n, float* den, float* mid, const NoisyWrite& nw = NoisyWrite());
// md = c_out*y + c_skip*xmid ; x = a_next*x + (1-a_next)*md
hipError_t launch_dpm_second(hipStream_t s, const float* y, const float* xmid, float c_out,
                             float c_skip, float a_next, size_t n, float* x, const NoisyWrite& nw = NoisyWrite());

// Denoising loss, forward only (gencast/gencast.py:229-280, common/losses.py:58-180); sigma [B] is a DEVICE array.
//   launch_loss_noisy   x = t + sigma_b nz;  xp[row][3 + slots[c]] = c_in(sigma_b) x
//   launch_loss_reduce  part[block][B][c_out] (double) = sum over the block's nodes of node_w (y + c_in (nz - sigma t))^2,
//                       loss_reduce_blocks(G, B, c_out) blocks; den != nullptr: also den = c_out y + c_skip x (else x is unused)
//   launch_loss_finish  blocks added in index order, times chan_w, folded into groups by chan_group:
//                       per_group[b][g] = c_out(sigma_b)^2 (...), loss[b] = lambda(sigma_b) sum_g group_w[g] per_group[b][g]
constexpr int kLossMaxBlocks = 2048;          // 8 workgroups of 4 waves per CU: a memory-bound pass wants the waves
constexpr int kLossMaxGroups = 64;
constexpr size_t kLossMaxLds = 32 * 1024;      // launch_loss_finish: (B c_out + B n_groups) doubles
int loss_reduce_blocks(int G, int B, int c_out);
hipError_t launch_loss_noisy(hipStream_t s, const float* t, const float* nz, const float* sigma, const int* slots, int rows,
                             int B, int c_out, int kp, float* x, float* xp);
hipError_t launch_loss_reduce(hipStream_t s, const float* y, const float* t, const float* nz, const float* x,
                              const float* sigma, const float* node_w, int G, int B, int c_out, double* part, float* den);
hipError_t launch_loss_finish(hipStream_t s, const double* part, int blocks, const float* sigma, const float* chan_w,
                              const int* chan_group, const float* group_w, int B, int c_out, int n_groups, float* loss,
                              float* per_group);

// Spherical white noise (gc_noise.hip): `count` N(0,1) values from Philox4x32-10 (key, stream), and the
// two-step synthesis out = (base ? base : 0) + scale * field, field [n_lat * n_lon][N] from coef [2][L][L][N].
hipError_t launch_noise_normals(hipStream_t s, float* out, size_t count, unsigned long long key,
                                unsigned long long stream);
hipError_t launch_noise_synthesis(hipStream_t s, const float* leg, const float* ctab, const float* stab,
                                  const float* coef, float* f, int L, int n_lat, int n_lon, int N,
                                  const float* base, float scale, float* out);

const char* kernel_class_name(int cls);

}  // namespace GC_KERNELS_NS
