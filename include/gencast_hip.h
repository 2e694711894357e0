/*
 * gencast_hip.h -- C ABI of libgencast_hip.so: the MI355X-native GenCast denoiser
 * forward + DPM-Solver++2S sampling path.
 *
 * The reference (fgiral000/gencast-flax-nnx) has no FFI layer: this path sits
 * behind three Python call contracts.  Each entry point below
 * names the reference interface it replaces (file:line into the reference).
 *
 * Conventions
 *   - every function returns an int status: 0 = OK, non-zero = gc_status code;
 *     the text of the last error on a handle is gc_last_error(h)
 *     (gc_last_error(NULL) = last error of a failed gc_create on this thread);
 *   - no C++ exceptions cross this boundary; no torch / framework types;
 *   - the CALLER owns every host buffer passed in; the LIBRARY owns all device
 *     memory, inside the opaque handle;
 *   - one handle = one GPU = one HIP stream; handles are independent, so N host
 *     threads (or N processes) may drive N GPUs concurrently.  A handle is not
 *     re-entrant;
 *   - all tensors are float32, row-major, node-major / batch-minor:
 *     [nodes, batch, channels] exactly like the reference's flat layout
 *     (gencast/denoiser.py:770-807); index arrays are int32;
 *   - there is NO CPU fallback: without a usable HIP device gc_create fails with
 *     GC_ERR_NO_DEVICE.
 */
#ifndef GENCAST_HIP_H_
#define GENCAST_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GC_ABI_VERSION 1

typedef struct gc_handle gc_handle;

typedef enum gc_status {
  GC_OK = 0,
  GC_ERR_INVALID_ARGUMENT = 1, /* bad dims / null pointer / unknown name (Python side raises ValueError) */
  GC_ERR_NO_DEVICE = 2,        /* no HIP device, or device_id out of range */
  GC_ERR_HIP = 3,              /* a HIP runtime call failed; text in gc_last_error */
  GC_ERR_STATE = 4,            /* call order violated (e.g. gc_denoise before gc_finalize) */
  GC_ERR_UNSUPPORTED = 5,      /* valid request outside what the kernels are built for */
  GC_ERR_INTERNAL = 6,         /* a C++ exception (e.g. out of host memory) was caught at the boundary */
  GC_ERR_COMM = 7              /* RCCL could not be loaded, or an RCCL call failed */
} gc_status;

/*
 * Model dimensions.  Mirrors DenoiserArchitectureConfig / SparseTransformerConfig /
 * NoiseEncoderConfig (gencast/denoiser.py:47-139) plus the data widths the
 * reference infers lazily on first call (gencast/denoiser.py:343-352).
 */
typedef struct gc_config {
  int32_t latent_size;      /* GNN latent = MLP hidden width (latent_size, hidden_layers = 1) */
  int32_t d_model;          /* transformer width; must equal latent_size */
  int32_t num_heads;
  int32_t ffw_hidden;
  int32_t num_layers;
  int32_t c_in;             /* stacked input + forcing channels per grid node (262 for the nano task) */
  int32_t c_out;            /* predicted channels per grid node (82) */
  int32_t batch;            /* B: batch / members evaluated together on this GPU */
  int32_t noise_num_frequencies; /* NoiseEncoderConfig.num_frequencies (32) */
  int32_t noise_hidden;          /* NoiseEncoderConfig.output_sizes[0] (32); [1] is fixed at 16 */
  float   noise_base_period;     /* NoiseEncoderConfig.base_period (16.0); apply_log_first = True */
} gc_config;

typedef struct gc_sample_stats {
  int32_t denoiser_calls;   /* network evaluations executed (39, or 40 with the dead call) */
  float   device_ms;        /* HIP-event time of the whole loop on the handle's stream */
} gc_sample_stats;

/* Library / build info; callable without a GPU. */
int         gc_abi_version(void);
const char* gc_build_info(void);               /* "... src:<16 hex>": hash of the csrc/ sources the library was built from (build.sh) */
int         gc_device_count(void);             /* 0 when no HIP device is visible */
/* PCI bus id ("0000:c1:00.0") of visible device `device_id` into out[cap] (cap >= 16): lets the ranks of one
 * launch check, before any collective, that no two of them sit on the same GPU (RCCL refuses that, and the rank
 * that entered ncclCommInitRank first would never leave it).  GC_ERR_INVALID_ARGUMENT for a bad index / buffer. */
int         gc_device_pci_bus_id(int32_t device_id, char* out, int64_t cap);
const char* gc_last_error(const gc_handle* h);

/*
 * Replaces: Denoiser.__init__ / DenoiserArchitecture.__init__
 * (gencast/denoiser.py:153-170, 231-301): allocates the handle on `device_id`
 * with its own stream.
 */
int gc_create(const gc_config* cfg, int device_id, gc_handle** out);
void gc_destroy(gc_handle* h);

/*
 * Runtime options (string key / value), callable any time after gc_create:
 *   "precision" = "f16x3" (default) | "f32"
 *       f16x3: every GEMM-shaped product runs as 3 fp16 MFMAs on operands split into
 *              hi + lo/2048 (22 significant bits; measured parity identical to f32);
 *       f32:   v_mfma_f32_32x32x2_f32 (exact f32 FMA chains), about 1.8x slower end to end.
 *   The environment variable GC_PRECISION sets the default for new handles.
 *   f16x3 domain: every GEMM operand must be finite with |x| <= 65504.  Nothing is clamped: an
 *   operand outside that range (an un-normalised field, NaN, Inf) poisons the result with NaN / Inf,
 *   the library checks the result of every call on the device and RE-RUNS a poisoned call on the
 *   exact-f32 kernels, whose treatment of such inputs is the reference's (f32 arithmetic, NaN / Inf
 *   propagate).  gc_get_counter("range_fallbacks") counts those re-runs.  For the resident
 *   (asynchronous) sampler the check is resolved by the next gc_download_sample / gc_sync /
 *   gc_rollout_advance.  Weights beyond the domain switch the handle to f32 kernels for good.
 *   The static embeddings, which gc_finalize makes once for every call to read, are checked and re-made the same way.
 *   "features" = "f32" (default) | "f16"   -- BASELINE.json configs[4], "fp16 node features":
 *       every activation is rounded to fp16 (round to nearest even) where it is produced -- grid
 *       input features, MLP hidden and output, LayerNorm + conditioning outputs, residual sums,
 *       q / k / v, softmax weights, attention output, segment sums -- while weights, conditioning
 *       vectors, GEMM accumulation, LayerNorm statistics, the softmax max / sum and the segment-sum
 *       accumulation stay float32: the points where the reference upcasts
 *       (gencast/sparse_transformer_utils.py:42-76, common/deep_typed_graph_net.py:396-403).  Attention
 *       then runs one fp16 MFMA per product instead of three, every other product two.  With precision
 *       f16x3 the activations are also STORED as 2-byte fp16 arrays in HBM (grid / mesh / edge latents, the
 *       residual stream, q / k / v, attention output, FFW hidden activation, segment sums: half the
 *       activation bytes of every kernel; split-K slabs, attention partials, the statically embedded
 *       latents and the network output stay float32); with precision f32, and in the exact-f32 re-run
 *       of the domain guard, the same values live in float32 containers.  Tensors at this boundary
 *       stay float32; parity tolerance vs the oracle in the same mode: DESIGN.md 3b.
 *   "graphs" = "on" (default) | "off"   -- HIP-graph replay of the sampler.  The reference's sampler is ONE compiled
 *       program (the jax.lax.fori_loop of gencast/dpm_solver_plus_plus_2s.py:157-158); here a sample is ~3 500
 *       kernel launches whose sequence depends only on (noise levels, skip_dead_call, precision, features), so the
 *       second gc_sample* call with one signature is captured into a hipGraph and later ones are a single
 *       hipGraphLaunch (host cost per sample: milliseconds -> tens of microseconds; same kernels, same arguments,
 *       same order: bit-identical samples).  Samples with stochastic churn, per-class profiling or the debug stops
 *       are always enqueued eagerly.  GC_TUNE_GRAPH=0 sets the default to off.
 *   "hidden_layers" = "1" (default) .. "4"   -- DenoiserArchitectureConfig.hidden_layers (gencast/denoiser.py:108,135;
 *       common/mlp.py:157-199): hidden layers of every MLP of the grid2mesh / mesh2grid GNNs.  It fixes the parameter
 *       names (`...network.network.layers.{0,2,..,2 n}`), so it must be set before the first gc_load_weight
 *       (GC_ERR_STATE afterwards).  n >= 2 runs every MLP as a chain of n fused launches, in both feature modes (with
 *       "f16" every hidden activation is an fp16 rounding point, the hand-over between the launches a float32 container
 *       of fp16 values); the reference trains with 1 (training/train_helpers.py:137), the tuned one-launch-per-MLP path.
 *   "grid2mesh_aggregate_normalization" = "none" (default) | "<positive constant>"   -- the summed grid2mesh edge
 *       messages of every mesh node are divided by it (common/deep_typed_graph_net.py:396-410; gencast/denoiser.py:123,138).
 *   "edge_term_cache_mb" = "4096" (default) | "<MiB>"   -- cap of the per-noise-level cache the sampler keeps at latent
 *       256, batch 1, f16x3, float32 features: the edge block of the two edge MLPs' first layer times the
 *       conditioned static edge embeddings, and the conditioned mesh embedding, one slot per distinct noise level of the
 *       sampler's list, built by the first sample that brings the list.  A list whose terms need more than the cap (and
 *       "0") keeps the per-call products: same samples to float32 rounding.
 */
int gc_set_option(gc_handle* h, const char* key, const char* value);

/*
 * Replaces: DenoiserArchitecture._maybe_init graph construction
 * (gencast/denoiser.py:343-363, 443-600) and Transformer.__init__'s mask set-up
 * (gencast/sparse_transformer.py:555-567).  The caller supplies the static graph
 * (built by gencast-flax-nnx_amd/geometry.py, or any other source):
 *   g2m edges   grid -> mesh,  E1 of them   (senders index grid nodes)
 *   m2g edges   mesh -> grid,  E2 of them   (senders index mesh nodes)
 *   khop CSR    row i = mesh nodes node i attends to (must contain i)
 *   *_struct    structural features: nodes (cos theta, cos phi, sin phi) [N,3],
 *               edges (|d|, d)/max|d| [E,4]  (common/model_utils.py:445-495)
 *   mesh_xyz    [M,3] unit vectors, used only to choose a cache-friendly internal
 *               node order; may be NULL.
 * Mesh node numbering is the caller's; the library renumbers internally.
 */
int gc_set_graph(gc_handle* h,
                 int32_t num_grid_nodes, int32_t num_mesh_nodes,
                 int32_t num_g2m_edges, const int32_t* g2m_senders, const int32_t* g2m_receivers,
                 int32_t num_m2g_edges, const int32_t* m2g_senders, const int32_t* m2g_receivers,
                 const int32_t* khop_rowptr, const int32_t* khop_cols,
                 const float* grid_struct, const float* mesh_struct,
                 const float* g2m_edge_struct, const float* m2g_edge_struct,
                 const float* mesh_xyz);

/*
 * Replaces: nnx.update(model, state) of a restored checkpoint
 * (training/evaluation.py:119-187).  `name` is the Flax-NNX attribute path of the
 * parameter (gencast-flax-nnx_amd/weights.py lists all of them),
 * `data` is row-major float32 with flax's kernel orientation (in, out).
 * Unknown names fail with GC_ERR_INVALID_ARGUMENT, except the reference's dead
 * mesh2grid mesh-node update, which is accepted and ignored.
 */
int gc_load_weight(gc_handle* h, const char* name, const float* data,
                   const int64_t* shape, int32_t ndim);

/* Number of parameters still missing (0 = ready for gc_finalize). */
int gc_missing_weights(gc_handle* h, int32_t* count);

/*
 * Checks that graph + every weight are present, lays weights out for the kernels
 * and pre-computes the embeddings whose inputs are static.
 * Must be called once before gc_denoise / gc_sample; call it again after
 * re-loading weights.
 */
int gc_finalize(gc_handle* h);

/*
 * Replaces: Denoiser.__call__ (gencast/denoisers_base.py:28-52;
 * gencast/denoiser.py:172-202 -> DenoiserArchitecture.__call__ :303-341), at the
 * flat-array level: raw network output F(X; sigma).
 *   grid_feats  [G, B, c_in]  inputs ++ forcings (noisy targets already scaled by c_in(sigma))
 *   sigma       [B]           noise levels (> 0)
 *   out         [G, B, c_out]
 * Host pointers; the call returns after the result has been copied back.
 */
int gc_denoise(gc_handle* h, const float* grid_feats, const float* sigma, float* out);

/*
 * Which columns of grid_feats hold the noisy targets, in output-channel order
 * (reference: `forcings.assign(noisy_targets)` + sorted-name stacking,
 * gencast/denoiser.py:184,770-807).  Needed by gc_sample / gc_sample_resident.
 */
int gc_set_noisy_slots(gc_handle* h, const int32_t* slots /* [c_out] */);

/*
 * Replaces: Sampler.__call__ of DPM-Solver++2S
 * (gencast/samplers_base.py:22-44; gencast/dpm_solver_plus_plus_2s.py:47-177,
 * preconditioning :181-205); stochastic churn when gc_set_churn installed a schedule.
 *   cond_feats  [G, B, c_in]   inputs ++ forcings; the noisy-slot columns are ignored
 *   init_noise  [G, B, c_out]  unit-variance noise; x0 = init_noise * sigmas[0]
 *   sigmas      [n + 1]        descending noise levels ending in 0 (samplers_utils.py:395-412)
 *   skip_dead_call  1 = omit the last step's mid-point evaluation whose result the
 *               reference discards (dpm_solver_plus_plus_2s.py:148-153); same output
 *   out         [G, B, c_out]  the sample
 */
int gc_sample(gc_handle* h, const float* cond_feats, const float* init_noise,
              const float* sigmas, int32_t n, int32_t skip_dead_call,
              float* out, gc_sample_stats* stats);

/*
 * Device-resident variants for callers that keep state in HBM between calls
 * (ensemble / autoregressive drivers, bench.py).
 *   gc_upload_cond      copy cond_feats [G,B,c_in] into the handle (H2D)
 *   gc_upload_cond_dev  same from a DEVICE pointer on this GPU (e.g. the buffer an
 *                       RCCL broadcast just filled), D2D on the handle's stream
 *   gc_sample_resident  run the sampler on the resident cond_feats and the noise set with
 *                       gc_upload_noise; asynchronous unless `stats` is non-NULL (then it waits
 *                       for the loop to read its HIP-event time)
 *   gc_upload_noise     copy init_noise [G,B,c_out] into the handle (H2D)
 *   Host buffers handed to gc_upload_cond / gc_upload_noise / gc_rollout_advance are copied into
 *   pinned staging memory owned by the handle before the call returns: the caller may reuse them
 *   at once.
 *   gc_download_sample  copy the last sample back (D2H), synchronising the stream
 *   gc_sync             wait for the handle's stream
 * Ordering while a resident sample's f16x3 domain check is still unresolved (gc_sample_resident without stats has
 * returned, gc_download_sample / gc_sync / gc_rollout_advance not yet called): the possible exact-f32 re-run of that
 * sample must see the inputs it was drawn from.  gc_upload_noise / gc_noise_draw for the NEXT sample are free -- the
 * initial noise is double-buffered -- so "sample, upload the next member's noise, download" pipelines without a
 * wait.  Every other entry point that changes sampler inputs (gc_upload_cond, gc_upload_cond_dev, gc_commit_cond,
 * gc_comm_broadcast_cond, gc_set_noisy_slots, gc_set_churn, gc_noise_seed) first resolves the pending check, i.e.
 * waits for the stream; so do gc_upload_targets and gc_loss_resident (the targets are an input of the loss evaluations,
 * which share the guard and, with draw_noise, overwrite the initial-noise buffer).  A second gc_sample_resident before any of these discards the first sample's check with
 * its result.
 */
int gc_upload_cond(gc_handle* h, const float* cond_feats);
int gc_upload_cond_dev(gc_handle* h, const void* cond_feats_dev);
int gc_upload_noise(gc_handle* h, const float* init_noise);
int gc_sample_resident(gc_handle* h, const float* sigmas, int32_t n, int32_t skip_dead_call,
                       gc_sample_stats* stats);
int gc_download_sample(gc_handle* h, float* out);
int gc_sync(gc_handle* h);
/*
 * Download overlapped with the next step (autoregressive drivers): gc_stash_sample waits for the last sample,
 * resolves its domain check and snapshots it into a second device buffer (a stream-ordered device-to-device copy);
 * the handle can then be given the context update and the next sample at once, and gc_download_stash copies the
 * snapshot to the host on a side stream WHILE they run (returns when `out` is complete).  Replaces nothing in the
 * reference (`jax.device_get` there, common/rollout.py:357-360); it removes the host copy from the gap between two
 * forecast steps.
 */
int gc_stash_sample(gc_handle* h);
int gc_download_stash(gc_handle* h, float* out);

/*
 * Device pointer of the resident cond_feats buffer ([G,B,c_in] float32), so a
 * collective library can write into it directly (rank != 0 receives the RCCL
 * broadcast there).  Call gc_commit_cond afterwards to re-pack it.
 */
int gc_cond_device_ptr(gc_handle* h, void** ptr, int64_t* nbytes);
int gc_commit_cond(gc_handle* h);

/*
 * Spherical white noise on the device and stochastic churn.
 * Replaces: spherical_white_noise_like / sample (gencast/samplers_utils.py:250-346) for the initial
 * state (dpm_solver_plus_plus_2s.py:71-78) and apply_stochastic_churn (samplers_utils.py:434-452) inside
 * the solver loop (dpm_solver_plus_plus_2s.py:128-137; the reference's array version of that call is
 * missing, the Dataset version defines the arithmetic).
 *   gc_noise_set_tables  static tables of the inverse real-spherical-harmonic transform on the model's
 *                        lat/lon grid (n_lat * n_lon = G; node = lat_i * n_lon + lon_j):
 *                          legendre  [lmax][n_lat][lmax]  Pn[m][lat][l] = normalised P_l^m(sin lat) *
 *                                    sqrt(4 pi p_l / (2l+1)), zero for l < m
 *                          cos_table [n_lon][lmax], sin_table [n_lon][lmax]   (sqrt(2) folded in for m > 0)
 *                        (gencast-flax-nnx_amd/noise.py builds them)
 *   gc_noise_seed        Philox4x32-10 key and the stream the next field uses; every field drawn
 *                        (initial noise or churn) advances the stream by one
 *   gc_noise_draw        fills the handle's initial-noise buffer with a fresh unit-variance field
 *                        [G, B, c_out] (instead of gc_upload_noise)
 *   gc_download_noise    copies the initial-noise buffer back (tests)
 *   gc_set_churn         per-step churn rates (stochastic_churn_rate_schedule, samplers_utils.py:415-431)
 *                        and noise_level_inflation_factor for the following gc_sample* calls; n must
 *                        equal their number of steps; n = 0 or all-zero rates switch churn off.
 *                        Step i with rate > 0:  s' = s_i (1 + rate),
 *                        x += noise * sqrt(max(s'^2 - s_i^2, 0)) * inflation, then the 2S step runs from s'.
 */
int gc_noise_set_tables(gc_handle* h, int32_t n_lat, int32_t n_lon, int32_t lmax, const float* legendre,
                        const float* cos_table, const float* sin_table);
int gc_noise_seed(gc_handle* h, uint64_t seed, uint64_t stream);
int gc_noise_draw(gc_handle* h);
int gc_download_noise(gc_handle* h, float* out);
int gc_set_churn(gc_handle* h, const float* rates, int32_t n, float noise_level_inflation_factor);

/*
 * Denoising loss, forward only: "what is this checkpoint's loss on this batch at these noise levels".
 * Replaces: GenCast.loss (gencast/gencast.py:229-280) with losses.weighted_mse_per_level
 * (common/losses.py:58-180), at the flat-array level; no backward pass.  For batch member b with noise level s_b:
 *   x = t + s_b n;   F = network(cond with c_in(s_b) x in the noisy slots; s_b);   D = c_out(s_b) F + c_skip(s_b) x
 *   per_group[b][g] = sum over nodes i and the channels c of group g of node_weight[i] channel_weight[c] (D - t)^2
 *   loss[b]         = c_out(s_b)^-2  sum_g group_weight[g] per_group[b][g]
 * (the reference's per-variable mean: node_weight = unit-mean latitude weight / G, channel_weight = level weight /
 * channels of the variable, one group per variable -- gencast-flax-nnx_amd/losses.py loss_plan builds them).
 * The device evaluates lambda (D - t)^2 as (F + c_in (n - s t))^2, the same quantity without the cancellation at small
 * s, forms and adds every term in double in a fixed order (no atomics: results are bit-reproducible) and rounds once,
 * to the float32 results.
 *   gc_loss_set_weights   node_weight [G], channel_weight [c_out], channel_group [c_out] (values in [0, n_groups)),
 *                         n_groups in 1..64, group_weight [n_groups].  GC_ERR_UNSUPPORTED when
 *                         batch * (c_out + 64) * 8 bytes exceed 32 KiB (batch > 28 at c_out = 82): the finishing kernel is
 *                         one workgroup that keeps every column and group sum in LDS
 *   gc_upload_targets     targets [G, B, c_out] into the handle (H2D; the caller's buffer is free on return)
 *   gc_loss_resident      n_eval evaluations back to back on the resident conditioning (gc_upload_cond*) and targets;
 *                         sigmas [n_eval][B] (> 0).  draw_noise = 1: every evaluation draws a fresh spherical field into
 *                         the initial-noise buffer (gc_noise_seed streams, one stream per field); draw_noise = 0: every
 *                         evaluation uses the field that buffer holds (gc_upload_noise / gc_noise_draw).  Synchronous:
 *                         loss [n_eval][B] and per_group [n_eval][B][n_groups] come back in one download at the end.
 *                         n_eval <= 2^20; the per-evaluation device buffers (B * 66 floats per evaluation) grow by
 *                         doubling and, like every device buffer of a handle, are released by gc_destroy only.
 *                         Each evaluation is one forward in gc_denoise's form, enqueued eagerly (never captured, the
 *                         per-sample embedding cache is not engaged); conditioning, the last sample, captured sample
 *                         graphs and (with draw_noise = 0) the initial noise are left as they were.
 *   gc_download_denoised  D [G, B, c_out] of the LAST evaluation of the last gc_loss_resident / gc_loss
 *   gc_loss               host-pointer convenience for one evaluation: gc_upload_cond + gc_upload_targets +
 *                         gc_upload_noise + gc_loss_resident(n_eval = 1, draw_noise = 0) (+ gc_download_denoised when
 *                         `denoised` is not NULL)
 * GC_ERR_STATE before gc_finalize, gc_set_noisy_slots, the weights, the targets, the conditioning or the noise are in
 * place.  f16x3 domain guard as in gc_denoise: an evaluation whose F holds NaN / Inf is run again on the exact-f32
 * kernels from the same noise and counted in "range_fallbacks".
 */
int gc_loss_set_weights(gc_handle* h, const float* node_weight, const float* channel_weight,
                        const int32_t* channel_group, int32_t n_groups, const float* group_weight);
int gc_upload_targets(gc_handle* h, const float* targets);
int gc_loss_resident(gc_handle* h, const float* sigmas, int32_t n_eval, int32_t draw_noise,
                     float* loss, float* per_group);
int gc_download_denoised(gc_handle* h, float* out);
int gc_loss(gc_handle* h, const float* cond_feats, const float* targets, const float* noise, const float* sigma,
            float* loss, float* per_group, float* denoised /* NULL allowed */);

/*
 * Ensemble verification: score M members against one truth on the device.  The reference
 * project has no verification metrics; the yardstick is the closed-form definition in float64.
 * Members x_0 .. x_{M-1} and the truth y are [G, B, c_out] float32 in the sample layout; w [G] is a node weight.
 * A point (g, b, c) counts when y and all M members are finite there; other points contribute nothing (NaN truth
 * over land).  Per counted point, in double from the float32 values:
 *   m  = (sum_i x_i) / M  (ascending slot order),   s2 = sum_i (x_i - m)^2 / (M - 1)  (two passes),
 *   ae = (sum_i |x_i - y|) / M,   d = sum_{i<j} |x_i - x_j| / (M (M-1) / 2),
 *   r  = #{i : x_i < y} in 0..M   (ties are not randomised: a member equal to y is not below it)
 * Per column (b, c), over the counted nodes g:
 *   sums[0] = sum w, [1] = sum w (m - y), [2] = sum w (m - y)^2, [3] = sum w s2, [4] = sum w ae, [5] = sum w d,
 *   rank_hist[b][c][r] = points of rank r (unweighted: they add up to the counted nodes of the column).
 * The sums are raw and additive (batches, dates, ranks merge by addition); rmse = sqrt(S2/S0), spread = sqrt(S3/S0),
 * fair CRPS = (S4 - S5/2)/S0, ensemble CRPS = (S4 - (M-1)/M S5/2)/S0, bias = S1/S0 are formed by the caller
 * (gencast-flax-nnx_amd/verification.py).  Every term is formed and added in double, in a fixed order, with no atomics
 * on floats: a call's results are bit-reproducible.
 *   gc_ens_reserve          a store of n_members fields on the handle, n_members in 2..64 (else GC_ERR_UNSUPPORTED);
 *                           frees and replaces an earlier store and everything sized by it, and empties every slot
 *                           (also the mean / variance fields count as not computed again)
 *   gc_ens_set_node_weight  w [G] (H2D; the caller's array is free on return); kept across gc_ens_reserve
 *   gc_ens_push             slot <- the last sample of `src` (NULL: of h itself): one stream-ordered device-to-device
 *                           copy.  The source's pending f16x3 domain check is resolved first, as in gc_stash_sample (the
 *                           member is the checked sample).  With another handle the copy runs on the source's stream and
 *                           the two streams are ordered by events, not by a host wait for the copy.
 *                           GC_ERR_INVALID_ARGUMENT: slot outside [0, n_members); src on another device or with other
 *                           G / batch / c_out.  GC_ERR_STATE: src holds no sample.
 *   gc_ens_push_host        slot <- field [G, B, c_out] from the host through pinned staging (the caller's buffer is
 *                           free on return): a member that was produced elsewhere (another rank, a rollout step)
 *   gc_ens_score            truth: host [G, B, c_out], uploaded and kept, or NULL = the truth uploaded last.
 *                           sums [6][B][c_out] doubles; rank_hist [B][c_out][M + 1] (NULL allowed).  want_fields != 0:
 *                           the pass also writes m and s2 of every point into two handle-owned float32 fields (from the
 *                           members alone; NaN where a member is not finite).  Synchronous.
 *                           GC_ERR_STATE: a slot not pushed since gc_ens_reserve, no node weights, no truth.
 *   gc_ens_download_fields  mean and / or variance [G, B, c_out] of the last gc_ens_score that asked for them (either
 *                           pointer may be NULL); GC_ERR_STATE when none did since gc_ens_reserve
 * Everything except gc_ens_push needs gc_set_graph only (no weights, no gc_finalize).  None of these entries touches the
 * conditioning, the last sample, the stash, the loss buffers or the captured sample graphs.  Counters: "ens_scores"
 * (scoring calls so far), "ens_score_device_us" (HIP-event time of the last call's two kernels), "ens_invalid_points"
 * (points the last call skipped).
 */
int gc_ens_reserve(gc_handle* h, int32_t n_members);
int gc_ens_set_node_weight(gc_handle* h, const float* w /* [G] */);
int gc_ens_push(gc_handle* h, int32_t slot, gc_handle* src /* NULL = h */);
int gc_ens_push_host(gc_handle* h, int32_t slot, const float* field /* [G,B,c_out] */);
int gc_ens_score(gc_handle* h, const float* truth /* NULL = the truth uploaded last */, int32_t want_fields,
                 double* sums /* [6][B][c_out] */, uint64_t* rank_hist /* [B][c_out][M+1], NULL allowed */);
int gc_ens_download_fields(gc_handle* h, float* mean, float* variance);

/*
 * Ensemble rollouts resident on the device: every member keeps a conditioning of its own in a
 * context store on one handle, and what is scored at a lead time is each member's STATE, not its sample.  With the
 * InputsAndResiduals wrapper a sample is a normalised residual relative to that member's own previous frame, so from the
 * second step on the samples of different members are not comparable with each other or with one truth; the advanced
 * conditioning (gc_rollout_advance) holds the state itself, in the input normalisation, one channel per target channel.
 * The reference project rolls members out independently and verifies on the host (common/rollout.py); nothing there is
 * replaced arithmetically: every entry below is a copy or a gather, so a member is bit for bit the single-member rollout.
 *   gc_ctx_reserve          a store of n conditioning arrays [G, B, c_in] float32 on the handle, n in 1..64 (else
 *                           GC_ERR_UNSUPPORTED); frees and replaces an earlier store and empties every slot.  Needs
 *                           gc_set_graph only.  Released by gc_destroy.
 *   gc_ctx_save             slot <- the CURRENT conditioning of `src` (NULL: of h itself): one stream-ordered
 *                           device-to-device copy on the source's stream, made after the source's pending f16x3 domain
 *                           check is resolved.
 *   gc_ctx_load             the conditioning of `dst` (NULL: of h itself) <- slot, with the semantics of gc_upload_cond_dev:
 *                           the destination's pending domain check is resolved, then the copy and gc_commit_cond run on
 *                           the destination's stream.
 *   gc_ctx_download         slot -> host [G, B, c_in] (tests, checkpoints).  Synchronous.
 *                           Ordering between handles is by events per slot, never by a host wait for a copy: a copy out of a
 *                           slot starts after the last copy into it has ended, a copy into a slot after every earlier copy
 *                           into or out of it has ended, whichever streams they ran on.
 *                           GC_ERR_INVALID_ARGUMENT: slot outside [0, n); the other handle on another device or with other
 *                           G / batch / c_in.  GC_ERR_STATE: no store; a slot never saved since gc_ctx_reserve
 *                           (gc_ctx_load, gc_ctx_download); no conditioning on the source (gc_ctx_save); the other handle
 *                           not finalized.
 *   gc_ens_push_state       member slot of the gc_ens_* store <- the state of `src` (NULL: h itself), one gather launch:
 *                             member[row][j] = state_src[j] >= 0 ? cond_src[row][state_src[j]] : sample_src[row][j]
 *                           for every row (g, b) and output channel j; cond_src is the source's current conditioning (call
 *                           it AFTER gc_rollout_advance), sample_src its last sample.  No arithmetic.  state_src [c_out]:
 *                           every entry < c_in and not one of the source's noisy slots (GC_ERR_INVALID_ARGUMENT); negative
 *                           = the target channel has no input channel (gencast-flax-nnx_amd/rollout.py state_channels
 *                           derives the table from the rollout plan).  Guard resolution, stream and event ordering, and
 *                           the other errors as gc_ens_push; GC_ERR_STATE also when the source has no conditioning.
 *   gc_ens_download_member  one stored member [G, B, c_out] -> host (tests, checkpoints of an ensemble).  Synchronous.
 *                           GC_ERR_STATE: slot not pushed since gc_ens_reserve.
 * None of these entries touches the last sample, the stash, the loss buffers, the spectrum buffers or the captured sample
 * graphs; gc_ctx_load changes the conditioning, as gc_upload_cond_dev does, and nothing else.  The noise of a member that
 * changes handle between steps: counter "noise_stream" is the Philox stream the next drawn field will use (initial noise
 * and churn fields both advance it); read it after the member's sample and hand it to gc_noise_seed, with the member's
 * key, on whichever handle runs the member's next step.
 */
int gc_ctx_reserve(gc_handle* h, int32_t n);
int gc_ctx_save(gc_handle* h, int32_t slot, gc_handle* src /* NULL = h */);
int gc_ctx_load(gc_handle* h, int32_t slot, gc_handle* dst /* NULL = h */);
int gc_ctx_download(gc_handle* h, int32_t slot, float* out /* [G,B,c_in] */);
int gc_ens_push_state(gc_handle* h, int32_t slot, gc_handle* src /* NULL = h */, const int32_t* state_src /* [c_out] */);
int gc_ens_download_member(gc_handle* h, int32_t slot, float* out /* [G,B,c_out] */);

/*
 * Spherical-harmonic power spectra of fields and ensembles on the device: the analysis direction
 * of the transform gc_noise_* synthesises with.  The reference project has no spectral diagnostics; the yardstick is the
 * definition below in float64 (tests/spectrum_reference.py).
 * Grid: n_lat x n_lon nodes, node = lat_i n_lon + lon_j, latitudes ascending with the poles, phi_j = 2 pi j / n_lon (the
 * grid of gc_noise_set_tables).  Basis: the real orthonormal Y_lm of noise.py.  Band limit 0 <= m <= l < lmax <= n_lon / 2.
 * A field is [G, B, c_out] float32: N = B c_out independent columns.  amp_0 = 1, amp_m = sqrt(2):
 *   Fourier    Fc[m][lat] = sum_j f(lat, j) cos_a[m][j],  cos_a[m][j] = amp_m cos(m phi_j) / n_lon   (Fs: sin_a), j ascending
 *   Legendre   a_lm = sum_lat Q[m][l][lat] Fc[m][lat]  (b_lm from Fs), lat ascending; Q_m = pinv(A_m),
 *              A_m[lat][l] = N_lm P_l^m(sin lat), l = m .. lmax-1: least squares, not quadrature (the latitudes with poles
 *              cannot integrate degree 2 lmax); a field band-limited below lmax is recovered exactly
 *   power      power[l] = (sum_m a_lm^2 + b_lm^2) / (4 pi), m ascending, the cosine term before the sine term; each square is
 *              rounded before it is added.  For a band-limited field sum_l power[l] is the area mean of f^2.
 * The tables are float32 (built in float64 on the host: spectra.py); every product and sum on the device is binary64, the
 * Legendre step with fused multiply-adds.  Every sum has one writer and a fixed order (j, lat, m, members ascending) and
 * there are no atomics on floats: the same call twice returns identical bytes.
 * Ensemble spectra, of the members x_0 .. x_{M-1} of the gc_ens_* store and a truth y: the mean has the coefficients
 * (sum_i a_i) / M, formed on the coefficients in double, ascending slot order.  Per (b, c, l), six raw sums, additive over dates:
 *   sums[0] = power(y)            sums[1] = sum_i power(x_i)   sums[2] = power(mean)
 *   sums[3] = sum_i power(x_i-y)  sums[4] = power(mean - y)    sums[5] = sum_i power(x_i - mean)
 * every difference taken on the coefficients before squaring, every power() complete before it is added, members ascending.
 * A column (b, c) in which the truth or any member holds a value that is not finite is NaN in every output (a transform
 * cannot skip points); counter "spec_invalid_columns" counts those columns of the last call.
 *   gc_spec_set_tables  legendre_analysis [lmax m][lmax l][n_lat] (zero for l < m), cos_a / sin_a [lmax][n_lon].  Needs
 *                       gc_set_graph only.  GC_ERR_INVALID_ARGUMENT: n_lat n_lon != G, lmax outside 1 .. n_lon / 2.  Replaces
 *                       earlier tables and every buffer sized by them.
 *   gc_spec_field       power [B][c_out][lmax] of one field: host [G, B, c_out] (through pinned staging; the caller's buffer
 *                       is free on return), or NULL = the handle's last sample, where it lies, after its pending f16x3 domain
 *                       check is resolved as in gc_stash_sample.  Synchronous.  GC_ERR_STATE: no tables; NULL and no sample.
 *   gc_ens_spectrum     truth: host [G, B, c_out], uploaded and kept, or NULL = the truth uploaded last (shared with
 *                       gc_ens_score).  sums [6][B][c_out][lmax]; member_power [M][B][c_out][lmax] (NULL allowed): power(x_i).
 *                       Synchronous.  GC_ERR_STATE: no tables, no member store, a slot not pushed since gc_ens_reserve, no truth.
 * The Fourier step of one field ([2][lmax][n_lat][N] doubles) and the coefficient sets ([2][lmax][lmax][N] doubles each: one
 * for gc_spec_field, M + 2 for gc_ens_spectrum) live in handle-owned buffers: made again when the tables change or a call
 * needs more sets than there are, freed by gc_destroy.  None of these entries touches the conditioning, the last sample, the
 * stash, the loss buffers, the member store's contents or the captured sample graphs.  Counters: "spec_calls" (calls so
 * far), "spec_device_us" (HIP-event time of the last call), "spec_invalid_columns".
 */
int gc_spec_set_tables(gc_handle* h, int32_t n_lat, int32_t n_lon, int32_t lmax,
                       const float* legendre_analysis /* [lmax][lmax][n_lat] */, const float* cos_a /* [lmax][n_lon] */,
                       const float* sin_a /* [lmax][n_lon] */);
int gc_spec_field(gc_handle* h, const float* field /* [G,B,c_out], NULL = the last sample */, double* power /* [B][c_out][lmax] */);
int gc_ens_spectrum(gc_handle* h, const float* truth /* NULL = the truth uploaded last */, double* sums /* [6][B][c_out][lmax] */,
                    double* member_power /* [M][B][c_out][lmax], NULL allowed */);

/*
 * Ensemble event verification on the device: the exceedance events of the members of the gc_ens_*
 * store -- "10 m wind above the 99th percentile" -- counted against what the truth did, as the joint table the Brier score,
 * the reliability curve, the ROC and the relative economic value are formed from (gencast-flax-nnx_amd/verification.py
 * EventScores).  The reference project has no verification metrics; the yardstick is the definition below, restated in
 * tests/event_reference.py.  Everything the device returns is an INTEGER: results are compared with ==.
 * Members x_0 .. x_{M-1} (2 <= M <= 64) and the truth y are [G, B, c_out] float32.  T threshold fields thr_t (1 <= T <= 8),
 * each [G, B, c_out] float32 -- a climatological percentile varies per node and channel, and under the residual normalisation
 * of a single-step sample per batch member too -- with a direction dir_t:
 *   dir_t > 0: the event is value > thr_t;   dir_t < 0: value < thr_t.   Both strict, on the float32 values: a value equal
 *   to the threshold is not an event.  dir_t == 0 is an invalid argument.
 * A point (g, b, c) counts for threshold t when y, all M members and thr_t are finite there; other points contribute nothing
 * (a NaN threshold: "this channel or point is not evaluated").  Per counted point:
 *   k = #{i : x_i in the event} in 0..M,   o = [y in the event].
 * wq [G] uint32 are integer node weights (verification.quantize_node_weights: rint(w 2^e) in float64, 2^e the largest power
 * of two with max(w) 2^e <= 2^32 - 1); the device never sees a float weight here.  Per (t, b, c), over the counted nodes g:
 *   weighted[t][b][c][o][k] = sum wq[g],   counts[t][b][c][o][k] = sum 1,   invalid[t] = points skipped.
 * All uint64 and additive over dates and batches.  Integer addition has no order: the results are bit-reproducible however
 * the launch is scheduled.  A column total is at most G (2^32 - 1): for G <= 2^21 below 2^53, so the conversion to float64
 * and the division by 2^e are exact.  Per point and threshold the device keeps one byte, code = k | (o << 7), or 255 where the
 * point does not count: the exceedance-probability map k / M with the observed flag (verification.event_probability).
 *   gc_ens_event_set       T threshold fields, their directions and the integer node weights, through pinned staging (the
 *                          caller's arrays are free on return).  Needs gc_set_graph only.  Thresholds, directions, weights
 *                          and the code buffers do not depend on M and survive gc_ens_reserve; the tables, sized by M and
 *                          T, are made again by the scoring call that finds either changed.  Repeated calls replace, they
 *                          do not add ("device_allocations" stays flat).  Released by gc_destroy.
 *                          GC_ERR_UNSUPPORTED: T outside 1..8.  GC_ERR_INVALID_ARGUMENT: a zero direction, a null pointer.
 *   gc_ens_event_score     truth: host [G, B, c_out], uploaded and kept, or NULL = the truth uploaded last (the buffer
 *                          gc_ens_score and gc_ens_spectrum use).  weighted [T][B][c_out][2][M + 1]; counts (same shape)
 *                          and invalid [T] may be NULL.  Two launches: a code pass that streams the M members once, and a
 *                          table pass over the code bytes.  Synchronous.
 *                          GC_ERR_STATE: no thresholds set, no member store, a slot not pushed since gc_ens_reserve, no truth.
 *   gc_ens_event_download  the codes [G, B, c_out] of threshold t from the last scoring call.  GC_ERR_STATE: none ran since
 *                          gc_ens_event_set / gc_ens_reserve.  GC_ERR_INVALID_ARGUMENT: t outside [0, T).
 * None of these entries touches the conditioning, the last sample, the stash, the loss or spectrum buffers, the member
 * store's contents or the captured sample graphs.  Counters: "ens_event_calls" (scoring calls so far),
 * "ens_event_device_us" (HIP-event time of the last call's kernels), "ens_event_invalid_points" (sum over the thresholds of
 * the last call).
 */
int gc_ens_event_set(gc_handle* h, int32_t n_thresholds, const float* thresholds /* [T][G,B,c_out] */,
                     const int32_t* direction /* [T] */, const uint32_t* node_weight_q /* [G] */);
int gc_ens_event_score(gc_handle* h, const float* truth /* NULL = the truth uploaded last */,
                       uint64_t* weighted /* [T][B][c_out][2][M+1] */, uint64_t* counts /* same, NULL allowed */,
                       uint64_t* invalid /* [T], NULL allowed */);
int gc_ens_event_download(gc_handle* h, int32_t threshold, uint8_t* code /* [G,B,c_out] */);

/*
 * Derived and pooled ensemble fields on the device: 10 m wind speed, which is no model channel, and
 * spatially pooled fields -- "the maximum within r km", the area mean over a region -- formed from the members and the truth
 * of one handle's gc_ens_* store and left in the member store of a SECOND handle, on which every scorer of this library
 * (gc_ens_score, gc_ens_spectrum, gc_ens_event_*, gc_ens_download_member, gc_ens_download_fields) then works as it is.  The
 * reference project has no verification code; the yardstick is the definition below, restated in tests/derive_reference.py.
 * Source handle `src`: a full store of M members and a truth y, each [G, B, c_src] float32, G = n_lat n_lon, node =
 * lat_i n_lon + lon_j (the grid of gc_spec_set_tables).  Destination handle `dst`: the same device, G and batch; its own
 * c_out = c_d is the number of derived channels.  It needs gc_set_graph only.
 * Step 1, per derived channel j, with op[j], src_a[j], src_b[j] and affine[j] = (sa, la, sb, lb):
 *   COPY  (0)  d = x[src_a], the same bits, no arithmetic; src_b and affine are ignored
 *   NORM2 (1)  d = (float) sqrt(u u + v v) in double, u = (double) x[src_a] sa + la, v = (double) x[src_b] sb + lb, rounded
 *              once: wind speed in physical units from normalised components
 * Step 2, pool in {NONE 0, MAX 1, MIN 2, MEAN 3} of the float32 field d over the latitude-adaptive window
 *   Win(i, j) = {(i', (j + t) mod n_lon) : max(0, i - r_lat) <= i' <= min(n_lat - 1, i + r_lat), |t| <= r_lon[i']}
 * The longitude wraps, the latitude is clipped (nothing crosses a pole), and the width of a row is that of the row i', not
 * of the centre row: the window approximates a fixed distance on the sphere and is separable.  Per (b, channel) the output
 * at (i, j) is NaN iff the centre d(i, j) is not finite; else the window points that are not finite (NaN, +-inf) are skipped:
 *   MAX / MIN  the extreme of the finite window values (exact)
 *   MEAN       sum row_weight[i'] d / sum row_weight[i'] over the finite window points, in double, rounded once
 *   NONE       d
 * The truth goes through the same map.
 *   gc_ens_derive_set  the plan: op, src_a, src_b [c_d], affine [c_d][4], pool, the grid, r_lat >= 0, r_lon [n_lat] with
 *                      0 <= r_lon[i] <= (n_lon - 1) / 2, row_weight [n_lat] finite and > 0 (r_lon and row_weight may be
 *                      NULL when pool == 0).  Needs gc_set_graph only.  Through pinned staging: the caller's arrays are
 *                      free on return.  Replaces an earlier plan ("device_allocations" stays flat), survives
 *                      gc_ens_reserve, released by gc_destroy.  GC_ERR_STATE: no graph.  GC_ERR_INVALID_ARGUMENT: a null
 *                      pointer, n_lat n_lon != G, a source channel outside [0, c_src), r_lat < 0, r_lon[i] out of range, a
 *                      row_weight that is not finite and > 0.  GC_ERR_UNSUPPORTED: an unknown op or pool; a row that
 *                      does not fit the 64 KB row tile of the pooling pass (n_lon > 16384; with MEAN, n_lon > 5461).
 *   gc_ens_derive      every slot of dst's store becomes the derived member and counts as pushed; dst's truth buffer
 *                      becomes the derived truth, so truth = NULL works in every scorer of dst; dst's event codes and mean
 *                      / variance fields count as not computed.  truth: host [G, B, c_src], uploaded into and kept in
 *                      src's truth buffer as gc_ens_score(src, truth, ...) would, or NULL = src's last truth.  The
 *                      kernels run on dst's stream, ordered behind src's stream by an event.  Synchronous.
 *                      GC_ERR_INVALID_ARGUMENT: src is NULL, dst itself or on another device; src has no graph, another
 *                      G or batch, or c_out != c_src of the plan.  GC_ERR_STATE: no plan, no store on dst, no store on
 *                      src, the two stores differ in M, a src slot not pushed since its gc_ens_reserve, no truth.
 * Launches: a derive pass (the whole call with pool == 0), then per chunk of at most 8 of the M + 1 fields a row pass
 * (one latitude row pooled along the longitude in LDS, at a cost per output that does not grow with r_lon) and a column
 * pass over a handle-owned intermediate (8 fields of a float, or a double and an int32, per point: made again only when
 * its size changes).  No atomics: the same call twice returns identical bytes.  Nothing else on either handle is
 * touched: not the conditioning, the last sample, the stash, the loss or spectrum buffers, src's store contents or the
 * captured sample graphs.  Counters: "ens_derive_calls" (calls so far), "ens_derive_device_us" (HIP-event time of the
 * last call's launches).
 */
int gc_ens_derive_set(gc_handle* dst, int32_t c_src, const int32_t* op, const int32_t* src_a, const int32_t* src_b,
                      const double* affine /* [c_out][4] */, int32_t pool, int32_t n_lat, int32_t n_lon, int32_t r_lat,
                      const int32_t* r_lon /* [n_lat] */, const double* row_weight /* [n_lat] */);
int gc_ens_derive(gc_handle* dst, gc_handle* src, const float* truth /* [G,B,c_src] host, NULL = src's last truth */);

/*
 * Derived fields across levels and along the grid: a plan with four more ops for step 1 of
 * gc_ens_derive.  gc_ens_derive_set_expr takes everything gc_ens_derive_set takes, with the same meaning and the same
 * errors, plus the tables below; gc_ens_derive runs whichever plan was set last, and everything behind step 1 (pooling,
 * the truth, the stream order, the scorers of dst) is unchanged.  gc_ens_derive_set itself is unchanged.
 * In the new ops a source channel c enters in physical units, p(c) = (double) x[c] scale[c] + loc[c], with scale, loc
 * [c_src] finite.  All arithmetic is in double without fused multiply-adds, the result is rounded to float32 once, no
 * atomics are used and two calls give the same bytes; non-finite inputs propagate by IEEE rules.
 *   SUM  (2)   d = (float) S1,                       S = sum_t coef_t p(a_t) (b_t >= 0 ? p(b_t) : 1), the terms of a list
 *   NORM (3)   d = (float) sqrt(S1 S1 + S2 S2)       added in ascending t, each term formed as (coef p(a)) p(b)
 *              term_start [c_out][3] = (s0, s1, s2): list 1 is the terms [s0, s1) and list 2 [s1, s2) of the table term_coef,
 *              term_a, term_b [n_terms]; SUM has s2 == s1.  Read for SUM and NORM channels only.  Geopotential thickness,
 *              wind shear, one level of a variable, column integrals, integrated vapour transport.
 *   VORTICITY (4), DIVERGENCE (5) of u = p(src_a), v = p(src_b) on the grid node = i n_lon + j.  The host passes per row
 *              i: coslat[i] = cos(lat_i), inv_rcos[i] = 1 / (R cos(lat_i)) with R = 6 371 000 m, inv_dphi[i] =
 *              1 / (lat_i+ - lat_i-) in radians with i- = max(i - 1, 0), i+ = min(i + 1, n_lat - 1) (one-sided at the end
 *              rows; either latitude order), pole_row[i] != 0 where |lat_i| >= 90 - 1e-9, there with coslat[i] = 0 exactly;
 *              and inv_2dlam = 1 / (2 dlambda).  On a row that is no pole row, the longitude wrapping:
 *                zeta  = ((v[i,j+1] - v[i,j-1]) inv_2dlam - (u[i+,j] coslat[i+] - u[i-,j] coslat[i-]) inv_dphi[i]) inv_rcos[i]
 *                delta = ((u[i,j+1] - u[i,j-1]) inv_2dlam + (v[i+,j] coslat[i+] - v[i-,j] coslat[i-]) inv_dphi[i]) inv_rcos[i]
 *              On a pole row every j gets the mean over j of the adjacent row's double results, summed in ascending j and
 *              divided by n_lon: a pole is one point.  affine is ignored for these ops (and for SUM, NORM, COPY).
 * Caps: 64 terms in a list, 1024 in a plan (the table is staged in LDS); with a pole row, n_lon <= 8191.
 * GC_ERR_INVALID_ARGUMENT beyond those of gc_ens_derive_set: scale or loc NULL or not finite; n_terms < 0; a term table
 * pointer NULL with n_terms > 0, term_start NULL with a SUM / NORM channel; a term channel outside [0, c_src) (term_b: -1
 * allowed); a coefficient that is not finite; a term_start row that is not 0 <= s0 < s1 <= s2 <= n_terms, with s2 > s1 for
 * NORM and s2 == s1 for SUM; with a VORTICITY / DIVERGENCE channel: a row table NULL, n_lon < 3, n_lat < 2, a coslat or
 * inv_dphi that is not finite, inv_dphi or inv_2dlam zero, inv_rcos not finite on a row that is no pole row, a pole row
 * that is no end row, has coslat != 0, or lies next to another pole row.  GC_ERR_UNSUPPORTED: an op outside 0 .. 5, a list or
 * a plan beyond the caps, n_lon beyond the cap of the pole pass.  The row tables may be NULL without such a channel.
 * Launches: one derive pass, and with a pole row and a VORTICITY / DIVERGENCE channel a pole pass of a workgroup per
 * (derived column, end row, field).  The tables live in the plan's one buffer and are released with it.
 */
int gc_ens_derive_set_expr(gc_handle* dst, int32_t c_src, const int32_t* op, const int32_t* src_a, const int32_t* src_b,
                           const double* affine /* [c_out][4] */, int32_t pool, int32_t n_lat, int32_t n_lon, int32_t r_lat,
                           const int32_t* r_lon /* [n_lat] */, const double* row_weight /* [n_lat] */,
                           const double* scale /* [c_src] */, const double* loc /* [c_src] */,
                           const int32_t* term_start /* [c_out][3] */, int32_t n_terms, const double* term_coef,
                           const int32_t* term_a, const int32_t* term_b /* [n_terms] */, const double* coslat,
                           const double* inv_rcos, const double* inv_dphi /* [n_lat] */, double inv_2dlam,
                           const int32_t* pole_row /* [n_lat] */);

/*
 * Spectral band views on the device: the members and the truth of one handle's gc_ens_* store,
 * low-, band- or high-pass filtered per total wavenumber, left in the member store of a SECOND handle, on which every scorer
 * of this library then works as it is -- the CRPS of the planetary waves, a wind event on the field without its small
 * scales.  The reference project has no spectral diagnostics; the yardstick is the definition below in float64, restated in
 * tests/band_reference.py.
 * Grid, basis and analysis are those of gc_spec_set_tables on `dst` (n_lat x n_lon = G, lmax = L): the filter needs them.
 * A plan has K bands (1 <= K <= 8), each a response w_k[l] (float64, l < L, finite) and a flag complement_k, and per derived
 * channel j of dst (c_d = dst's c_out) a pair (src_channel[j], band[j]).  For one field -- a member or the truth -- and one
 * source column with data f, k = band[j]:
 *   1  a = analysis(f), the coefficients of gc_spec_field: once per DISTINCT source column, however many bands read it
 *   2  b[part][m][l] = w_k[l] a[part][m][l]                                                      in binary64, rounded
 *   3  G[part][m][lat] = sum_{l = m .. L-1} S[m][lat][l] b[part][m][l]                            l ascending, fused multiply-adds
 *      S = legendre_synthesis = float32(N_lm P_l^m(sin lat)): the plain A_m of the analysis, zero for l < m
 *   4  g(lat, j) = sum_m (cos_s[m][j] G[0][m][lat] + sin_s[m][j] G[1][m][lat])                    m ascending, the cosine term
 *      before the sine term, fused; cos_s[m][j] = float32(amp_m cos(m phi_j)), sin_s likewise, amp_0 = 1, else sqrt 2
 *   5  d = (float) g, or with complement_k d = (float) ((double) f - g): rounded once
 * Tables are float32 (built in float64 on the host: spectra.py), every product and sum on the device is binary64, every sum
 * has one writer and a fixed order, and the only atomics are the integer ORs of the analysis' flags: the same call twice
 * returns identical bytes.  complement is what makes a true high-pass: a grid field is not band-limited below L, f - low(f)
 * keeps the part of f outside the span of the basis, synth((1 - w) a) drops it.  The truth goes through the same map.
 * A source column of a field that holds a value that is not finite makes every derived channel reading it NaN at every
 * node of THAT field (a transform cannot skip points); other fields and columns are unaffected.  Counter
 * "ens_band_invalid_columns": the (field, batch member, distinct source channel) triples of the last call that were so.
 *   gc_ens_band_set  the plan.  Needs gc_set_graph and gc_spec_set_tables on dst (else GC_ERR_STATE).  Through pinned staging:
 *                    the caller's arrays are free on return.  Replaces an earlier plan ("device_allocations" stays flat),
 *                    survives gc_ens_reserve, released by gc_destroy; gc_spec_set_tables on dst drops it.
 *                    GC_ERR_UNSUPPORTED: K outside 1..8.  GC_ERR_INVALID_ARGUMENT: a null pointer, c_src < 1, a source
 *                    channel outside [0, c_src), a band index outside [0, K), a response value that is not finite.
 *   gc_ens_band      the contract of gc_ens_derive: every slot of dst's store becomes the band field and counts as pushed;
 *                    dst's truth buffer becomes the band truth; dst's event codes and mean / variance fields count as not
 *                    computed.  truth: host [G, B, c_src], uploaded into and kept in src's truth buffer, or NULL = src's
 *                    last truth.  The kernels run on dst's stream, ordered behind src's stream by an event.  Synchronous.
 *                    GC_ERR_INVALID_ARGUMENT: src is NULL, dst itself or on another device; src has no graph, another G or
 *                    batch, or c_out != c_src of the plan.  GC_ERR_STATE: no tables, no plan, no store on dst, no store on
 *                    src, the two stores differ in M, a src slot not pushed since its gc_ens_reserve, no truth.
 * Launches, per field (the M members, then the truth, one at a time): a gather of the distinct source columns, the two
 * analysis kernels of gc_spec_field, a Legendre synthesis with the response multiply in its loader, and a Fourier synthesis
 * whose epilogue subtracts, rounds and writes straight into dst's slot.  The scratch of ONE field (the gathered columns, the
 * two analysis steps, [2][L][n_lat][B c_d] doubles of the Legendre synthesis) and the flags are handle-owned and made again
 * only when their size changes.  Nothing else on either handle is touched.  Counters: "ens_band_calls" (calls so far),
 * "ens_band_device_us" (HIP-event time of the last call's launches), "ens_band_invalid_columns".
 */
int gc_ens_band_set(gc_handle* dst, int32_t c_src, int32_t n_bands, const double* response /* [K][lmax] */,
                    const int32_t* complement /* [K] */, const int32_t* src_channel /* [c_out] */,
                    const int32_t* band /* [c_out] */, const float* legendre_synthesis /* [lmax m][n_lat][lmax l], zero for l < m */,
                    const float* cos_s /* [lmax][n_lon] */, const float* sin_s /* [lmax][n_lon] */);
int gc_ens_band(gc_handle* dst, gc_handle* src, const float* truth /* [G,B,c_src] host, NULL = src's last truth */);

/*
 * Ensemble order statistics on the device: the M members of every point of the gc_ens_* store in
 * ascending order, and what follows from that order -- quantile fields (the median, a p10 / p90 band) and the bin sums of
 * Hersbach's (2000) decomposition of the ensemble CRPS into a reliability and a potential part (gencast-flax-nnx_amd/
 * verification.py OrderScores).  The reference project has no verification code; the yardstick is the definition below,
 * restated in float64 in tests/order_reference.py.
 * Members x_0 .. x_{M-1} (2 <= M <= 64) and the truth y are [G, B, c_out] float32, w [G] the node weights of
 * gc_ens_set_node_weight; per point x_(1) <= .. <= x_(M) are the member values in ascending order.  A point is member-valid
 * when all M members are finite, and counted when it is member-valid and y is finite (the rule of gc_ens_score).
 * Quantile fields, for Q probabilities p_q in [0, 1] (0 <= Q <= 8): the HOST forms h = p_q (M - 1), lo = min(floor(h), M - 1),
 * hi = min(lo + 1, M - 1), f = h - lo in double, per call from the current M, and the device computes at a member-valid point
 *   Q_q = (float)((double)x_(lo+1) + f ((double)x_(hi+1) - (double)x_(lo+1)))       no fused multiply-add; NaN elsewhere
 * -- NumPy's "linear" rule; p = 0 and p = 1 give the minimum and the maximum bit for bit.
 * Bin terms per counted point, in double (differences of float32 values are formed in double):
 *   0 < k < M:  c = min(max(y, x_(k)), x_(k+1)),  alpha_k = c - x_(k),  beta_k = x_(k+1) - c
 *   alpha_0 = 0,  beta_0 = max(x_(1) - y, 0);     alpha_M = max(y - x_(M), 0),  beta_M = 0
 * Per column (b, c), over the counted nodes g:
 *   bins[b][c][k] = (sum w alpha_k, sum w beta_k)       extra[b][c] = (sum w, sum w [y < x_(1)], sum w [y > x_(M)])
 *   pinball[b][c][q] = sum w u (p_q - [u < 0]),  u = (double)y - (double)Q_q (the stored float32 field value)
 *   counts[b][c][q] = #{y < Q_q} for q < Q,  counts[b][c][Q] = counted points          invalid = points not counted
 * Every term is formed and added in double; every partial sum has one writer and the order of addition is fixed (no atomics
 * on floats), so the same call twice returns identical bytes.  All outputs are raw and additive over batches and dates.
 * Hersbach's uncertainty and resolution need the climatological distribution of the observations, which is not additive
 * over dates: they are not formed here.
 *   gc_ens_order_set       the probabilities.  Needs gc_set_graph only; survives gc_ens_reserve (they do not depend on M);
 *                          replaces an earlier setting ("device_allocations" stays flat); released by gc_destroy.
 *                          GC_ERR_UNSUPPORTED: Q outside 0..8.  GC_ERR_INVALID_ARGUMENT: a probability that is NaN or
 *                          outside [0, 1]; probs NULL with Q > 0.
 *   gc_ens_order_score     truth: host [G, B, c_out], uploaded and kept, or NULL = the truth uploaded last (the buffer
 *                          gc_ens_score, gc_ens_spectrum and gc_ens_event_score use).  bins [B][c_out][M + 1][2] and extra
 *                          [B][c_out][3] are required; pinball [B][c_out][Q], counts [B][c_out][Q + 1] and invalid [1] may
 *                          be NULL.  Also leaves the Q quantile fields on the device.  Two launches: a pass that reads the
 *                          M members of a point once and sorts them in registers with a bitonic network, and a finish that
 *                          adds the per-block partials in block order.  Synchronous.
 *                          GC_ERR_STATE: no gc_ens_order_set, no member store, a slot not pushed since gc_ens_reserve, no
 *                          node weights, no truth.
 *   gc_ens_order_fields    the quantile fields only: the same pass without its truth-dependent half.  Needs neither
 *                          weights nor truth.  Synchronous.
 *   gc_ens_order_download  quantile field q [G, B, c_out] of the last order call.  GC_ERR_STATE: none ran since
 *                          gc_ens_order_set / gc_ens_reserve (/ gc_ens_derive into this handle).
 *                          GC_ERR_INVALID_ARGUMENT: q outside [0, Q).
 * None of these entries touches the conditioning, the last sample, the stash, the loss, spectrum, event or derive buffers,
 * the member store's contents, the mean and variance fields or the captured sample graphs.  Counters: "ens_order_calls"
 * (calls so far), "ens_order_device_us" (HIP-event time of the last call's launches), "ens_order_invalid_points" (of the
 * last scoring call).
 */
int gc_ens_order_set(gc_handle* h, int32_t n_quantiles, const double* probs /* [Q], NULL when Q = 0 */);
int gc_ens_order_score(gc_handle* h, const float* truth /* NULL = the truth uploaded last */,
                       double* bins /* [B][c_out][M+1][2] */, double* extra /* [B][c_out][3] */,
                       double* pinball /* [B][c_out][Q], NULL allowed */, uint64_t* counts /* [B][c_out][Q+1], NULL allowed */,
                       uint64_t* invalid /* [1], NULL allowed */);
int gc_ens_order_fields(gc_handle* h);                    /* quantile fields only: no truth read, no sums */
int gc_ens_order_download(gc_handle* h, int32_t q, float* field /* [G,B,c_out] */);

/*
 * An ensemble scored against a climatology on the device: the raw sums of the anomaly correlation
 * coefficient (ACC) of the ensemble mean and of the CRPS skill score (CRPSS) against a climatological ensemble
 * (gencast-flax-nnx_amd/verification.py ClimatologyScores).  The reference project has no verification code; the yardstick
 * is the definition below, restated in float64 in tests/clim_reference.py.
 * Members x_0 .. x_{M-1} come from the store of `h`, climatological samples c_0 .. c_{K-1} (past states for the same
 * calendar date) from the store of `clim`, a second handle -- graph-only will do -- on the same device with the same G,
 * batch and c_out, filled with gc_ens_reserve(clim, K) and gc_ens_push_host; 2 <= M, K <= 64, and a plain climatological
 * mean field is pushed twice.  The truth y and w [G], the node weights, are those of `h`.  All fields are [G, B, c_out]
 * float32.  A point is counted when y, all M members and all K samples are finite; every other point adds to `invalid`
 * and to nothing else.  Per counted point, in double from the float32 values, no fused multiply-add:
 *   m    = (sum_i x_i) / M,  cbar = (sum_j c_j) / K         ascending slot order (m is the m of gc_ens_score)
 *   fa = m - cbar,  oa = y - cbar
 *   ae_x = (sum_i |x_i - y|) / M,   ae_c = (sum_j |c_j - y|) / K
 *   d_x  = sum_{k=1}^{M-1} k (M - k) (x_(k+1) - x_(k)) / (M (M - 1) / 2)     over the members sorted ascending: the mean of
 *          |x_i - x_j| over the pairs, every term >= 0;   d_c the same over the sorted samples
 *   q_x  = (sum_i (x_i - cbar)^2) / M
 * Per column (b, c), over the counted nodes g, sums[b][c][0..11] in this order:
 *   A0 = sum w     A1 = sum w fa     A2 = sum w oa     A3 = sum w fa oa     A4 = sum w fa^2     A5 = sum w oa^2
 *   A6 = sum w q_x A7 = sum w (m - y)^2                F4 = sum w ae_x      F5 = sum w d_x
 *   C4 = sum w ae_c                  C5 = sum w d_c
 * counts[b][c] = counted points, invalid = points not counted.  Every partial sum has one writer and the order of addition
 * is fixed (no atomics on floats), so the same call twice returns identical bytes.  All outputs are raw and additive over
 * batches and dates; ACC = A3 / sqrt(A4 A5), CRPSS = 1 - (F4 - F5/2) / (C4 - C5/2) and the rest are formed on the host.
 *   truth: host [G, B, c_out], uploaded and kept, or NULL = the truth uploaded last (the buffer gc_ens_score uses).
 *   sums [B][c_out][12] is required; counts [B][c_out] and invalid [1] may be NULL.  Two launches on h's stream, ordered
 *   behind clim's stream by an event: a pass that reads the K samples and the M members of a point once each and sorts each
 *   in registers (the network of gc_ens_order_score), and a finish that adds the per-block partials in block order.
 *   Synchronous.
 *   GC_ERR_STATE: no gc_set_graph, no member store on either handle, a slot of either not pushed since its gc_ens_reserve
 *   (of clim's: "climatology member slot ..."), no node weights, no truth.
 *   GC_ERR_INVALID_ARGUMENT: clim NULL or == h, sums NULL, clim on another device or with another G, batch or c_out.
 * The call touches nothing of either handle but its own buffers and the shared truth buffer of h.  Counters (on h):
 * "ens_clim_calls", "ens_clim_device_us" (HIP-event time of the last call's launches), "ens_clim_invalid_points".
 */
int gc_ens_clim_score(gc_handle* h, gc_handle* clim, const float* truth /* NULL = the truth uploaded last */,
                      double* sums /* [B][c_out][12] */, uint64_t* counts /* [B][c_out], NULL allowed */,
                      uint64_t* invalid /* [1], NULL allowed */);

/*
 * The Extreme Forecast Index on the device (Lalaurette 2003, Zsoter 2006): at every point, how far
 * the M members of `h` are shifted against the K climatological samples in the store of `clim` (the second handle of
 * gc_ens_clim_score: same device, G, batch and c_out; 2 <= M, K <= 64), weighted towards the tails
 * (gencast-flax-nnx_amd/verification.py EfiScores).  The reference project has no verification code; the yardstick is the
 * definition below, restated in float64 in tests/efi_reference.py.  Per point, comparisons on the float32 values:
 *   le(v) = #{j : c_j <= v}     lt(v) = #{j : c_j < v}
 *   f = (sum_i (a[le(x_i)] + a[lt(x_i)])) / M        i ascending, in double: the EFI, in [-1, 1]
 *   o = a[le(y)] + a[lt(y)]                          the observed index: the same expression for the truth alone
 * `table` is a[0 .. K] = asin(2 n / K - 1) / pi, made on the host (verification.efi_table): this is the integral
 * (2 / pi) int_0^1 (p - F_f(p)) / sqrt(p (1 - p)) dp in closed form, ties counted half.  The device does comparisons, integer
 * counts, lookups, double additions in slot order and one division, so both fields (float32, rounded once) equal the
 * float64 reference byte for byte.  A point counts when y, all M members and all K samples are finite; elsewhere both
 * fields are NaN and the point adds to `invalid` alone.  Per column (b, c), over the counted nodes, w [G] the node weights:
 *   sums[b][c][0..5] = sum w, sum w f, sum w o, sum w f o, sum w f^2, sum w o^2        (f in double, before rounding)
 * in double, every sum in one fixed order (no atomics on floats): the same call twice returns identical bytes.  For event
 * t < T of the truth -- direction > 0: lt(y) >= rank_t, direction < 0: le(y) <= rank_t -- and the EFI bin
 * e = min(E - 1, (int)((f + 1) E / 2)):
 *   weighted[t][b][c][o_t][e] += wq[g]      counts[t][b][c][o_t][e] += 1              (wq: the integer weights of gc_ens_event_set)
 * integers, compared with ==.  Everything is raw and additive over batches and dates; mean EFI, the correlation of f and o
 * and the ROC of the index against the event are formed on the host.
 *   gc_ens_efi_set       the events and the bins.  Needs gc_set_graph only; survives gc_ens_reserve; replaces an earlier
 *                        setting; wq [G] may be NULL when n_events == 0.
 *                        GC_ERR_INVALID_ARGUMENT: n_events outside 0..4, n_bins outside 2..32, a direction of 0, a NULL array.
 *   gc_ens_efi_score     truth: host [G, B, c_out], uploaded and kept, or NULL = the truth uploaded last.  sums is required,
 *                        weighted where T > 0; counts (the shape of weighted) and invalid [1] may be NULL.  Three launches on
 *                        h's stream, ordered behind clim's stream by an event: the index pass (the K samples of a point
 *                        in registers, the M members streamed past them; fields, one 16-bit code per point, per-block
 *                        column sums), the ascending block finish, the table pass over the codes.  Synchronous.
 *   gc_ens_efi_fields    the EFI field alone: no truth, no weights and no gc_ens_efi_set needed, nothing returned.
 *   gc_ens_efi_download  field 0 (the EFI) or 1 (the observed index) of the last of the two calls on this store.
 *   GC_ERR_STATE: no gc_set_graph, no member store on either handle, a slot of either not pushed (of clim's: "climatology
 *   member slot ..."), no gc_ens_efi_set, no node weights, no truth; download: no fields of this store on the device
 *   (gc_ens_reserve and every call that rewrites the store forget them), or the observed index after gc_ens_efi_fields.
 *   GC_ERR_INVALID_ARGUMENT: clim NULL or == h, table or sums NULL, clim on another device or with another G, batch or
 *   c_out, a table that is not antisymmetric (a[K - n] == -a[n]) and non-decreasing, `which` outside 0..1.
 * Counters (on h): "ens_efi_calls", "ens_efi_device_us" (HIP-event time of the last call's launches),
 * "ens_efi_invalid_points" (of the last gc_ens_efi_score).
 */
int gc_ens_efi_set(gc_handle* h, int32_t n_events /* T, 0..4 */, const int32_t* rank /* [T] */, const int32_t* direction /* [T] */,
                   int32_t n_bins /* E, 2..32 */, const uint32_t* wq /* [G]; NULL allowed when T == 0 */);
int gc_ens_efi_score(gc_handle* h, gc_handle* clim, const double* table /* [K + 1] */,
                     const float* truth /* NULL = the truth uploaded last */, double* sums /* [B][c_out][6] */,
                     uint64_t* weighted /* [T][B][c_out][2][E] */, uint64_t* counts /* as weighted, NULL allowed */,
                     uint64_t* invalid /* [1], NULL allowed */);
int gc_ens_efi_fields(gc_handle* h, gc_handle* clim, const double* table /* [K + 1] */);
int gc_ens_efi_download(gc_handle* h, int32_t which /* 0 EFI, 1 observed index */, float* field /* [G,B,c_out] */);

/*
 * Score maps on the device: every unit above ends in a table per batch member and channel; this one
 * says WHERE the forecast is good.  The marginal scores of gc_ens_score are kept per grid point and added up over dates on
 * the device, one set of planes per slot (a slot is a lead time).  The reference project has no verification code; the
 * yardstick is the definition below, restated in tests/map_reference.py.
 * Store, truth and validity are those of gc_ens_score: members x_0 .. x_{M-1} and truth y are [G, B, c_out] float32; a point
 * counts when y and all M members are finite there.  No node weight is read.  The plan selects C' channels (ascending,
 * distinct; NULL = all), L slots and T event thresholds.
 * Per counted point, in double from the float32 values, each operation rounded once and nothing contracted:
 *   m  = (sum_i x_i) / M                                i ascending (slot order)
 *   s2 = (sum_i (x_i - m) (x_i - m)) / (M - 1)          the same order
 *   e  = m - y
 *   with the members sorted ascending x_(0) <= .. <= x_(M-1):
 *   ae = (sum_k |x_(k) - y|) / M                        k ascending
 *   d  = (sum_{k=1}^{M-1} (double)(k (M - k)) (x_(k) - x_(k-1))) / (M (M - 1) / 2)     k ascending; no term cancels
 *   c  = ae - 0.5 d                                     the fair CRPS of the point
 *   r  = #{i : x_i < y}                                 a member equal to y is not below it
 * The planes of a slot, per point (g, b, c'); dates add in call order, so a plane is the left fold of the per-date doubles:
 *   sums   [6]: P0 += e   P1 += e e   P2 += s2   P3 += ae   P4 += d   P5 += c c          (double)
 *   counts [3]: N0 += 1   N1 += [r == 0]   N2 += [r == M]                                 (uint32)
 * A point that does not count on a date adds nothing to any plane.  Event planes, from the byte per point and threshold
 * that gc_ens_event_score leaves (code = k | o << 7, 255 = not counted), uint32:
 *   events [T][5]: E0 += 1   E1 += k   E2 += k k   E3 += k o   E4 += o
 * Every point has one owner thread: no partials, no finish pass, no atomics; the planes equal the definition byte for byte.
 * Scores are formed on the host from the planes (bias = P0 / N0, fair crps = (P3 - P4 / 2) / N0,
 * brier = (E2 / M^2 - 2 E3 / M + E4) / E0 ...); the planes add over dates and merge over runs, scores do not.
 *   gc_ens_map_set                the plan; allocates and zeroes [L][6 + 3 + 5 T] planes of G B C' values.  A repeated call
 *                                 replaces and zeroes ("device_allocations" stays flat).  The planes are not sized by M and
 *                                 survive gc_ens_reserve; released by gc_destroy.  GC_ERR_UNSUPPORTED: n_slots outside
 *                                 1..128, n_event_thresholds outside 0..8.  GC_ERR_INVALID_ARGUMENT: n_channels outside
 *                                 1..c_out, a channel outside [0, c_out), channels not ascending or repeated.
 *   gc_ens_map_accumulate         adds the date in the store into `slot`.  Synchronous.  A slot remembers the M of its first
 *                                 date.  Faults, in this order: no graph; no plan; slot outside [0, L)
 *                                 (GC_ERR_INVALID_ARGUMENT); no member store; a member slot not pushed; no truth; another M
 *                                 than the slot holds ("reset the slot first").  All but the slot are GC_ERR_STATE.
 *   gc_ens_map_accumulate_events  adds the codes of the last gc_ens_event_score into `slot`.  Faults, in this order: no
 *                                 graph; no plan; a plan without event planes; slot outside [0, L); no member store; the T
 *                                 of gc_ens_event_set differs from the plan's; no event score since gc_ens_event_set /
 *                                 gc_ens_reserve / the last rewrite of the store; another M than the slot holds.
 *   gc_ens_map_download           the planes of one slot and the number of field / event calls added into it.
 *                                 GC_ERR_INVALID_ARGUMENT: a bad slot, sums or counts NULL, events given for a plan with T = 0.
 *   gc_ens_map_reset              zeroes a slot (-1: every slot) and forgets its M and its dates.
 * All five need gc_set_graph only; download and reset report no graph, no plan, the slot, in that order.  None of them
 * touches the member store, the truth (beyond storing the one passed), the mean / variance, quantile, EFI or code fields,
 * the conditioning, the last sample or the captured graphs.
 * Counters: "ens_map_calls", "ens_map_device_us" (HIP-event time of the last accumulate), "ens_map_invalid_points" (selected
 * points the last gc_ens_map_accumulate skipped), "ens_map_blocks" (grid.x of the last pass: one point per thread up to
 * 1024 workgroups, which then stride), "ens_map_bytes" (the accumulator bytes of the plan).
 */
int gc_ens_map_set(gc_handle* h, int32_t n_channels, const int32_t* channel /* [C'] or NULL = all */,
                   int32_t n_slots /* 1..128 */, int32_t n_event_thresholds /* 0..8, 0 = no event planes */);
int gc_ens_map_accumulate(gc_handle* h, int32_t slot, const float* truth /* NULL = the truth uploaded last */);
int gc_ens_map_accumulate_events(gc_handle* h, int32_t slot);   /* the codes of the last gc_ens_event_score */
int gc_ens_map_download(gc_handle* h, int32_t slot, double* sums /* [6][G][B][C'] */, uint32_t* counts /* [3][G][B][C'] */,
                        uint32_t* events /* [T][5][G][B][C'], NULL allowed */, int64_t* dates /* [2]: field / event calls, NULL allowed */);
int gc_ens_map_reset(gc_handle* h, int32_t slot /* -1 = every slot */);

/*
 * Time-window ensemble fields on the device: accumulations, means, changes and extremes over the
 * last L lead times of a rollout -- 24 h precipitation from 12 h steps, a weekly mean, the highest wind speed within three
 * days -- formed from the members and the truths that one handle's gc_ens_* store held at those lead times and left in the
 * member store of a SECOND handle, on which every scorer of this library then works as it is.  The reference project has
 * no verification code; the yardstick is the definition below, restated in tests/window_reference.py, bit for bit.
 * Source handle `src`: a complete store of M members and a truth, each [G, B, c] float32 -- a handle that samples, or the
 * destination of gc_ens_derive.  Window handle `win`: the same device, G and batch, c_out == c; it needs gc_set_graph only.
 * It owns a RING of the last L pushes; a push is a copy of src's M members and truth as they stand.
 * Plan: kind in {LINEAR 0, MAX 1, MIN 2}, 1 <= L <= 64 and, for LINEAR, coefficients a[0 .. L-1], finite doubles.  With
 * x_t, t = 0 (oldest) .. L - 1 (newest), the float32 values of one element of one field over the last L pushes, for every
 * element of each of the M + 1 fields (the truth is field M):
 *   any x_t not finite (NaN, +-inf) gives NaN, for every kind and also where a_t == 0
 *   LINEAR     acc = 0.0, then for t ascending acc = acc + a_t (double) x_t: the product is rounded, then the sum (no fused
 *              multiply-add); the output is (float) acc, rounded once -- a finite double beyond float32 range becomes +-inf
 *   MAX / MIN  m = x_0, then for t ascending m = x_t where x_t > m (MIN: x_t < m): exact, one of the inputs' bits, the
 *              older one on a tie (so also between +0 and -0)
 *   gc_ens_window_set    the plan.  coef [L] doubles, oldest first (NULL unless LINEAR).  Needs gc_set_graph only.  A new
 *                        plan clears the push count; the ring is freed and made again only by the push that finds L or M
 *                        changed ("device_allocations" stays flat).  GC_ERR_STATE: no graph.  GC_ERR_INVALID_ARGUMENT:
 *                        length < 1, LINEAR with coef NULL, a coefficient that is not finite.  GC_ERR_UNSUPPORTED: an
 *                        unknown kind, length > 64.
 *   gc_ens_window_push   src's M members and truth, device to device, into ring slot pushes % L; then pushes += 1.  truth:
 *                        host [G, B, c], uploaded into and kept in src's truth buffer as gc_ens_score(src, truth, ...)
 *                        would, or NULL = src's last truth.  The copies run on win's stream, ordered behind src's stream
 *                        by an event.  Synchronous: after the call src's store may be overwritten without changing the ring.
 *                        GC_ERR_INVALID_ARGUMENT: src is NULL, win itself or on another device; src has no graph, another
 *                        G, batch or c_out.  GC_ERR_STATE: no plan, no store on src, a src slot not pushed since its
 *                        gc_ens_reserve, no truth, an M other than the ring's while pushes > 0 (gc_ens_window_reset first).
 *   gc_ens_window_emit   pushes - L .. pushes - 1, in that order, reduced into every slot of win's member store and into
 *                        win's truth buffer: afterwards every slot counts as pushed and truth = NULL works in every scorer
 *                        of win; win's event codes, mean / variance fields and order results count as not computed.  One
 *                        launch.  Synchronous.  The ring is unchanged: an emit after every push gives sliding windows.
 *                        GC_ERR_STATE: no plan, pushes < L, no store on win, a store whose M differs from the ring's.
 *   gc_ens_window_reset  pushes = 0; the plan and the ring's memory stay.
 * No atomics: the same emit twice returns identical bytes.  The calls touch nothing on src but its truth buffer, and on win
 * only the ring, the member store and the truth.  Counters (on win): "ens_window_pushes" (pushes since the last set / reset),
 * "ens_window_emits" (emits so far), "ens_window_device_us" (HIP-event time of the last emit's launch),
 * "ens_window_ring_bytes" (the ring as it stands: L slots of (M + 1) fields, each slot padded to 16 bytes).
 */
int gc_ens_window_set(gc_handle* win, int32_t kind, int32_t length, const double* coef /* [length], NULL unless LINEAR */);
int gc_ens_window_push(gc_handle* win, gc_handle* src, const float* truth /* [G,B,c] host, NULL = src's last truth */);
int gc_ens_window_emit(gc_handle* win);
int gc_ens_window_reset(gc_handle* win);

/*
 * Multivariate ensemble scores on the device: the raw sums of the energy score over groups of
 * channels and whole fields, and of the variogram score over pairs of grid points a fixed offset apart
 * (gencast-flax-nnx_amd/verification.py EnergyScores, VariogramScores).  Every other score of this library is marginal: it
 * looks at one point and one channel at a time.  The reference project has no verification code; the yardstick is the
 * definition below, restated in float64 in tests/multivar_reference.py.
 * Members x_0 .. x_{M-1} and the truth y are [G, B, c_out] float32, w[g] the node weight of gc_ens_set_node_weight.  A
 * point (g, b, c) is valid iff y and all M members are finite there.  Write x_M = y.
 * Energy.  The plan gives K groups (1 <= K <= 32) and a per-channel scale: group[c] in {-1, 0 .. K-1}, where -1 means
 * the channel is in no group; every group is non-empty; a[c] is finite and > 0 for grouped channels.  Per batch member b,
 * group k and pair 0 <= i < j <= M, with pair index p = j (j - 1) / 2 + i and P = M (M + 1) / 2:
 *   D2[b][k][p] = sum omega (d d) over the valid points of the group
 *                 omega = (double)w[g] a[c];  d = (double)x_i - (double)x_j, which is exact; each product and each addition
 *                 is a rounded double operation with no contraction
 *   S0[b][k]    = sum omega over the same points         invalid = the number of skipped points of grouped channels
 * Invalid points are skipped, not multiplied by zero.  On the host D[i][j] = sqrt(D2 / S0), err = mean_i D[i][M],
 * pair = mean_{i<j<M} D[i][j], fair ES = err - pair / 2, ensemble ES = err - (M - 1) / M pair / 2 -- the pairing of the
 * fair and ensemble CRPS of gc_ens_score.  A group with S0 = 0 gives NaN.  ES is not additive in the raw sums: a result
 * keeps err and pair per forecast.  Units are the store's own; a[c] carries level or variable weights.
 * Variogram.  The plan gives the grid n_lat n_lon = G with node = i n_lon + j (as in gc_ens_derive_set), O offsets (di, dj)
 * with 1 <= O <= 16, not (0, 0), |di| < n_lat, |dj| < n_lon, and an order p in {0.5, 1, 2}: formed with sqrt, identity and
 * a product, no pow.  The partner of (i, j) is (i + di, (j + dj) mod n_lon).  The pair is skipped when i + di leaves
 * [0, n_lat), and when either end is invalid.  Per valid pair, in double:
 *   omega = (w[g] + w[g']) / 2      v(u) = |u_g - u_g'|^p      vx = (sum_i v(x_i)) / M in ascending slot order      vy = v(y)
 * Per (b, c, o):  V0 = sum omega,  V1 = sum omega (vy - vx)^2,  V2 = sum omega vx,  V3 = sum omega vy, and a uint64 pair
 * count.  These sums are additive; variogram score = V1 / V0, roughness ratio = V2 / V3 on the host.
 *   gc_ens_energy_set       the plan: group [c_out], scale [c_out].  Needs gc_set_graph only; survives gc_ens_reserve;
 *                           replaces an earlier plan ("device_allocations" stays flat); released by gc_destroy.
 *                           GC_ERR_UNSUPPORTED: K outside 1..32.  GC_ERR_INVALID_ARGUMENT: a NULL array, a group index
 *                           outside -1 .. K - 1, an empty group, a scale of a grouped channel that is not finite and > 0.
 *   gc_ens_energy_score     truth: host [G, B, c_out], uploaded and kept, or NULL = the truth uploaded last (the buffer
 *                           gc_ens_score uses).  d2 [B][K][P] and s0 [B][K] are required, invalid [1] may be NULL.  Two
 *                           launches: a pass in which a workgroup takes one (b, k) and a node range, stages tiles of 256
 *                           points of the M + 1 fields in LDS and keeps the P pair sums in registers, spread over its
 *                           threads; and a finish that adds the per-block partials in block order.  Synchronous.
 *   gc_ens_variogram_set    the plan.  Needs gc_set_graph only; survives gc_ens_reserve; replaces an earlier plan
 *                           ("device_allocations" stays flat).  GC_ERR_UNSUPPORTED: O outside 1..16, p not 0.5, 1 or 2.
 *                           GC_ERR_INVALID_ARGUMENT: offsets NULL, n_lat n_lon != G, an offset (0, 0) or beyond the grid.
 *   gc_ens_variogram_score  sums [4][B][c_out][O] (V0 .. V3) is required, counts [B][c_out][O] may be NULL.  Two launches:
 *                           a pass with one thread per column of a node lane and one offset per workgroup, and the
 *                           finish.  Synchronous.
 * Both scoring entries: GC_ERR_STATE for no plan, no member store, a slot not pushed since gc_ens_reserve, no node weights,
 * no truth; GC_ERR_INVALID_ARGUMENT for a required array that is NULL.  No atomics on floats and a fixed order of every
 * sum: the same call twice returns identical bytes.  Nothing else on the handle is touched.  Counters: "ens_energy_calls",
 * "ens_energy_device_us" (HIP-event time of the last call's launches), "ens_energy_invalid_points" (of the last call),
 * "ens_variogram_calls", "ens_variogram_device_us".
 */
int gc_ens_energy_set(gc_handle* h, int32_t n_groups, const int32_t* group /* [c_out] */, const double* scale /* [c_out] */);
int gc_ens_energy_score(gc_handle* h, const float* truth /* NULL = the truth uploaded last */, double* d2 /* [B][K][P] */,
                        double* s0 /* [B][K] */, uint64_t* invalid /* [1], NULL allowed */);
int gc_ens_variogram_set(gc_handle* h, int32_t n_lat, int32_t n_lon, int32_t n_offsets, const int32_t* offsets /* [O][2] */,
                         double p);
int gc_ens_variogram_score(gc_handle* h, const float* truth /* NULL = the truth uploaded last */,
                           double* sums /* [4][B][c_out][O] */, uint64_t* counts /* [B][c_out][O], NULL allowed */);

/*
 * Threshold-weighted CRPS on the device: how good the forecast distribution of the gc_ens_* store is
 * in one tail (Gneiting & Ranjan 2011), in the chaining form of Allen et al. (2023): for the weight 1{z >= t} the twCRPS is
 * the plain CRPS of the clamped values max(z, t), for 1{z <= t} of min(z, t).  Clamping keeps the order of the members, so a
 * point is sorted once and every threshold costs O(M) (gencast-flax-nnx_amd/verification.py TailScores).  The reference
 * project has no verification code; the yardstick is the definition below, restated in float64 in tests/tail_reference.py.
 * Members x_0..x_{M-1} (2 <= M <= 64) and truth y are [G,B,c_out] float32 in the sample layout.  w[g] are the float node
 * weights of gc_ens_set_node_weight.  There are T threshold fields thr_t (1 <= T <= 8), each [G,B,c_out] float32, with a
 * direction dir_t != 0.  This is the convention of gc_ens_event_set.
 * A point counts for threshold t when y, all M members and thr_t are finite there.  A NaN threshold means "not evaluated"
 * for that t only.
 * Per counted point, with x_(0) <= ... <= x_(M-1) the members in ascending order:
 *   v(z) = fmaxf(z, thr_t) when dir_t > 0.  This is the upper tail, weight 1{z >= thr}.
 *   v(z) = fminf(z, thr_t) when dir_t < 0.  Both are exact in float32.
 *   u_k = v(x_(k)), which is still ascending.
 *   AE = sum_{k=0}^{M-1} |(double)u_k - (double)v(y)|, added in ascending k.  ae = AE / M.
 *   PD = sum_{k=1}^{M-1} (double)(k (M-k)) ((double)u_k - (double)u_{k-1}), added in ascending k.  d = PD / (M(M-1)/2).
 *     This "gap form" equals sum_{i<j} |u_i - u_j|.  Every term is non-negative, so there is no cancellation.
 *   o = [y in the event], strict as in section 8f: y > thr_t for dir_t > 0, y < thr_t for dir_t < 0.
 * Every operation is a rounded double operation with no contraction.
 * Per (t, b, c), over the counted nodes:
 *   sums[t][b][c][0..3] = sum w, sum w ae, sum w d, sum w o
 *   counts[t][b][c] = counted points (uint64)
 *   invalid[t] = points skipped
 * All of these are raw and additive over batches and dates.  On the host, with S0..S3 the four sums: fair twCRPS =
 * (S1 - S2/2)/S0, ensemble twCRPS = (S1 - (M-1)/M S2/2)/S0 (the pairing of gc_ens_score's sums 4 and 5: d is the same Gini
 * mean difference), base rate = S3/S0.
 *   gc_ens_tail_set    the threshold fields and directions.  Needs gc_set_graph only; buffers of its own, independent of
 *                      gc_ens_event_set (both may be set, with different T); survives gc_ens_reserve; a repeated call
 *                      replaces ("device_allocations" stays flat); released by gc_destroy.  GC_ERR_UNSUPPORTED: T outside
 *                      1..8.  GC_ERR_INVALID_ARGUMENT: a zero direction or a null pointer.  GC_ERR_STATE: before gc_set_graph.
 *   gc_ens_tail_score  truth: host [G, B, c_out], uploaded and kept, or NULL = the truth uploaded last (the buffer
 *                      gc_ens_score uses).  sums is required, counts and invalid may be NULL.  Two launches: a pass that
 *                      reads the M members of a point once, sorts them in registers and walks the T thresholds, and a
 *                      finish that adds the per-block partials in block order.  Synchronous.  GC_ERR_STATE: no thresholds,
 *                      no member store, a slot not pushed since gc_ens_reserve, no node weights, no truth.
 * No atomics on floats and a fixed order of every sum: the same call twice returns identical bytes.  Nothing else on the
 * handle is touched.  Counters: "ens_tail_calls", "ens_tail_device_us" (HIP-event time of the last call's launches),
 * "ens_tail_invalid_points" (of the last call, over all thresholds).
 */
int gc_ens_tail_set(gc_handle* h, int32_t n_thresholds, const float* thresholds /* [T][G,B,c_out] */,
                    const int32_t* direction /* [T] */);
int gc_ens_tail_score(gc_handle* h, const float* truth /* NULL = the truth uploaded last */,
                      double* sums /* [T][B][c_out][4] */, uint64_t* counts /* [T][B][c_out], NULL allowed */,
                      uint64_t* invalid /* [T], NULL allowed */);

/*
 * Regional ensemble scores on the device: the sums of gc_ens_score for R regions of grid nodes --
 * tropics, extratropics, land, sea, boxes -- from ONE scoring pass over the nodes that belong to any region
 * (gencast-flax-nnx_amd/verification.py RegionSpec, RegionScores).  The reference project has no verification code; the
 * yardstick is tests/verification_reference.py on each region's node subset (tests/region_reference.py).
 * node_bits[g] is a uint32 per grid node: bit r set = node g belongs to region r (r < R <= 32).  Regions may overlap.  A node
 * with node_bits == 0 belongs to nothing: it is not read, and it is counted in no invalid[r].  A region without a node is
 * legal: its sums and counts are zero.
 * Per region r, over the nodes with bit r set and with the node weights of gc_ens_set_node_weight, sums S0..S5, the rank
 * histogram and the skipped points are exactly those of gc_ens_score (section 8c): the validity rule (y and all M members
 * finite), the tie rule (a member equal to y is not below it), the ascending slot order of the mean, the second pass for s2
 * and rounded double operations without contraction carry over.
 *   gc_ens_region_set    builds the plan on the host.  An ATOM is a distinct non-zero value of node_bits; the listed nodes
 *                        are grouped by atom (ascending atom value, ascending node index inside an atom) and cut into node
 *                        ranges that each lie inside one atom: an atom of n_a nodes gets ceil(n_a / per) workgroups, per as
 *                        gc_ens_score would cut the listed nodes.  Needs gc_set_graph only; survives gc_ens_reserve and every
 *                        score; a repeated call replaces ("device_allocations" stays flat); released by gc_destroy.
 *                        GC_ERR_UNSUPPORTED: R outside 1..32, or more than 256 atoms (the previous plan stays in force).
 *                        GC_ERR_INVALID_ARGUMENT: a null pointer, or a bit at or above R.  GC_ERR_STATE: before gc_set_graph.
 *   gc_ens_region_score  truth: host [G, B, c_out], uploaded and kept, or NULL = the truth uploaded last (the buffer
 *                        gc_ens_score uses).  sums is required, hist and invalid may be NULL.  Two launches: the pass of
 *                        gc_ens_score over the listed nodes, whose per-workgroup partials belong to one atom each, and a
 *                        finish over (column tile, region) that adds the partials of the atoms with bit r in ascending
 *                        workgroup order.  The cost is one scoring pass over the listed nodes, whatever R is.  Synchronous.
 *                        GC_ERR_STATE: no plan, no member store, a slot not pushed since gc_ens_reserve, no node weights,
 *                        no truth.
 * No atomics on floats and a fixed order of every sum: the same call twice returns identical bytes.  Nothing else on the
 * handle is touched.  Counters: "ens_region_calls", "ens_region_device_us" (HIP-event time of the last call's launches),
 * "ens_region_invalid_points" (of the last call, summed over the regions).
 */
int gc_ens_region_set(gc_handle* h, int32_t n_regions /* R, 1..32 */,
                      const uint32_t* node_bits /* [G]: bit r set = node g belongs to region r */);
int gc_ens_region_score(gc_handle* h, const float* truth /* NULL = the truth uploaded last */,
                        double* sums /* [R][6][B][c_out] */, uint64_t* hist /* [R][B][c_out][M + 1], NULL allowed */,
                        uint64_t* invalid /* [R], NULL allowed */);

/*
 * Ensemble feature detection on the device: where each member, and the truth, puts a weather
 * system.  Per field of the store of a source handle `src` and per detector d < D, the CENTRES -- local extrema of one
 * source channel that pass a threshold and a ring (depth) test -- as a sparse list, and as a dense 0 / 1 STRIKE field in
 * the store of the destination handle `dst` (c_out == D, the same device, G and batch; it needs gc_set_graph only), which
 * every scorer of the library reads as it is: its ensemble mean is the strike-probability map.  The reference project
 * has no tracker; the yardstick is the definition below, restated in tests/feature_reference.py.
 * Per field z (a member, or the truth), batch entry b and detector d, on the grid node = lat_i n_lon + lon_j:
 *   signed value  x = the source value at channel[d]; s = x for direction[d] < 0 (a minimum), s = -x for direction[d] > 0
 *   window        window(n; r_lat, r_lon) = Win(i, j) of gc_ens_derive_set: rows |i' - i| <= r_lat clipped at the poles,
 *                 circular |j' - j| <= r_lon[i'] in row i'
 *   extremum      s[n] is finite, and for every other n' of window(n; r_lat[d], r_lon[d]) with finite s[n']: s[n] < s[n'],
 *                 or s[n] == s[n'] and n < n' (IEEE comparison: -0.0 == +0.0); non-finite neighbours are skipped
 *   threshold     where use_threshold[d]: s[n] <= t, t = threshold[d] for a minimum, -threshold[d] for a maximum
 *   ring          where ring_lat[d] > 0: the boundary of window(n; ring_lat[d], ring_lon[d]) -- the rows i +- ring_lat that
 *                 exist over all |t| <= ring_lon[i'], and in every row strictly between them the two nodes t = +-ring_lon[i'] --
 *                 holds a finite value and (double) min_finite_ring(s) - (double) s[n] >= depth[d] (one double subtraction)
 *   centre        an extremum that passes the tests that are enabled
 *   list          the centres in ascending node index; count is their true number, the first max_centres are kept (node,
 *                 and value = x, the same bits); entries past the last centre read node -1, value 0
 *   strike field  dst channel d at node n: 1.0f if any centre (listed or not) lies in window(n; strike_lat[d],
 *                 strike_lon[d]), else 0.0f; NaN where the source value at n is not finite
 *   gc_ens_feature_set      the plan on dst.  D must equal dst's c_out, 1 <= D <= 8; max_centres in 1..1024; thresholds and
 *                           depths in the members' units.  Needs gc_set_graph only; through pinned staging; replaces an
 *                           earlier plan ("device_allocations" stays flat), survives gc_ens_reserve, released by gc_destroy.
 *                           GC_ERR_STATE: no graph.  GC_ERR_INVALID_ARGUMENT: a null pointer, c_src < 1, D, n_lat n_lon != G,
 *                           max_centres, a channel outside [0, c_src), direction 0, a threshold in use or a depth of a ring
 *                           in use that is not finite, a negative r_lat / ring_lat / strike_lat, a *_lon outside
 *                           0 .. (n_lon - 1) / 2.  GC_ERR_UNSUPPORTED: a row that does not fit the 64 KB of LDS of the row
 *                           pass (n_lon > 4096).
 *   gc_ens_feature          every slot of dst's store becomes the member's strike fields and counts as pushed, dst's truth
 *                           buffer the truth's; dst's event codes, mean / variance fields and order statistics count as
 *                           not computed.  truth, the stream order and every error as gc_ens_derive.  Synchronous.
 *   gc_ens_feature_centres  the lists of the last gc_ens_feature, field M = the truth.  GC_ERR_STATE: no call since the
 *                           plan was set.
 * Launches per chunk of at most 8 of the M + 1 fields: a gather of the detection channel into dense 64-bit keys (value
 * order above node index), a row pass (window minimum along the longitude in LDS), a column pass (extremum, threshold, ring,
 * strike rectangles) and a list pass.  Integer comparisons and one double subtraction, no float atomics: the same call
 * twice returns identical bytes.  Nothing else on either handle is touched.  Counters: "ens_feature_calls",
 * "ens_feature_device_us" (HIP-event time of the last call's launches).
 */
int gc_ens_feature_set(gc_handle* dst, int32_t c_src, int32_t D, const int32_t* channel /* [D] */,
                       const int32_t* direction /* [D] < 0 minimum, > 0 maximum */, const int32_t* use_threshold /* [D] */,
                       const float* threshold /* [D] */, int32_t n_lat, int32_t n_lon, const int32_t* r_lat /* [D] */,
                       const int32_t* r_lon /* [D][n_lat] */, const int32_t* ring_lat /* [D], 0 = no ring test */,
                       const int32_t* ring_lon /* [D][n_lat] */, const double* depth /* [D] */,
                       const int32_t* strike_lat /* [D] */, const int32_t* strike_lon /* [D][n_lat] */, int32_t max_centres);
int gc_ens_feature(gc_handle* dst, gc_handle* src, const float* truth /* [G,B,c_src] host, NULL = src's last truth */);
int gc_ens_feature_centres(gc_handle* dst, int32_t* count /* [M + 1][B][D] */, int32_t* node /* [M + 1][B][D][max_centres] */,
                           float* value /* [M + 1][B][D][max_centres] */);

/*
 * Fractions skill score on the device: every event score above is point-wise, so a sharp forecast that
 * puts a maximum two grid points beside the analysis is punished twice.  The fractions skill score (Roberts & Lean 2008) of
 * the neighbourhood ensemble probability (Schwartz et al. 2010) compares the fraction of a neighbourhood in the event,
 * forecast against observed, at up to 8 neighbourhood sizes from one pass over the code bytes gc_ens_event_score left on the
 * device.  The reference project has no verification code; the yardstick is the definition below, restated in
 * tests/fss_reference.py.
 * Inputs, on a handle whose last gc_ens_event_score is still valid: the codes code_t [G, B, c_out] for t < T, the member
 * count M they were made with, the node weights wq [G] of gc_ens_event_set.  A point counts iff code != 255; there
 * k = code & 127 and o = code >> 7.  The plan: S scales (1 <= S <= 8), the grid n_lat n_lon = G (node = lat_i n_lon + lon_j),
 * per scale r_lat[s] >= 0 and r_lon[s][i] in 0 .. (n_lon - 1) / 2, integer row weights 1 <= row_wq[i] <= 2^24 - 1.  Win_s(i, j)
 * is the window of gc_ens_derive: latitude clipped, longitude wrapping, the width of a row that of the row i'.
 * Per counted centre p = (i, j), over the counted q in Win_s(p), in integers:
 *   A = sum row_wq[i'] k(q),   B = sum row_wq[i'] o(q),   N = sum row_wq[i']       (below 2^51 for G <= 2^21, M <= 64)
 * then in double, each operation rounded once and nothing contracted:
 *   P = (double) A / ((double) M (double) N),   O = (double) B / (double) N        (N >= row_wq[i] >= 1)
 * Per (t, s, b, c) four double sums over the counted centres, w = (double) wq[g]:
 *   sums[0] = sum w ((P - O)(P - O)),  sums[1] = sum w (P P + O O),  sums[2] = sum w P,  sums[3] = sum w O
 * formed without float atomics and in a fixed order: two calls give the same bytes.  A column with no counted point gives
 * four zeros.  FSS = 1 - sums[0] / sums[1]; over several dates 1 - sum sums[0] / sum sums[1]: the sums add, scores do not.
 *   gc_ens_fss_set     the plan, through pinned staging (the caller's arrays are free on return).  Needs gc_set_graph only.
 *                      Replaces an earlier plan ("device_allocations" stays flat), survives gc_ens_reserve, released by
 *                      gc_destroy.  GC_ERR_STATE: no graph.  GC_ERR_UNSUPPORTED: S outside 1..8, n_lon > 16384.
 *                      GC_ERR_INVALID_ARGUMENT: a null pointer, n_lat n_lon != G, r_lat[s] < 0, an r_lon out of range, a
 *                      row_wq of 0 or above 2^24 - 1.
 *   gc_ens_fss_score   sums [T][S][B][c_out][4].  Per threshold and chunk of columns a row pass (prefix sums of one latitude
 *                      row in LDS, the row-window sums of every scale from that one prefix), a column pass with a block
 *                      reduction and a finish pass, over a handle-owned work buffer of at most max(256 MiB,
 *                      8 (S + 1) G tile) bytes.  Synchronous.
 *   gc_ens_fss_fields  for one (t, s): prob = (float) P and obs = (float) O, each [G, B, c_out], NaN where the point does
 *                      not count.  GC_ERR_INVALID_ARGUMENT: t outside [0, T), s outside [0, S), a null pointer.
 * Both: GC_ERR_STATE without a graph, a plan, or valid codes -- a gc_ens_event_set, gc_ens_reserve, gc_ens_derive,
 * gc_ens_window_emit or gc_ens_feature since the last gc_ens_event_score invalidates them.
 * None of these entries touches the sampler state, the member store, the codes, the event tables or the captured sample
 * graphs.  Counters: "ens_fss_calls" (scoring calls so far), "ens_fss_device_us" (HIP-event time of the last call's launches).
 */
int gc_ens_fss_set(gc_handle* h, int32_t n_scales, int32_t n_lat, int32_t n_lon, const int32_t* r_lat /* [S] */,
                   const int32_t* r_lon /* [S][n_lat] */, const uint32_t* row_wq /* [n_lat] */);
int gc_ens_fss_score(gc_handle* h, double* sums /* [T][S][B][c_out][4] */);
int gc_ens_fss_fields(gc_handle* h, int32_t threshold, int32_t scale, float* prob /* [G,B,c_out] */, float* obs /* [G,B,c_out] */);

/*
 * Ensemble exchange.  Replaces: the replication of inputs / forcings over the local
 * devices in chunked_prediction_generator_multiple_runs (common/rollout.py:41-75 `_replicate_dataset`,
 * :123-139 `device_put_sharded`); members then run independently, one per GPU (:312-322), and are
 * pulled back per device (:357-360 -> gc_download_sample on every rank).
 * One process (or thread) per GPU, each with its own handle.  The ONLY collective on the path is
 * the broadcast of the packed conditioning [G, B, c_in] from `root`, issued by the library itself:
 * ncclBroadcast (RCCL, over xGMI between the GPUs of a node) in place on the handle's resident
 * buffer and on the handle's stream, followed by the re-pack -- no host copy, no torch.  Nothing
 * inside the denoiser or the sampler communicates.
 *   gc_comm_unique_id      rank 0: a GC_COMM_ID_BYTES blob (ncclUniqueId); hand it to every rank by
 *                          any means (file, socket, environment)
 *   gc_comm_init           collective over all ranks: ncclCommInitRank on this handle's device
 *   gc_comm_broadcast_cond collective: root's resident conditioning (gc_upload_cond) -> every rank
 *   gc_comm_allreduce_max  collective: *value <- max over ranks (benchmark timing); also a barrier
 *   gc_comm_info           what RCCL itself says about this handle's communicator: ncclCommCount / ncclCommUserRank
 *                          (0 ranks, rank -1 without a communicator) -- lets a driver verify that the exchange it
 *                          reports really spans all its ranks
 * librccl.so.1 is loaded at the first gc_comm_* call (GC_RCCL_LIBRARY overrides the path); failures
 * return GC_ERR_COMM.
 */
#define GC_COMM_ID_BYTES 128
int gc_comm_unique_id(void* id_out /* [GC_COMM_ID_BYTES] */);
int gc_comm_init(gc_handle* h, const void* id, int32_t rank, int32_t world_size);
int gc_comm_info(gc_handle* h, int32_t* num_ranks, int32_t* rank);
int gc_comm_broadcast_cond(gc_handle* h, int32_t root);
int gc_comm_allreduce_max(gc_handle* h, double* value);
int gc_comm_destroy(gc_handle* h);

/*
 * Autoregressive context update on the device.
 * Replaces, for the packed conditioning: the context roll of autoregressive_rollout
 * (training/train_helpers.py:596-622: drop the oldest frame, append the predicted one, carry
 * input-only variables, take forcing variables from this step's forcings) together with
 * InputsAndResiduals' un-normalise + add-last-input and the re-normalisation of the next step
 * (common/normalization.py:100-121,200-238), which in normalised space is one affine per channel.
 * For every conditioning channel c of [G, B, c_in] (plan arrays have c_in entries):
 *   kind 0  keep       new[c] = old[c]
 *   kind 1  copy       new[c] = old[src[c]]
 *   kind 2  residual   new[c] = old[src[c]] + a[c] * sample[sidx[c]] + b[c]
 *   kind 3  forcing    new[c] = forcings[sidx[c]]          (row-wise, forcings is [G, B, n_forcing])
 *   kind 4  direct     new[c] = a[c] * sample[sidx[c]] + b[c]
 * `sample` is the last sample held by the handle (gc_sample_resident / gc_sample).
 * gc_rollout_advance applies the plan to all rows in one launch and re-packs the conditioning;
 * `forcings` is a HOST array (NULL allowed when the plan has no kind 3).
 */
int gc_rollout_plan(gc_handle* h, const int32_t* kind, const int32_t* src, const int32_t* sidx,
                    const float* a, const float* b, int32_t n_forcing);
int gc_rollout_advance(gc_handle* h, const float* forcings);
/* Copies the resident conditioning [G, B, c_in] back to the host (tests, checkpoints). */
int gc_download_cond(gc_handle* h, float* out);

/*
 * Measurement support (bench.py, rocprof cross-check).  Kernel classes are
 * indexed 0..gc_num_kernel_classes()-1; gc_kernel_class_name gives the label
 * that also prefixes the HIP kernel symbol.  With profiling enabled on a class,
 * every launch of that class is bracketed by HIP events on the handle's stream;
 * gc_profile_read synchronises and returns launches and total milliseconds.
 */
int         gc_num_kernel_classes(void);
const char* gc_kernel_class_name(int cls);
int gc_profile_enable(gc_handle* h, int cls /* -1 = off */);
/* Bracket only every `stride`-th launch of the profiled class (default 1) so that the event
 * records do not perturb a timed region. */
int gc_profile_set_stride(gc_handle* h, int stride);
int gc_profile_read(gc_handle* h, int32_t* launches, float* total_ms);
/* Algorithmic FLOPs and compulsory HBM bytes of ONE denoiser call for this
 * handle's configuration (formulas in DESIGN.md). */
int gc_algorithmic_work(gc_handle* h, double* flops, double* bytes);
/* Named counters: "range_fallbacks" (calls re-run on the f32 kernels by the f16x3 domain guard),
 * "static_embedding_fallbacks" (times the static embeddings -- made in gc_finalize and when "precision" or "features"
 * changes -- left the f16x3 domain and were made again on the f32 kernels; calls are not affected; not checked with
 * "features" = "f16", where an overflow to Inf is that mode's defined arithmetic),
 * "launches_per_call" (kernel launches of the last denoiser forward), "weights_f16_unsafe",
 * "graph_captures" / "graph_replays" (sampler graphs captured / samples launched as one hipGraphLaunch),
 * "fp16_storage" (1 when the last forward kept its activations as 2-byte fp16 arrays in HBM: features = f16 on the
 * f16x3 weight-streaming kernels; 0 when it ran on float32 containers), "split_edge" (1 when the edge MLPs run with their first layer split by input block: on
 * from latent 512), "attention_items" (work items of the last call's attention launches when they ran as a host-made item list -- one whole
 * query tile per CU, then the remaining tiles as key-range pieces merged by the out-projection: the 1-degree size, 512; 0: plain launch),
 * "m2g_fused_sum" (1 when the last forward added every grid node's three updated mesh2grid edges inside the edge MLP's epilogue --
 * jraph.segment_sum of common/typed_graph_net.py:175-182 without storing the edges; 0: edge update + a segment-sum launch, the form
 * any mesh2grid edge set with other in-degrees than 3 takes), "embed_cache" (samples so far whose grid embedding ran on the cached
 * per-sample-constant part of its first layer: only the c_out noisy-target columns are multiplied per call, the other 3 + c_in - c_out
 * once per sample -- dpm_solver_plus_plus_2s.py:107-112 closes over them; float32 node features, hidden_layers = 1),
 * "edge_term_samples" (samples so far whose edge MLPs read their first layer's edge block from the per-noise-level cache:
 * gc_set_option "edge_term_cache_mb"), "edge_term_cache_bytes" (device bytes that cache holds now; 0: not built),
 * "loss_evaluations" (denoising-loss evaluations so far: gc_loss_resident / gc_loss), "loss_device_us" (HIP-event time of
 * the evaluations of the last gc_loss_resident call, microseconds). */
/* Launch geometry of the last call of an ensemble unit (0 before its first call): "<prefix>_blocks" for the prefixes
 * ens_event, ens_derive, ens_band, ens_order, ens_clim, ens_efi, ens_energy, ens_variogram, ens_tail, ens_region,
 * ens_feature, ens_fss and ens_map, and "ens_score_blocks" for gc_ens_score -- the node-range workgroups (grid.x) of the call's main
 * pass.  Every pass caps that number (2048, 1024, 1024 / (thresholds x column tiles), 2048 / (batch x groups), 256 ...);
 * above the cap a workgroup walks more nodes and the trailing workgroups may have none, so the counter says which regime
 * a call ran in.  Where a call has two passes of different geometry it is the pass with a cap of its own:
 * gc_ens_efi_score with events reports its table pass, without events (and gc_ens_efi_fields) the index pass;
 * gc_ens_order_score the sorting pass, gc_ens_order_fields its field pass; gc_ens_derive the point pass, not the pooling
 * passes; gc_ens_fss_score the column pass; gc_ens_region_score the entries of the plan's block table; gc_ens_feature and
 * gc_ens_band, which have no node-range pass, the workgroups of their gather.  "ens_fss_chunks": the column chunks every
 * threshold of the last gc_ens_fss_score went through (the work buffer's byte budget or the 256-column limit cut them). */
/* ... and "device_allocations" (device buffers the handle holds now: gc_finalize and gc_set_noisy_slots replace theirs, they do not add),
 * "noise_stream" (the Philox stream the next drawn field will use: gc_noise_seed sets it, every initial-noise and churn field adds one). */
/* Poison mode, a debugging aid that is never timed: with GC_DEBUG_POISON=1 in the environment when gc_create runs, every
 * device buffer the handle allocates from then on is filled before anything else touches it -- bytes 0xFF where it holds
 * floating-point values (float, double, the fp16 K / V planes: every word a NaN), bytes 0x01 where it holds integers or
 * mixed work bytes (a stray count reads 16 843 009, a stray index stays small) -- and the pinned staging buffers are filled
 * with 0xFF on the host.  A result that depends on a word the library never wrote then differs from the result without
 * the switch.  "poison_allocs" (device buffers filled so far) and "poison_bytes" (their bytes) read 0 without the switch. */
int gc_get_counter(gc_handle* h, const char* name, int64_t* value);

#ifdef __cplusplus
}
#endif
#endif /* GENCAST_HIP_H_ */
