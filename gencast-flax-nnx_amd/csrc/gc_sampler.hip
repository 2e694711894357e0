// The sampler around the denoiser forward: the DPM-Solver++2S loop, its HIP-graph replay, the f16x3 domain guard,
// spherical noise fields and one evaluation of the denoising loss.
#include "gc_handle.h"

namespace gci {

// ---- f16x3 domain guard -------------------------------------------------------------------------
// Enqueues the finite check of `p` and the copy of the counter to pinned host memory.
int guard_enqueue(gc_handle* h, const float* p, size_t n) {
  if (!make_route(h).f16) return GC_OK;
  int rc = launch(h, gc::KC_PACK, [&] { return gc::launch_finite_check(h->stream, p, n, h->d_nonfinite); });
  if (rc) return rc;
  GC_HIP(h, hipMemcpyAsync(h->h_nonfinite, h->d_nonfinite, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
  return GC_OK;
}
// After the stream has been synchronised: did the check that guard_enqueue queued see NaN / Inf?
bool guard_tripped(gc_handle* h) {
  if (*h->h_nonfinite == h->nonfinite_seen) return false;
  h->nonfinite_seen = *h->h_nonfinite;
  return true;
}

// f32 scalar arithmetic of the preconditioning (dpm_solver_plus_plus_2s.py:181-205, sigma_data = 1)
float f_c_in(float s) { return 1.0f / std::sqrt(s * s + 1.0f); }
float f_c_out(float s) { return s / std::sqrt(s * s + 1.0f); }
float f_c_skip(float s) { return 1.0f / (s * s + 1.0f); }

// out = (base ? base : 0) + scale * (a fresh unit-variance spherical white-noise field [G, B, c_out])
int noise_field(gc_handle* h, const float* base, float scale, float* out) {
  if (h->nz_L == 0) return fail(h, GC_ERR_STATE, "gc_noise_set_tables has not been called");
  const int N = h->cfg.batch * h->cfg.c_out;
  const size_t ncoef = (size_t)2 * h->nz_L * h->nz_L * N;
  const unsigned long long stream = h->nz_stream++;
  int rc = launch(h, gc::KC_NOISE, [&] { return gc::launch_noise_normals(h->stream, h->d_nz_coef, ncoef, h->nz_key, stream); });
  if (rc) return rc;
  return launch(h, gc::KC_NOISE, [&] {
    return gc::launch_noise_synthesis(h->stream, h->d_nz_leg, h->d_nz_cos, h->d_nz_sin, h->d_nz_coef, h->d_nz_f,
                                      h->nz_L, h->nz_lat, h->nz_lon, N, base, scale, out);
  });
}

// Everything one sample enqueues on h->stream between the two timing events: kernel launches and one device-to-device
// copy, no allocation, no host synchronisation -- so it can run under stream capture (run_sampler).
int sampler_body(gc_handle* h, const float* sigmas, int n, int skip_dead, const std::vector<float>& call_sigma,
                 bool multi, int* calls_out) {
  const gc_config& c = h->cfg;
  const int rows = h->hg.G * c.batch;
  const size_t ne = (size_t)rows * c.c_out;
  hipStream_t s = h->stream;
  int rc, calls = 0;
  const size_t cond_call = (size_t)c.batch * h->cond_total;
  const bool churn = !h->churn_rates.empty();
  // The kernel that produces a state also writes it, times the next call's c_in, into the noisy-target slots of the
  // packed grid input (one launch per denoiser call less); with stochastic churn in front of a call the state changes
  // once more first, and the write stays a launch of its own.
  // The per-sample-constant part of the grid embedding's first layer, once per sample (gc_handle::embed_cache): the
  // noisy columns of the packed input are cleared (their weights are zero in w1st, but 0 x NaN is NaN), then
  // P = xp @ W1_static (the LDS-staged GEMM: K = kp is a multiple of 32, not of 128; float32 out, no bias -- the
  // MLP adds b1 itself).  From here on the sampler writes the noisy channels into the compact array d_xn.
  h->embed_cache_live = true;
  struct CacheOff { gc_handle* h; ~CacheOff() { h->embed_cache_live = false; } } cache_off{h};   // gc_denoise keeps the full form
  const Route route = make_route(h);
  const bool cache = route.embed_cache;
  if (cache) {
    if ((rc = launch(h, gc::KC_PACK, [&] { return gc::launch_zero_slots(s, h->d_slots, rows, c.c_out, h->kp, h->d_xp); }))) return rc;
    gc::GemmArgs ga{};
    ga.a = h->d_xp; ga.lda = h->kp; ga.a_f32 = 1; ga.ldw = h->kp; ga.rows = rows; ga.n = c.latent_size; ga.k_slice = h->kp;
    ga.bias = nullptr; ga.act = 0; ga.out = h->d_pstat; ga.ldo = c.latent_size; ga.round16 = 0; ga.out_f32 = 1;
    ga.wt = route.f16 ? h->w1st_s : h->w1st_t;
    if ((rc = launch(h, gc::KC_GEMM_NODE, [&] { return gc::launch_gemm(s, gc::KC_GEMM_NODE, ga, 1, 0, route.f16); }))) return rc;
    ++h->embed_cache_samples;
  }
  // edge terms: every call reads the slot of its noise level (run_sampler made the cache hold this sample's list)
  if (route.edge_terms) {
    if (!multi || h->terms.call_slot.size() != call_sigma.size() ||
        std::memcmp(h->terms.sigmas.data(), call_sigma.data(), call_sigma.size() * sizeof(float)))
      return fail(h, GC_ERR_INTERNAL, "sampler: the edge-term cache was built for another noise-level list");
    ++h->edge_term_samples;
  }
  auto noisy_write = [&](float sigma_next_call) {
    gc::NoisyWrite nw;
    nw.slots = h->d_slots; nw.c_out = c.c_out; nw.kp = h->kp; nw.scale = f_c_in(std::max(sigma_next_call, 1e-6f));
    if (cache) { nw.xn = h->d_xn; nw.ldn = h->nwp; }
    else nw.xp = h->d_xp;
    return nw;
  };
  auto churned = [&](int i) { return churn && i < n && h->churn_rates[i] > 0.f; };
  // x0 = noise * sigma_0  (dpm_solver_plus_plus_2s.py:71-78)
  bool written = false;                          // the packed input already holds c_in * (state of the next call)
  {
    const gc::NoisyWrite nw = (n > 0 && !churned(0)) ? noisy_write(sigmas[0]) : gc::NoisyWrite();
    if ((rc = launch(h, gc::KC_PACK, [&] { return gc::launch_scale(s, h->d_noise, sigmas[0], ne, h->d_sx, nw); })))
      return rc;
    written = nw.active();
  }
  if (multi) {
    gc::SigmaList sl{};
    for (size_t i = 0; i < call_sigma.size(); ++i) sl.v[i] = call_sigma[i];
    if ((rc = launch(h, gc::KC_COND, [&] {
           return gc::launch_cond_multi(s, sl, (int)call_sigma.size(), c.batch, h->d_nw0t, h->d_nb0, h->d_nw1t,
                                        h->d_nb1, c.noise_num_frequencies, c.noise_hidden, c.noise_base_period,
                                        h->d_wc_all, h->d_bc_all, h->cond_total, h->d_cond_all);
         })))
      return rc;
  }
  auto denoise = [&](const float* x, float sigma) -> int {
    const float ss = std::max(sigma, 1e-6f);  // :84-85
    if (!written) {
      int r = launch(h, gc::KC_PACK, [&] {
        return cache ? gc::launch_write_noisy_compact(s, x, rows, c.c_out, h->nwp, f_c_in(ss), h->d_xn)
                     : gc::launch_write_noisy(s, x, h->d_slots, rows, c.c_out, h->kp, f_c_in(ss), h->d_xp);
      });
      if (r) return r;
    }
    written = false;
    const float* ready = nullptr;
    if (multi) {
      if (calls >= (int)call_sigma.size() || call_sigma[calls] != ss)
        return fail(h, GC_ERR_INTERNAL, "sampler: noise-level list out of step with the loop");
      ready = h->d_cond_all + (size_t)calls * cond_call;
    }
    h->term_slot = route.edge_terms ? h->terms.call_slot[calls] : -1;
    ++calls;
    return forward(h, ss, ready);
  };
  for (int i = 0; i < n; ++i) {
    float sg = sigmas[i];
    const float sn = sigmas[i + 1];
    if (churn && h->churn_rates[i] > 0.f) {
      // apply_stochastic_churn (gencast/samplers_utils.py:434-452; called at dpm_solver_plus_plus_2s.py:128-137):
      // x <- x + spherical white noise * sqrt(max(s'^2 - s^2, 0)) * inflation, s' = s (1 + rate); the step
      // then runs from s'
      const float s_new = sg * (1.0f + h->churn_rates[i]);
      const float extra = std::sqrt(std::max(s_new * s_new - sg * sg, 0.0f)) * h->churn_inflation;
      if ((rc = noise_field(h, h->d_sx, extra, h->d_sx))) return rc;
      sg = s_new;
    }
    const float sm = std::sqrt(sg * sn);
    if ((rc = denoise(h->d_sx, sg))) return rc;
    const float ss = std::max(sg, 1e-6f);
    const float a_mid = sm / sg;
    {
      const bool mid_call = (sn != 0.0f) || !skip_dead;              // the mid-point state is denoised next
      const gc::NoisyWrite nw = mid_call ? noisy_write(sm) : gc::NoisyWrite();
      if ((rc = launch(h, gc::KC_PACK, [&] {
             return gc::launch_dpm_first(s, h->d_y, h->d_sx, f_c_out(ss), f_c_skip(ss), a_mid, ne,
                                         h->d_sden, h->d_smid, nw);
           })))
        return rc;
      written = nw.active();
    }
    if (sn == 0.0f) {
      // where(sigma_next == 0, x_denoised, x_next) (:148-153): the mid-point call is dead.
      if (!skip_dead && (rc = denoise(h->d_smid, sm))) return rc;
      GC_HIP(h, hipMemcpyAsync(h->d_sx, h->d_sden, ne * sizeof(float), hipMemcpyDeviceToDevice, s));
      written = false;
      continue;
    }
    if ((rc = denoise(h->d_smid, sm))) return rc;
    const float sms = std::max(sm, 1e-6f);
    const float a_next = sn / sg;
    {
      const gc::NoisyWrite nw = (i + 1 < n && !churned(i + 1)) ? noisy_write(sigmas[i + 1]) : gc::NoisyWrite();
      if ((rc = launch(h, gc::KC_PACK, [&] {
             return gc::launch_dpm_second(s, h->d_y, h->d_smid, f_c_out(sms), f_c_skip(sms), a_next, ne,
                                          h->d_sx, nw);
           })))
        return rc;
      written = nw.active();
    }
  }
  *calls_out = calls;
  return GC_OK;
}

int run_sampler(gc_handle* h, const float* sigmas, int n, int skip_dead, gc_sample_stats* stats) {
  const gc_config& c = h->cfg;
  const size_t ne = (size_t)h->hg.G * c.batch * c.c_out;
  hipStream_t s = h->stream;
  int rc, calls = 0;
  const unsigned long long stream0 = h->nz_stream;   // churn noise of this sample starts here
  const bool churn = !h->churn_rates.empty();
  if (churn && (int)h->churn_rates.size() != n)
    return fail(h, GC_ERR_INVALID_ARGUMENT, "gc_set_churn was given a schedule of another length than this sample");
  // The noise level of every denoiser call is known before the loop (churn included): all conditioning
  // vectors of the sample come from ONE launch instead of one per call.
  std::vector<float> call_sigma;
  for (int i = 0; i < n; ++i) {
    float sg = sigmas[i];
    if (churn && h->churn_rates[i] > 0.f) sg = sg * (1.0f + h->churn_rates[i]);
    call_sigma.push_back(std::max(sg, 1e-6f));
    const float sn = sigmas[i + 1];
    if (sn != 0.0f || !skip_dead) call_sigma.push_back(std::max(std::sqrt(sg * sn), 1e-6f));
  }
  const bool multi = (int)call_sigma.size() <= gc::kMaxSigmaList;
  const size_t cond_call = (size_t)c.batch * h->cond_total;
  if (multi && call_sigma.size() * cond_call > h->cond_all_cap) {
    if ((rc = dev_alloc(h, &h->d_cond_all, call_sigma.size() * cond_call))) return rc;
    h->cond_all_cap = call_sigma.size() * cond_call;
  }
  // the edge terms of this list of noise levels: built by the first sample that brings it, outside any capture
  if ((rc = multi ? ensure_edge_terms(h, call_sigma) : drop_edge_terms(h))) return rc;

  // ---- HIP-graph replay (the reference runs its whole sampler as ONE compiled program: the jax.lax.fori_loop of
  // dpm_solver_plus_plus_2s.py:157-158).  One sample is ~3 500 kernel launches that cost the host ~25 ms to enqueue
  // for ~50 ms of GPU work (nano), which caps how many members one thread can keep in flight.  A sample's launch
  // sequence depends only on its signature -- the noise levels (baked into kernel arguments), skip_dead, the
  // precision / feature mode and which of the two noise buffers it starts from -- so the SECOND sample with a
  // signature is captured (hipStreamBeginCapture on the handle's stream; the first ran eagerly and did every lazy
  // one-time set-up) and every later one is a single hipGraphLaunch.  Eager always: stochastic churn (its noise
  // stream counter is a kernel argument that changes per sample), per-class profiling (events between launches),
  // the debug stops.  Same kernels, same arguments, same order: samples are bit-identical to the eager path.
  const bool eligible = h->use_graphs && multi && !churn && h->prof_cls < 0 && h->debug_layer_limit < 0 &&
                        h->debug_stop_layer < 0;
  gc_handle::SampleGraph* sg = nullptr;
  if (eligible) {
    const Route r = make_route(h);
    for (auto& g : h->sample_graphs)
      if (g.skip_dead == skip_dead && g.noise == h->d_noise && g.route.f16 == r.f16 && g.feat16 == h->feat16 && g.route.st16 == r.st16 &&
          (int)g.sigmas.size() == n + 1 && !std::memcmp(g.sigmas.data(), sigmas, (n + 1) * sizeof(float)))
        sg = &g;
    if (!sg) {
      if (h->sample_graphs.size() >= 8) {            // forget the least recently used signature
        size_t lru = 0;
        for (size_t i = 1; i < h->sample_graphs.size(); ++i)
          if (h->sample_graphs[i].last_use < h->sample_graphs[lru].last_use) lru = i;
        destroy_sample_graph(h->sample_graphs[lru]);
        h->sample_graphs.erase(h->sample_graphs.begin() + lru);
      }
      gc_handle::SampleGraph g;
      g.sigmas.assign(sigmas, sigmas + n + 1);
      g.skip_dead = skip_dead; g.noise = h->d_noise; g.route = r; g.feat16 = h->feat16;
      g.last_use = ++h->graph_clock;
      h->sample_graphs.push_back(g);
      sg = nullptr;                                  // first sight: eager
    } else {
      sg->last_use = ++h->graph_clock;
    }
  }
  GC_HIP(h, hipEventRecord(h->ev0, s));
  // Threads and graphs (round 4; the record is in DESIGN.md section 5, "the six-thread hang").  What hung once in
  // round 3 was SIX host threads, each inside its handle's first graph call at the same moment: stream capture of
  // ~3 500 launches + hipGraphInstantiate, concurrently, on ROCm 7.2.  Replays alone never did (two threads replaying
  // captured graphs, and one thread driving six handles, ran clean; a hipGraphLaunch behind a running instance returns
  // in 0.06 ms: profiles/r03_graph_probe_nano20.txt).  So exactly that is serialised: capture + instantiate hold a
  // process-wide mutex; launches hold nothing.  Independently of it no executable is launched while its previous
  // instance may still run (two executables per signature, alternated, each behind its own event), and nothing lazy
  // is left for a capturing thread to do: the first, eager sample of a signature has made every one-time runtime
  // call (dynamic-LDS attributes are per device, not per thread; allocations).
  static std::mutex capture_mutex;
  // Field fallback: the cause of the round-3 hang was found by elimination, not observed in a debugger.
  // GC_TUNE_GRAPH_SERIALIZE=1 (h->graph_serialize) restores round 3's wider serialisation -- every hipGraphLaunch also
  // takes the mutex -- without a rebuild, should concurrent launch + capture ever misbehave on another ROCm.
  auto launch_exec = [&](gc_handle::SampleGraph* g) -> int {
    std::unique_lock<std::mutex> launch_lock(capture_mutex, std::defer_lock);
    if (h->graph_serialize) launch_lock.lock();
    const int i = g->exec2 ? g->next : 0;
    hipGraphExec_t ex = i ? g->exec2 : g->exec;
    if (!g->done[i]) GC_HIP(h, hipEventCreateWithFlags(&g->done[i], hipEventDisableTiming));
    else GC_HIP(h, hipEventSynchronize(g->done[i]));   // its previous instance has ended (usually long ago)
    GC_HIP(h, hipGraphLaunch(ex, s));
    GC_HIP(h, hipEventRecord(g->done[i], s));
    g->next = i ^ 1;
    return GC_OK;
  };
  if (sg && sg->exec) {
    if ((rc = launch_exec(sg))) return rc;
    calls = sg->calls;
    h->launches_last_call = sg->launches_per_call;
    h->route = h->last_route = sg->route;
    if (sg->route.edge_terms) ++h->edge_term_samples;
    ++h->graph_replays;
  } else if (sg) {
    const int64_t l0 = h->launch_count;
    auto say = [&](const char* what) { if (h->graph_verbose) { std::fprintf(stderr, "[gc graph] %s\n", what); std::fflush(stderr); } };
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr, exec2 = nullptr;
    {
      std::lock_guard<std::mutex> capture_lock(capture_mutex);
      say("begin capture");
      GC_HIP(h, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      rc = sampler_body(h, sigmas, n, skip_dead, call_sigma, multi, &calls);
      const hipError_t e_end = hipStreamEndCapture(s, &graph);
      say("end capture");
      if (rc) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
      }
      if (e_end != hipSuccess || !graph) return fail(h, GC_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e_end));
      hipError_t e_inst = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      if (e_inst == hipSuccess) e_inst = hipGraphInstantiate(&exec2, graph, nullptr, nullptr, 0);
      if (e_inst != hipSuccess) {
        if (exec) (void)hipGraphExecDestroy(exec);
        (void)hipGraphDestroy(graph);
        return fail(h, GC_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e_inst));
      }
      say("instantiated");
    }
    sg->graph = graph; sg->exec = exec; sg->exec2 = exec2; sg->calls = calls; sg->next = 0;
    sg->launches = h->launch_count - l0;
    sg->launches_per_call = h->launches_last_call;
    sg->route = h->last_route;
    ++h->graph_captures;
    if ((rc = launch_exec(sg))) return rc;
    say("launched");
    ++h->graph_replays;
  } else if ((rc = sampler_body(h, sigmas, n, skip_dead, call_sigma, multi, &calls))) {
    return rc;
  }
  GC_HIP(h, hipEventRecord(h->ev1, s));
  h->has_sample = true;
  // domain guard: NaN / Inf stick to a sample row once they appear, so one check of the final sample
  // covers all 39 calls; it is resolved at the next synchronising entry point (resolve_guard)
  if (make_route(h).f16) {
    if ((rc = guard_enqueue(h, h->d_sx, ne))) return rc;
    h->last_sigmas.assign(sigmas, sigmas + n + 1);
    h->last_skip_dead = skip_dead;
    h->guard_pending = true;
    h->last_stream0 = stream0;
    h->last_noise = h->d_noise;
  }
  if (stats) {
    GC_HIP(h, hipEventSynchronize(h->ev1));
    float ms = 0.f;
    GC_HIP(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    stats->denoiser_calls = calls;
    stats->device_ms = ms;
  }
  return GC_OK;
}

// Waits for the stream; if the last resident sample left the f16x3 domain (its output holds NaN /
// Inf), samples again with the exact-f32 kernels from the same noise and conditioning.
int resolve_guard(gc_handle* h) {
  GC_HIP(h, hipStreamSynchronize(h->stream));
  if (!h->guard_pending) return GC_OK;
  h->guard_pending = false;
  if (!guard_tripped(h)) return GC_OK;
  ++h->range_fallbacks;
  h->in_fallback = true;
  const unsigned long long stream_end = h->nz_stream;
  h->nz_stream = h->last_stream0;                    // the re-run draws the same churn noise
  const std::vector<float> sig = h->last_sigmas;
  float* const noise_next = h->d_noise;              // the re-run starts from the noise of the sample it repeats
  h->d_noise = h->last_noise;
  int rc = run_sampler(h, sig.data(), (int)sig.size() - 1, h->last_skip_dead, nullptr);
  h->d_noise = noise_next;
  h->nz_stream = stream_end;
  h->in_fallback = false;
  if (rc) return rc;
  GC_HIP(h, hipStreamSynchronize(h->stream));
  return GC_OK;
}

void destroy_sample_graph(gc_handle::SampleGraph& g) {
  for (hipEvent_t& e : g.done)                       // an executable is destroyed only after its last launch has ended
    if (e) { (void)hipEventSynchronize(e); (void)hipEventDestroy(e); e = nullptr; }
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.exec2) (void)hipGraphExecDestroy(g.exec2);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = g.exec2 = nullptr;
  g.graph = nullptr;
}

// Captured sampler graphs bake device pointers and launch geometry: dropped whenever those may change.
void drop_sample_graphs(gc_handle* h) {
  for (auto& g : h->sample_graphs) destroy_sample_graph(g);
  h->sample_graphs.clear();
}

// One evaluation of the denoising objective on the resident conditioning and targets (gc_loss_resident): optionally a
// fresh noise field into the initial-noise buffer, x = t + sigma n and its scaled copy into the packed input, the forward
// in the every-column form of gc_denoise (no embed cache, never captured), the reduction into slot `e` of the result
// arrays.  `sig` = this evaluation's noise levels on the device.
int loss_eval(gc_handle* h, int e, const float* sig, bool draw_noise, bool want_den) {
  const gc_config& c = h->cfg;
  const int G = h->hg.G, B = c.batch, ng = h->loss_groups;
  hipStream_t s = h->stream;
  int rc;
  if (draw_noise) {
    if ((rc = noise_field(h, nullptr, 1.0f, h->d_noise))) return rc;
    h->has_noise = true;
  }
  if ((rc = launch(h, gc::KC_PACK, [&] {
         return gc::launch_loss_noisy(s, h->d_targets, h->d_noise, sig, h->d_slots, G * B, B, c.c_out, h->kp, h->d_lx, h->d_xp);
       })))
    return rc;
  float* const sigma_own = h->d_sigma;           // forward(h, -1) reads the noise levels from h->d_sigma
  h->d_sigma = const_cast<float*>(sig);
  rc = forward(h, -1.0f);
  h->d_sigma = sigma_own;
  if (rc) return rc;
  if ((rc = launch(h, gc::KC_PACK, [&] {
         return gc::launch_loss_reduce(s, h->d_y, h->d_targets, h->d_noise, h->d_lx, sig, h->d_lw_node, G, B, c.c_out,
                                       h->d_lpart, want_den ? h->d_lden : nullptr);
       })))
    return rc;
  return launch(h, gc::KC_PACK, [&] {
    return gc::launch_loss_finish(s, h->d_lpart, gc::loss_reduce_blocks(G, B, c.c_out), sig, h->d_lw_chan, h->d_l_group,
                                  h->d_lw_group, B, c.c_out, ng, h->d_lloss + (size_t)e * B, h->d_lpg + (size_t)e * B * ng);
  });
}

}  // namespace gci
