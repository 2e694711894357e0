// Time-window ensemble fields on the device (include/gencast_hip.h, gc_ens_window_*): the members and the truth of the
// last L lead times of one handle's gc_ens_* store, kept in a ring on a second handle, become in that handle's store one
// field each -- an accumulation or any other linear combination over time, or the extreme over time.  Every scorer of the
// library then works on that store as it is.  Kernel and host code live together here; DESIGN.md section 8j has the
// definitions.
//
// The ring is ONE buffer of L slots; a slot is the flat array of the M member fields followed by the truth,
// (M + 1) field floats, at a stride padded to a multiple of four floats.  A push is two device-to-device copies into slot
// pushes % L.  An emit is one launch: a thread owns four consecutive floats of the flat array, reads them from the L slots
// in time order (oldest first) and writes once.  No atomics, one writer per output, a fixed order of addition: the same
// emit twice gives the same bytes.
#include "gc_store.h"

// the per-element arithmetic is the definition, operation for operation: a rounded product, then a rounded sum
#pragma clang fp contract(off)

namespace gc {

enum { kWinLinear = 0, kWinMax = 1, kWinMin = 2 };
constexpr int kWinMaxLength = 64;
constexpr int kWinAhead = 4;                     // slots whose loads are issued in front of the serial chain

// One time step of one element.  LINEAR: acc <- acc + a x in double.  MAX / MIN: the strict comparison keeps the older
// value on a tie, so the result is a fixed one of the inputs (also between +0 and -0).
template <int KIND>
__device__ inline void win_step(double& acc, float& ext, bool& bad, float x, double a, bool first) {
  bad = bad || !isfinite(x);
  if constexpr (KIND == kWinLinear) {
    const double p = a * (double)x;
    acc = acc + p;
  } else if constexpr (KIND == kWinMax) {
    ext = (first || x > ext) ? x : ext;
  } else {
    ext = (first || x < ext) ? x : ext;
  }
}

// ring [L][stride]; element e of the flat array of a slot is member e / field's float e % field for e < n_mem = M field,
// the truth's float e - n_mem behind.  Thread g owns e = 4 g .. 4 g + 3: stride % 4 == 0 and the ring is aligned like
// every hipMalloc, so its four floats of every slot are one aligned float4 that lies inside the slot (the padding at the
// end of a slot is read by the last thread and not used).  The outputs are two buffers, the member store and the truth:
// a thread whose four floats lie inside the member store writes a float4, the threads across the seam and in the truth
// write float by float.
template <int KIND>
__global__ __launch_bounds__(256) void gc_ens_window_kernel(const float* __restrict__ ring, size_t stride, int L, int start,
                                                             const double* __restrict__ coef, float* __restrict__ mem,
                                                             float* __restrict__ truth, size_t n_mem, size_t total) {
  const size_t e0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (e0 >= total) return;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  float ext[4] = {0.f, 0.f, 0.f, 0.f};
  bool bad[4] = {false, false, false, false};
  int slot = start;                                // the oldest push of the window; then in time order, wrapping
  for (int t0 = 0; t0 < L; t0 += kWinAhead) {
    float4 v[kWinAhead];
    int s = slot;
#pragma unroll
    for (int k = 0; k < kWinAhead; ++k) {
      if (t0 + k < L) v[k] = *reinterpret_cast<const float4*>(ring + (size_t)s * stride + e0);
      if (++s == L) s = 0;
    }
    slot = s;
#pragma unroll
    for (int k = 0; k < kWinAhead; ++k) {
      if (t0 + k < L) {
        const double a = KIND == kWinLinear ? coef[t0 + k] : 0.0;
        const bool first = t0 + k == 0;
        win_step<KIND>(acc[0], ext[0], bad[0], v[k].x, a, first);
        win_step<KIND>(acc[1], ext[1], bad[1], v[k].y, a, first);
        win_step<KIND>(acc[2], ext[2], bad[2], v[k].z, a, first);
        win_step<KIND>(acc[3], ext[3], bad[3], v[k].w, a, first);
      }
    }
  }
  float out[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float r = KIND == kWinLinear ? (float)acc[i] : ext[i];
    out[i] = bad[i] ? __builtin_nanf("") : r;
  }
  if (e0 + 4 <= n_mem) {
    *reinterpret_cast<float4*>(mem + e0) = make_float4(out[0], out[1], out[2], out[3]);
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const size_t e = e0 + i;
    if (e < n_mem) mem[e] = out[i];
    else if (e < total) truth[e - n_mem] = out[i];
  }
}

static hipError_t launch_ens_window(hipStream_t s, int kind, const float* ring, size_t stride, int L, int start,
                                    const double* coef, float* mem, float* truth, size_t n_mem, size_t total) {
  const dim3 grid((unsigned)((total + 1023) / 1024));
  if (kind == kWinLinear)
    hipLaunchKernelGGL((gc_ens_window_kernel<kWinLinear>), grid, dim3(256), 0, s, ring, stride, L, start, coef, mem, truth, n_mem, total);
  else if (kind == kWinMax)
    hipLaunchKernelGGL((gc_ens_window_kernel<kWinMax>), grid, dim3(256), 0, s, ring, stride, L, start, coef, mem, truth, n_mem, total);
  else
    hipLaunchKernelGGL((gc_ens_window_kernel<kWinMin>), grid, dim3(256), 0, s, ring, stride, L, start, coef, mem, truth, n_mem, total);
  return hipGetLastError();
}

}  // namespace gc

using namespace gci;

// floats of one ring slot: the M members and the truth, padded to whole float4s
static size_t win_stride(const gc_handle* h, int M) { return ((size_t)(M + 1) * field_len(h) + 3) / 4 * 4; }

extern "C" {

int gc_ens_window_set(gc_handle* h, int32_t kind, int32_t length, const double* coef) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  if (int rc = need_graph(h)) return rc;
  if (kind < gc::kWinLinear || kind > gc::kWinMin) return fail(h, GC_ERR_UNSUPPORTED, "kind must be 0 (linear), 1 (max) or 2 (min)");
  if (length < 1) return fail(h, GC_ERR_INVALID_ARGUMENT, "length must be at least 1");
  if (length > gc::kWinMaxLength) return fail(h, GC_ERR_UNSUPPORTED, "length must be at most 64");
  if (kind == gc::kWinLinear) {
    if (!coef) return fail(h, GC_ERR_INVALID_ARGUMENT, "a linear window needs its coefficients");
    for (int t = 0; t < length; ++t)
      if (!std::isfinite(coef[t])) return fail(h, GC_ERR_INVALID_ARGUMENT, "coef[" + std::to_string(t) + "] is not finite");
  }
  GC_HIP(h, hipSetDevice(h->device));
  int rc;
  if (!h->d_win_coef) {                              // 64 doubles, made once
    if ((rc = dev_alloc(h, &h->d_win_coef, (size_t)gc::kWinMaxLength))) return rc;
    GC_HIP(h, h->ev_win_src.ensure());
  }
  h->win_set = false;
  double a[gc::kWinMaxLength] = {};
  if (kind == gc::kWinLinear) std::copy(coef, coef + length, a);
  if ((rc = store_upload(h, h->d_win_coef, a, sizeof(a)))) return rc;
  h->win_kind = kind;
  h->win_L = length;
  h->win_pushes = 0;                                 // (the ring itself is made again by the push that finds L or M changed)
  h->win_set = true;
  return GC_OK;
  });
}

int gc_ens_window_push(gc_handle* h, gc_handle* src, const float* truth) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_source(h, src)) || (rc = need_graph(h)) || (rc = need(h, h->win_set, "no plan (gc_ens_window_set)")) ||
      (rc = check_peer(h, src, "source", false, h->cfg.c_out)))
    return rc;
  const int M = src->ens_members, L = h->win_L;
  const size_t ring_M = h->win_allocs.key[1];
  if ((rc = need(h, M != 0, "no member store on the source handle (gc_ens_reserve)"))) return rc;
  if (h->win_pushes > 0 && (size_t)M != ring_M)
    return fail(h, GC_ERR_STATE, "the source holds " + std::to_string(M) + " members, the ring " + std::to_string(ring_M) +
                                     " (gc_ens_window_reset first)");
  if ((rc = store_complete(h, src, "source "))) return rc;
  GC_HIP(h, hipSetDevice(h->device));
  if ((rc = take_truth(h, src, truth, "gc_ens_window_push"))) return rc;   // into the source's truth buffer, as gc_ens_derive does
  const size_t field = field_len(h), stride = win_stride(h, M);
  if ((rc = sized_for(h, h->win_allocs, {(size_t)L, (size_t)M}, buf(&h->d_win_ring, (size_t)L * stride)))) return rc;
  hipStream_t s = h->stream;
  // the source's store and truth are complete on ITS stream: this handle's stream goes on behind them
  if ((rc = order_behind(h, h->ev_win_src, src->stream, s))) return rc;
  float* const slot = h->d_win_ring + (size_t)(h->win_pushes % L) * stride;
  GC_HIP(h, hipMemcpyAsync(slot, src->d_ens, (size_t)M * field * sizeof(float), hipMemcpyDeviceToDevice, s));
  GC_HIP(h, hipMemcpyAsync(slot + (size_t)M * field, src->d_ens_truth, field * sizeof(float), hipMemcpyDeviceToDevice, s));
  GC_HIP(h, hipStreamSynchronize(s));                // (the copies have read the source's store: it may be pushed into again)
  ++h->win_pushes;
  return GC_OK;
  });
}

int gc_ens_window_emit(gc_handle* h) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  int rc;
  if ((rc = need_graph(h)) || (rc = need(h, h->win_set, "no plan (gc_ens_window_set)"))) return rc;
  const int L = h->win_L, M = h->ens_members;
  if (h->win_pushes < L)
    return fail(h, GC_ERR_STATE, "the window needs " + std::to_string(L) + " pushes, the ring holds " + std::to_string(h->win_pushes));
  if ((rc = need_store(h))) return rc;
  if (h->win_allocs.differs({(size_t)L, (size_t)M}))
    return fail(h, GC_ERR_STATE, "the member store holds " + std::to_string(M) + " members, the ring " + std::to_string(h->win_allocs.key[1]));
  GC_HIP(h, hipSetDevice(h->device));
  const size_t field = field_len(h), stride = win_stride(h, M);
  if ((rc = own_truth_buffer(h))) return rc;             // the source here is the ring: of fill_open, the parts that apply
  hipStream_t s = h->stream;
  store_rewritten(h);
  const int start = (int)((h->win_pushes - L) % L);
  rc = timed(h, h->win,
             [&] {
               return launch_each(h, [&] {
                 return gc::launch_ens_window(s, h->win_kind, h->d_win_ring, stride, L, start, h->d_win_coef, h->d_ens, h->d_ens_truth,
                                              (size_t)M * field, (size_t)(M + 1) * field);
               });
             },
             no_readbacks);
  if (rc) return rc;
  fill_close(h);
  return GC_OK;
  });
}

int gc_ens_window_reset(gc_handle* h) {
  return guarded(h, [&]() -> int {
  if (!h) return GC_ERR_INVALID_ARGUMENT;
  h->win_pushes = 0;
  return GC_OK;
  });
}

}  // extern "C"
