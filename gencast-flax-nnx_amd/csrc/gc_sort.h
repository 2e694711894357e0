// The register sorting network of the scorers that need the members of a point in ascending order (gc_order.hip,
// gc_clim.hip, gc_tail.hip): the padded load, the network, and the host's choice of the padded size.  P is the padded
// size, a power of two in 2..64.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace gc {

// The n <= P values base[k * stride + i], k < n, into v, +inf behind them (the network sorts the padding to the end).
// Each load is coalesced across the wave.  Returns whether all n are finite: the network must never see a NaN.
// each(x) sees every loaded value in slot order k = 0, 1, ..: the place for sums that are defined in that order.
template <int P, class Each>
__device__ inline bool load_padded(float (&v)[P], const float* __restrict__ base, size_t stride, size_t i, int n, Each each) {
  bool fin = true;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    v[k] = __builtin_inff();
    if (k < n) {
      const float x = base[(size_t)k * stride + i];
      v[k] = x;
      fin = fin && isfinite(x);
      each(x);
    }
  }
  return fin;
}
template <int P>
__device__ inline bool load_padded(float (&v)[P], const float* __restrict__ base, size_t stride, size_t i, int n) {
  return load_padded<P>(v, base, stride, i, n, [](float) {});
}

// f(std::integral_constant<int, P>) for the smallest padded size P >= n (host code; n <= 64)
template <class F>
static auto pad_dispatch(int n, F&& f) {
  if (n <= 2) return f(std::integral_constant<int, 2>{});
  if (n <= 4) return f(std::integral_constant<int, 4>{});
  if (n <= 8) return f(std::integral_constant<int, 8>{});
  if (n <= 16) return f(std::integral_constant<int, 16>{});
  if (n <= 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

template <int P>
struct OrdLog { static constexpr int value = P == 2 ? 1 : P == 4 ? 2 : P == 8 ? 3 : P == 16 ? 4 : P == 32 ? 5 : 6; };

// Bitonic network over P = 2^n registers, ascending: P/2 compare-exchanges per stage, n (n + 1) / 2 stages, every index
// a compile-time constant.  No branch depends on the data.
template <int P>
__device__ inline void ord_sort(float (&v)[P]) {
  constexpr int kLog = OrdLog<P>::value;
  static_assert(P == 1 << kLog, "P is a power of two in 2..64");
#pragma unroll
  for (int s = 1; s <= kLog; ++s) {                // merges of runs of 2^s
#pragma unroll
    for (int t = s - 1; t >= 0; --t) {             // compare-exchange at distance 2^t
#pragma unroll
      for (int i = 0; i < P; ++i) {
        const int l = i ^ (1 << t);
        if (l > i) {
          const float a = v[i], b = v[l];
          const float lo = fminf(a, b), hi = fmaxf(a, b);
          const bool up = (i & (1 << s)) == 0;
          v[i] = up ? lo : hi;
          v[l] = up ? hi : lo;
        }
      }
    }
  }
}

}  // namespace gc
