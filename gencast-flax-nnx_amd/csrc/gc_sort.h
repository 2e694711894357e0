// The register sorting network of the scorers that need the members of a point in ascending order (gc_order.hip,
// gc_clim.hip).  Device code only; P is the padded size, a power of two in 2..64.
#pragma once
#include <hip/hip_runtime.h>

namespace gc {

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
