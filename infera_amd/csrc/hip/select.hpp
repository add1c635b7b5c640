// select.hpp -- the running best-k list shared by nearest.hip and reduce.hip (TopK): K (value, index) pairs in registers, kept sorted by
// the total order "smaller value first, NaN after every number, equal values (and NaNs) by lower index".  Every index is static after
// unrolling, so the list never leaves the VGPRs.
#pragma once

#include "device_common.hpp"

namespace infera_hip::kern {

constexpr int kSelectNone = 0x7fffffff;  // the index of an empty entry: (NaN, kSelectNone) ranks after every candidate

__device__ __forceinline__ bool select_before(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an != bn) return bn;
  return av < bv || (!(av > bv) && ai < bi);
}

template <int K>
struct BestList {
  float v[K];
  int i[K];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < K; j++) v[j] = __builtin_nanf(""), i[j] = kSelectNone;
  }
  // keeps the best K of the list and (cv, ci)
  __device__ __forceinline__ void insert(float cv, int ci) {
    if (!select_before(cv, ci, v[K - 1], i[K - 1])) return;
    v[K - 1] = cv, i[K - 1] = ci;
#pragma unroll
    for (int j = K - 1; j > 0; j--) {
      const bool sw = select_before(v[j], i[j], v[j - 1], i[j - 1]);
      const float tv = v[j - 1];
      const int ti = i[j - 1];
      v[j - 1] = sw ? v[j] : tv, i[j - 1] = sw ? i[j] : ti;
      v[j] = sw ? tv : v[j], i[j] = sw ? ti : i[j];
    }
  }
};

}  // namespace infera_hip::kern
