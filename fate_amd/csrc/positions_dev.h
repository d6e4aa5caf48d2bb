// SecureBoost bin indexes -> fold terms (fphe_positions_terms).
#pragma once
#include "mont_dev.h"

namespace {
using namespace fphe;

// positions [ns][npos] (int32 or int64, sample-major as iupdate's Vec<Vec<usize>>): term
// (i, j, t) = pair p = i npos + j, then t < stride, at p stride + t: src = i stride + t, slot =
// pos stride + t, or -1 when pos is outside [0, lim) (fphe_fold_segments then reports the
// segment out of range).  One thread per pair; the range test runs on the position's own width.
template <typename PT>
__global__ __launch_bounds__(256) void k_positions_terms(const PT* __restrict__ pos, size_t npairs, uint32_t npos,
                                                          int32_t stride, int64_t lim, int32_t* __restrict__ src,
                                                          int32_t* __restrict__ slot) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < npairs; p += (size_t)gridDim.x * blockDim.x) {
    const int64_t v = (int64_t)pos[p];
    const bool ok = v >= 0 && v < lim;
    const int32_t i = (int32_t)(p / npos);
    for (int32_t t = 0; t < stride; ++t) {
      src[p * stride + t] = i * stride + t;
      slot[p * stride + t] = ok ? (int32_t)v * stride + t : -1;
    }
  }
}
}  // namespace
