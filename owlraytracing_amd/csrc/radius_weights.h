// radius_weights.h -- the kernel weights of include/owlknn_reduce.h (TKNN_W_*), for the calls that weigh the points within a
// radius: tknnRadiusReduce (radius_reduce.hip) and tknnMeanShift (mean_shift.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "owlknn_reduce.h"

namespace owlmi {
namespace {

// of a point that passed the predicate: d2 = knn_dist2, d = knn_sqrt(d2), every operation rounded on its own
template <int WEIGHT>
__device__ __forceinline__ float rd_weight(float d2, float d, float coef) {
#pragma clang fp contract(off)
  if constexpr (WEIGHT == TKNN_W_GAUSS) {
    return expf(d2 * coef);
  } else if constexpr (WEIGHT == TKNN_W_EPANECHNIKOV) {
    return fmaxf(0.f, 1.f - d2 * coef);
  } else if constexpr (WEIGHT == TKNN_W_CUBIC_SPLINE) {
    const float s = d * coef, s2 = s * s, t = 2.f - s;
    const float inner = (1.f - 1.5f * s2) + 0.75f * (s2 * s), outer = fmaxf(0.f, 0.25f * ((t * t) * t));
    return s <= 1.f ? inner : outer;
  } else {
    return 1.f;
  }
}
__device__ __forceinline__ float rd_weight_of(int weight, float d2, float d, float coef) {
  switch (weight) {
    case TKNN_W_GAUSS: return rd_weight<TKNN_W_GAUSS>(d2, d, coef);
    case TKNN_W_EPANECHNIKOV: return rd_weight<TKNN_W_EPANECHNIKOV>(d2, d, coef);
    case TKNN_W_CUBIC_SPLINE: return rd_weight<TKNN_W_CUBIC_SPLINE>(d2, d, coef);
    default: return 1.f;
  }
}

}  // namespace
}  // namespace owlmi
