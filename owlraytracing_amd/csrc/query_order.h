// query_order.h -- the order in which the engine works through query points that are NOT in the tree (tknnQuery in
// trueknn_query.hip, tknnDbscanQuery in dbscan.hip, its kernel in dbscan_label.hip): along the tree's own curve, so that the lanes of a wave and the waves of a
// workgroup's neighbours walk neighbouring nodes.  The key kernel and the radix sort are written here once; a caller brings the
// four columns and the sort's temporary storage from its own workspace layout.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <hipcub/hipcub.hpp>

#include "curve_key.h"
#include "lbvh.h"  // OWLMI_HIP

namespace owlmi {
namespace {

constexpr int kQueryOrderBlock = 256;
constexpr int kCodeBits = 30;  // ten bits per axis order 10 M queries well enough, and sort in half the passes

// The tree's quantisation (cubic cells over the scene box, one scale for all axes: lbvh.hip) at ten bits per
// axis, along the curve the tree was sorted by (the key is hierarchical: ten levels order the queries as the first ten
// of the tree's 21 order its points); queries outside the box are clamped to its faces, queries with a NaN coordinate sort last.
__global__ void __launch_bounds__(kQueryOrderBlock) query_code_kernel(const float *__restrict__ queries, int32_t m, const float *__restrict__ scene,
                                                                     uint32_t *__restrict__ codes, uint32_t *__restrict__ order, int curve) {
  const int32_t i = blockIdx.x * kQueryOrderBlock + threadIdx.x;
  if (i >= m) return;
  const float c[3] = {queries[3 * (int64_t)i], queries[3 * (int64_t)i + 1], queries[3 * (int64_t)i + 2]};
  const float ext = fmaxf(fmaxf(scene[3] - scene[0], scene[4] - scene[1]), scene[5] - scene[2]);
  const uint32_t code = (uint32_t)curve_point_key(curve, c[0], c[1], c[2], scene[0], scene[1], scene[2], ext, kCodeBits / 3);
  codes[i] = code;
  order[i] = (uint32_t)i;
}

// bytes of temporary storage the sort of m queries asks for
inline size_t query_order_sort_bytes(int64_t m, hipStream_t s) {
  uint32_t *null_u32 = nullptr;
  size_t sort_bytes = 0;
  OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, null_u32, null_u32, null_u32, null_u32, (int)m, 0, kCodeBits + 1, s));
  return sort_bytes;
}

// order[i] = the caller's index of the query worked on at position i.  `scene`, `curve`: the tree's (Lbvh::scene_device(),
// Lbvh::curve()); codes, codes_sorted, order_in, order: m words each; sort_tmp: query_order_sort_bytes(m) bytes.
inline void query_order(const float *d_queries, int64_t m, const float *scene, int curve, uint32_t *codes, uint32_t *codes_sorted, uint32_t *order_in,
                        uint32_t *order, void *sort_tmp, size_t sort_bytes, hipStream_t s) {
  hipLaunchKernelGGL(query_code_kernel, dim3((unsigned)((m + kQueryOrderBlock - 1) / kQueryOrderBlock)), dim3(kQueryOrderBlock), 0, s, d_queries, (int32_t)m,
                     scene, codes, order_in, curve);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, codes, codes_sorted, order_in, order, (int)m, 0, kCodeBits + 1, s));
}

}  // namespace
}  // namespace owlmi
