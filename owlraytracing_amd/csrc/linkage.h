// linkage.h -- what linkage.hip offers the two calls that build a dendrogram (Engine::linkage, Engine::hdbscan_labels): the
// workspace it needs and the solve on arrays the caller owns.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "lbvh.h"  // OWLMI_HIP

namespace owlmi {

// the dendrogram's arrays (include/owlknn_hdbscan.h), none of them null: what the caller did not ask for lies in the workspace
struct LinkageArrays {
  int32_t *parent;        // n + edges
  int32_t *left, *right;  // edges
  int32_t *size;          // edges
};
struct LinkageRun {
  int rounds = 0;
  int64_t absorbed = 0, host_edges = 0, roots = 0;
};

inline size_t linkage_align(size_t b) { return (b + 255) & ~(size_t)255; }
// the bytes linkage_run needs at `ws` for n vertices and that many records
size_t linkage_workspace_bytes(int64_t n, int64_t edges, hipStream_t s);
// The dendrogram of the records (d_u, d_v) in their order; `h_words` are four pinned words for the rounds' read-backs.
// Synchronises the stream.
LinkageRun linkage_run(char *ws, int64_t n, int64_t edges, const int32_t *d_u, const int32_t *d_v, const LinkageArrays &out, int max_rounds,
                       unsigned long long *h_words, hipStream_t s);

// device memory for the length of a call, where the engine's one workspace is taken by a call inside it or the need is rare
struct DeviceBuffer {
  void *p = nullptr;
  explicit DeviceBuffer(size_t bytes) { OWLMI_HIP(hipMalloc(&p, bytes > 16 ? bytes : 16)); }
  ~DeviceBuffer() { (void)hipFree(p); }
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
};

// 16^passes >= count: the launches of a sixteen-step pointer jump after which every chain of `count` pointers has ended
inline int jump_passes(int64_t count) {
  int p = 1;
  while (p < 16 && (1ll << (4 * p)) < count) p++;
  return p;
}

}  // namespace owlmi
