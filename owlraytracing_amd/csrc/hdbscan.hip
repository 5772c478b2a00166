// hdbscan.hip -- HDBSCAN's labels of a sorted forest (tknnHdbscanLabels) and the whole pipeline on the built set (tknnHdbscan),
// include/owlknn_hdbscan.h; tests/hdbscan_spec.py labels() is the same in numpy.
//
// After the dendrogram (linkage.hip) the nodes are the leaves 0 .. n-1 and n + i for record i; mcs is min_cluster_size.
//   hd_kind_kernel:    per internal node: big (size >= mcs), split (both children big).
//   hd_head_kernel:    a big node is a cluster head if it is a root or its parent is a split; jump[x] = x for a head, else parent.
//   hd_jump_kernel:    launched jump_passes(edges) times: jump[x] = the nearest head at or above the big node x, its cluster.
//   hd_points_kernel:  a(p) = the lowest big strict ancestor of point p, fewer than mcs steps up (sizes grow strictly upwards);
//                      lambda_p = lambda(a(p)).
//   hd_stability_kernel: every point adds lambda_p - birth to the cluster of a(p), every split size * (lambda - birth) to the
//                      cluster it ends; fp64 atomics, the lanes of a wave that share a cluster summed first.
//   hd_records_kernel: the heads, numbered in ascending node order by a scan: (stability, parent cluster) for the host.
//   the host: the excess-of-mass pass over those records -- ascending order is children before parents, a parent's rank is the
//                      higher --, then downwards the highest winning ancestor-or-self of every cluster.
//   hd_raw_label_kernel, hd_first_row_kernel, a scan, hd_number_kernel: a point takes the chosen cluster of the cluster it left;
//                      the chosen clusters are numbered by their smallest row.
// What a kernel reads was written by an earlier launch, except in hd_jump_kernel (relaxed atomics of agent scope; a stale pointer
// is an ancestor on the same chain and costs a step, no more).  Every loop has a step count; none waits for another thread.
// Input that is no forest leaves nodes without children or sizes: the kernels check every index they take from the arrays.
#include "linkage.h"
#include "trueknn_engine.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <vector>

namespace owlmi {

namespace {

constexpr int kHdBlock = 256;
constexpr int kHdJumpSteps = 16;
constexpr uint8_t kHdBig = 1, kHdSplit = 2, kHdHead = 4;
constexpr uint32_t kHdNoRow = 0xffffffffu;
// the call's words: [0] cluster heads, [1] labels given, [2] noise points
constexpr int kHdHeads = 0, kHdClusters = 1, kHdNoise = 2, kHdWords = 4;

struct HdArgs {
  int32_t n, edges, mcs;
  const float *w;
  const int32_t *parent, *left, *right, *size;
  uint8_t *kind;       // per internal node
  int32_t *jump;       // per internal node: towards its cluster's head (node numbers)
  int32_t *a;          // per point: its lowest big strict ancestor, or -1
  double *stab;        // per internal node, meaningful at heads
  int32_t *head_flag, *cluster_of;  // per internal node: 1 at heads; the scan: a head's number among the heads
  double *c_stab;      // per cluster
  int32_t *c_parent;   // per cluster: the cluster its head's parent lies in, -1 for a root cluster
  int32_t *chosen;     // per cluster, from the host: the highest winning ancestor-or-self, -1 if none
  uint32_t *first_row; // per cluster: the smallest row labelled with it
  int32_t *row_flag, *row_number;   // per row: 1 where a chosen cluster has its smallest row; the scan
  int32_t *labels;
  double *lambda;
  unsigned long long *words;
};

__device__ __forceinline__ bool hd_internal(const HdArgs &a, int32_t x) { return x >= a.n && x < a.n + a.edges; }
__device__ __forceinline__ double hd_lambda(const HdArgs &a, int32_t x) {  // x: an internal node
  double w = (double)a.w[x - a.n];
  if (w == 0.0) w = 0x1p-126;  // FLT_MIN
  return 1.0 / w;
}
__device__ __forceinline__ double hd_birth(const HdArgs &a, int32_t head) {
  const int32_t up = a.parent[head];
  return hd_internal(a, up) ? hd_lambda(a, up) : 0.0;
}
__device__ __forceinline__ int32_t hd_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// table[at] += v for the lanes with `has`, every lane of the wave calling: the lanes of one destination are summed first
__device__ __forceinline__ void hd_group_add(bool has, int32_t at, double v, double *table) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(has);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t to = __shfl(at, leader);
    const bool mine = has && at == to;
    const unsigned long long group = __ballot(mine);
    double sum = mine ? v : 0.0;
    if (group & (group - 1)) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    }
    if (lane == leader) atomicAdd(table + to, sum);
    todo &= ~group;
  }
}
// table[at] = min(table[at], v), likewise
__device__ __forceinline__ void hd_group_min(bool has, int32_t at, uint32_t v, uint32_t *table) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(has);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t to = __shfl(at, leader);
    const bool mine = has && at == to;
    const unsigned long long group = __ballot(mine);
    uint32_t m = mine ? v : kHdNoRow;
    if (group & (group - 1)) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) m = min(m, (uint32_t)__shfl_xor(m, off));
    }
    if (lane == leader && __hip_atomic_load(table + to, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > m) atomicMin(table + to, m);
    todo &= ~group;
  }
}

__global__ void __launch_bounds__(kHdBlock) hd_kind_kernel(HdArgs a) {
  const int32_t i = blockIdx.x * kHdBlock + threadIdx.x;
  if (i >= a.edges) return;
  auto big = [&](int32_t x) { return x >= 0 && x < a.n + a.edges && (x >= a.n ? a.size[x - a.n] : 1) >= a.mcs; };
  uint8_t kind = a.size[i] >= a.mcs ? kHdBig : 0;
  if (big(a.left[i]) && big(a.right[i])) kind |= kHdSplit;
  a.kind[i] = kind;
  a.stab[i] = 0.0;
}

__global__ void __launch_bounds__(kHdBlock) hd_head_kernel(HdArgs a) {
  const int32_t i = blockIdx.x * kHdBlock + threadIdx.x;
  if (i >= a.edges) return;
  const int32_t x = a.n + i, up = a.parent[x];
  const bool big = a.kind[i] & kHdBig;
  const bool head = big && (!hd_internal(a, up) || (a.kind[up - a.n] & kHdSplit));
  if (head) a.kind[i] |= kHdHead;
  a.head_flag[i] = head;
  a.jump[i] = big && !head ? up : x;
}

__global__ void __launch_bounds__(kHdBlock) hd_jump_kernel(HdArgs a) {
  const int32_t i = blockIdx.x * kHdBlock + threadIdx.x;
  if (i >= a.edges) return;
  const int32_t x = a.n + i;
  int32_t r = hd_load(a.jump + i);
  if (r == x) return;
#pragma unroll 1
  for (int step = 0; step < kHdJumpSteps; step++) {
    const int32_t up = hd_load(a.jump + (r - a.n));  // (r: an internal node, hd_head_kernel put nothing else here)
    if (up == r) break;
    r = up;
  }
  __hip_atomic_store(a.jump + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kHdBlock) hd_points_kernel(HdArgs a) {
  const int32_t p = blockIdx.x * kHdBlock + threadIdx.x;
  if (p >= a.n) return;
  int32_t x = a.parent[p];
#pragma unroll 1
  for (int32_t step = 0; step < a.mcs && hd_internal(a, x) && !(a.kind[x - a.n] & kHdBig); step++) x = a.parent[x];
  if (!hd_internal(a, x) || !(a.kind[x - a.n] & kHdBig)) x = -1;
  a.a[p] = x;
  if (a.lambda) a.lambda[p] = x >= 0 ? hd_lambda(a, x) : 0.0;
}

// one thread per node: the points first, then the internal nodes (the splits among them)
__global__ void __launch_bounds__(kHdBlock) hd_stability_kernel(HdArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kHdBlock + threadIdx.x;
  bool has = false;
  int32_t head = 0;
  double term = 0.0;
  if (t < a.n) {
    const int32_t x = a.a[t];
    if (x >= 0) {
      head = a.jump[x - a.n];
      term = hd_lambda(a, x) - hd_birth(a, head);
      has = true;
    }
  } else if (t < (int64_t)a.n + a.edges) {
    const int32_t i = (int32_t)(t - a.n);
    if ((a.kind[i] & (kHdBig | kHdSplit)) == (kHdBig | kHdSplit)) {
      head = a.jump[i];
      term = (double)a.size[i] * (hd_lambda(a, (int32_t)t) - hd_birth(a, head));
      has = true;
    }
  }
  hd_group_add(has, head - a.n, term, a.stab);
}

__global__ void __launch_bounds__(kHdBlock) hd_records_kernel(HdArgs a) {
  const int32_t i = blockIdx.x * kHdBlock + threadIdx.x;
  if (i >= a.edges) return;
  if (i == a.edges - 1) a.words[kHdHeads] = (unsigned long long)(a.cluster_of[i] + a.head_flag[i]);
  if (!a.head_flag[i]) return;
  const int32_t c = a.cluster_of[i], up = a.parent[a.n + i];
  a.c_stab[c] = a.stab[i];
  a.c_parent[c] = hd_internal(a, up) ? a.cluster_of[a.jump[up - a.n] - a.n] : -1;
}

__global__ void __launch_bounds__(kHdBlock) hd_raw_label_kernel(HdArgs a, int32_t clusters) {
  const int32_t p = blockIdx.x * kHdBlock + threadIdx.x;
  int32_t to = -1;
  if (p < a.n) {
    const int32_t x = a.a[p];
    if (x >= 0) {
      const int32_t head = a.jump[x - a.n];
      const int32_t c = (a.kind[head - a.n] & kHdHead) ? a.cluster_of[head - a.n] : -1;
      if (c >= 0 && c < clusters) to = a.chosen[c];
    }
    a.labels[p] = to;
  }
  hd_group_min(to >= 0, to, (uint32_t)p, a.first_row);
}

__global__ void __launch_bounds__(kHdBlock) hd_first_row_kernel(HdArgs a, int32_t clusters) {
  const int32_t c = blockIdx.x * kHdBlock + threadIdx.x;
  if (c >= clusters) return;
  const uint32_t row = a.first_row[c];
  if (row != kHdNoRow && row < (uint32_t)a.n) a.row_flag[row] = 1;
}

__global__ void __launch_bounds__(kHdBlock) hd_number_kernel(HdArgs a) {
  const int32_t p = blockIdx.x * kHdBlock + threadIdx.x;
  bool noise = false;
  if (p < a.n) {
    const int32_t to = a.labels[p];
    noise = to < 0;
    a.labels[p] = noise ? -1 : a.row_number[a.first_row[to]];
    if (p == a.n - 1) a.words[kHdClusters] = (unsigned long long)(a.row_number[p] + a.row_flag[p]);
  }
  const unsigned long long m = __ballot(noise);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.words + kHdNoise, (unsigned long long)__popcll(m));
}

// ---- the pipeline's own kernels ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kHdBlock) hd_core_kernel(const float *__restrict__ dist, int32_t k, int32_t n, float *__restrict__ core) {
  const int32_t i = blockIdx.x * kHdBlock + threadIdx.x;
  if (i < n) core[i] = dist[(size_t)i * k + (k - 1)];
}
__global__ void __launch_bounds__(kHdBlock) hd_names_kernel(LbvhView bvh, uint32_t *__restrict__ name, int32_t *__restrict__ row) {
  const int32_t t = blockIdx.x * kHdBlock + threadIdx.x;
  if (t >= bvh.n) return;
  name[t] = (uint32_t)bvh.points[t].id;
  row[t] = bvh.prim_id[t];
}
// rows[i] = the row of the point named names[i] (sorted_name ascending, sorted_row beside it), -1 for a name that is not there
__global__ void __launch_bounds__(kHdBlock) hd_rows_kernel(const int32_t *__restrict__ names, int32_t count, const uint32_t *__restrict__ sorted_name,
                                                          const int32_t *__restrict__ sorted_row, int32_t n, int32_t *__restrict__ rows) {
  const int32_t i = blockIdx.x * kHdBlock + threadIdx.x;
  if (i >= count) return;
  const uint32_t want = (uint32_t)names[i];
  int32_t lo = 0, hi = n;  // the first entry >= want
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (sorted_name[mid] < want) lo = mid + 1; else hi = mid;
  }
  rows[i] = lo < n && sorted_name[lo] == want ? sorted_row[lo] : -1;
}

struct Event {
  hipEvent_t e = nullptr;
  Event() { OWLMI_HIP(hipEventCreate(&e)); }
  ~Event() { (void)hipEventDestroy(e); }
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  void record(hipStream_t s) { OWLMI_HIP(hipEventRecord(e, s)); }
};
float between(const Event &a, const Event &b) {
  float ms = 0;
  OWLMI_HIP(hipEventElapsedTime(&ms, a.e, b.e));
  return ms;
}

// The excess-of-mass pass.  Clusters in ascending order of their heads: children before parents.  chosen[c] = the highest winning
// ancestor-or-self of c, -1 if none.  A record that names no later cluster as its parent (input that is no forest) counts as a root.
void select_clusters(const std::vector<double> &stab, std::vector<int32_t> &up, std::vector<int32_t> &chosen) {
  const int32_t count = (int32_t)stab.size();
  std::vector<double> best(count), below(count, 0.0);
  std::vector<uint8_t> has_children(count, 0), wins(count, 0);
  for (int32_t c = 0; c < count; c++) {
    if (up[c] <= c || up[c] >= count) up[c] = -1;
    wins[c] = up[c] >= 0 && (!has_children[c] || stab[c] >= below[c]);  // (a root cluster never wins)
    best[c] = has_children[c] ? std::max(stab[c], below[c]) : stab[c];
    if (up[c] >= 0) {
      below[up[c]] += best[c];
      has_children[up[c]] = 1;
    }
  }
  chosen.assign(count, -1);
  for (int32_t c = count - 1; c >= 0; c--) {
    const int32_t above = up[c] >= 0 ? chosen[up[c]] : -1;
    chosen[c] = above >= 0 ? above : wins[c] ? c : -1;
  }
}

}  // namespace

void Engine::hdbscan_labels(const tknnHdbscanLabelsOptions &o, tknnHdbscanLabelsInfo *info, hipStream_t s) {
  const int64_t n = o.n, edges = o.edges, nodes = n + edges;
  const int64_t e1 = std::max<int64_t>(edges, 1);
  size_t scan_e = 0, scan_n = 0;
  {
    int32_t *k32 = nullptr;
    OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_e, k32, k32, (int)e1, s));
    OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_n, k32, k32, (int)n, s));
  }
  // the workspace: the dendrogram's | the linkage arrays | the columns below | the scans' space
  const size_t link_b = linkage_workspace_bytes(n, edges, s), col_nodes = linkage_align((size_t)nodes * sizeof(int32_t)),
               col_e = linkage_align((size_t)e1 * sizeof(int32_t)), col_n = linkage_align((size_t)n * sizeof(int32_t)), words_b = linkage_align(kHdWords * sizeof(unsigned long long)),
               scan_b = linkage_align(std::max(scan_e, scan_n));
  char *ws = (char *)workspace(link_b + col_nodes + 3 * col_e + words_b + 8 * col_e + 2 * (2 * col_e) + 3 * col_n + scan_b);
  char *at = ws + link_b;
  auto take = [&](size_t bytes) {
    char *p = at;
    at += bytes;
    return p;
  };
  LinkageArrays tree;
  char *spare_parent = take(col_nodes), *spare_left = take(col_e), *spare_right = take(col_e), *spare_size = take(col_e);
  tree.parent = o.d_parent ? o.d_parent : (int32_t *)spare_parent;
  tree.left = o.d_left ? o.d_left : (int32_t *)spare_left;
  tree.right = o.d_right ? o.d_right : (int32_t *)spare_right;
  tree.size = o.d_size ? o.d_size : (int32_t *)spare_size;
  HdArgs a;
  std::memset(&a, 0, sizeof a);
  a.n = (int32_t)n, a.edges = (int32_t)edges, a.mcs = o.min_cluster_size;
  a.w = o.d_w;
  a.parent = tree.parent, a.left = tree.left, a.right = tree.right, a.size = tree.size;
  a.words = (unsigned long long *)take(words_b);
  a.kind = (uint8_t *)take(col_e);
  a.jump = (int32_t *)take(col_e);
  a.head_flag = (int32_t *)take(col_e);
  a.cluster_of = (int32_t *)take(col_e);
  a.c_parent = (int32_t *)take(col_e);
  a.chosen = (int32_t *)take(col_e);
  a.first_row = (uint32_t *)take(col_e);
  take(col_e);  // (spare)
  char *spare_stab = take(2 * col_e);
  a.stab = o.d_stability ? o.d_stability : (double *)spare_stab;
  a.c_stab = (double *)take(2 * col_e);
  a.a = (int32_t *)take(col_n);
  a.row_flag = (int32_t *)take(col_n);
  a.row_number = (int32_t *)take(col_n);
  void *scan_tmp = take(scan_b);
  a.labels = o.d_labels;
  a.lambda = o.d_lambda;

  const dim3 block(kHdBlock);
  auto grid = [](int64_t items) { return dim3((unsigned)((std::max<int64_t>(items, 1) + kHdBlock - 1) / kHdBlock)); };
  Event t0, t1, t2, t3, t4;
  t0.record(s);
  const LinkageRun run = linkage_run(ws, n, edges, o.d_u, o.d_v, tree, o.max_rounds, h_counters_, s);
  t1.record(s);

  // the condensed tree
  OWLMI_HIP(hipMemsetAsync(a.words, 0, kHdWords * sizeof(unsigned long long), s));
  int64_t clusters = 0;
  if (edges > 0) {
    hipLaunchKernelGGL(hd_kind_kernel, grid(edges), block, 0, s, a);
    hipLaunchKernelGGL(hd_head_kernel, grid(edges), block, 0, s, a);
    for (int p = 0, passes = jump_passes(edges); p < passes; p++) hipLaunchKernelGGL(hd_jump_kernel, grid(edges), block, 0, s, a);
  }
  hipLaunchKernelGGL(hd_points_kernel, grid(n), block, 0, s, a);
  if (edges > 0) {
    hipLaunchKernelGGL(hd_stability_kernel, grid(nodes), block, 0, s, a);
    OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_e, a.head_flag, a.cluster_of, (int)edges, s));
    hipLaunchKernelGGL(hd_records_kernel, grid(edges), block, 0, s, a);
  }
  OWLMI_HIP(hipGetLastError());
  t2.record(s);

  // the selection, on the host: one record per cluster
  if (edges > 0) {
    OWLMI_HIP(hipMemcpyAsync(h_counters_, a.words, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
    clusters = std::min<int64_t>((int64_t)h_counters_[kHdHeads], edges);
  }
  if (clusters > 0) {
    std::vector<double> stab((size_t)clusters);
    std::vector<int32_t> up((size_t)clusters), chosen;
    OWLMI_HIP(hipMemcpyAsync(stab.data(), a.c_stab, (size_t)clusters * sizeof(double), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipMemcpyAsync(up.data(), a.c_parent, (size_t)clusters * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
    select_clusters(stab, up, chosen);
    OWLMI_HIP(hipMemcpyAsync(a.chosen, chosen.data(), (size_t)clusters * sizeof(int32_t), hipMemcpyHostToDevice, s));
    OWLMI_HIP(hipStreamSynchronize(s));  // (chosen is freed on return from this block)
  }
  t3.record(s);

  // labels, numbered by their smallest row
  OWLMI_HIP(hipMemsetAsync(a.first_row, 0xff, (size_t)e1 * sizeof(uint32_t), s));
  OWLMI_HIP(hipMemsetAsync(a.row_flag, 0, (size_t)n * sizeof(int32_t), s));
  hipLaunchKernelGGL(hd_raw_label_kernel, grid(n), block, 0, s, a, (int32_t)clusters);
  if (clusters > 0) hipLaunchKernelGGL(hd_first_row_kernel, grid(clusters), block, 0, s, a, (int32_t)clusters);
  OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_n, a.row_flag, a.row_number, (int)n, s));
  hipLaunchKernelGGL(hd_number_kernel, grid(n), block, 0, s, a);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipMemcpyAsync(h_counters_, a.words, kHdWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  t4.record(s);
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->clusters = (int64_t)h_counters_[kHdClusters];
    info->noise = (int64_t)h_counters_[kHdNoise];
    info->condensed_clusters = clusters;
    info->absorbed = run.absorbed;
    info->host_edges = run.host_edges;
    info->rounds = run.rounds;
    info->solve_ms = between(t0, t4);
    info->linkage_ms = between(t0, t1);
    info->condense_ms = between(t1, t2);
    info->select_ms = between(t2, t3);
    info->label_ms = between(t3, t4);
  }
}

void Engine::hdbscan(const tknnHdbscanOptions &o, tknnHdbscanInfo *info, hipStream_t s) {
  const LbvhView tv = bvh_.view();
  const int64_t n = tv.n, rows = std::max<int64_t>(n - 1, 1);
  const int k = o.min_samples - 1;
  const dim3 block(kHdBlock);
  auto grid = [](int64_t items) { return dim3((unsigned)((std::max<int64_t>(items, 1) + kHdBlock - 1) / kHdBlock)); };
  Event t0, t1;
  t0.record(s);

  // the core distances: the last column of the own points' kNN rows.  (The calls inside take the engine's workspace, so what
  // must outlive them is allocated for the length of this call.)
  tknnKnnInfo knn_info;
  std::memset(&knn_info, 0, sizeof knn_info);
  DeviceBuffer own_core(o.d_core_dist || k == 0 ? 0 : (size_t)n * sizeof(float));
  float *core = k == 0 ? nullptr : o.d_core_dist ? o.d_core_dist : (float *)own_core.p;
  if (k > 0) {
    DeviceBuffer idx((size_t)n * k * sizeof(int32_t)), dist((size_t)n * k * sizeof(float));
    tknnKnnOptions ko;
    std::memset(&ko, 0, sizeof ko);
    ko.m = n, ko.k = k;
    ko.d_idx = (int32_t *)idx.p, ko.d_dist = (float *)dist.p;
    knn(ko, &knn_info, s);
    hipLaunchKernelGGL(hd_core_kernel, grid(n), block, 0, s, (const float *)dist.p, (int32_t)k, (int32_t)n, core);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipStreamSynchronize(s));  // (the rows are freed here)
  }

  // the tree under them
  DeviceBuffer own_u(o.d_u ? 0 : (size_t)rows * sizeof(int32_t)), own_v(o.d_v ? 0 : (size_t)rows * sizeof(int32_t)), own_w(o.d_w ? 0 : (size_t)rows * sizeof(float));
  tknnEmstOptions eo;
  std::memset(&eo, 0, sizeof eo);
  eo.d_core_dist = core;
  eo.d_u = o.d_u ? o.d_u : (int32_t *)own_u.p;
  eo.d_v = o.d_v ? o.d_v : (int32_t *)own_v.p;
  eo.d_w = o.d_w ? o.d_w : (float *)own_w.p;
  tknnEmstInfo emst_info;
  std::memset(&emst_info, 0, sizeof emst_info);
  emst(eo, &emst_info, s);
  const int64_t edges = emst_info.edges;

  // the records name their points; the dendrogram's leaves are rows
  const int32_t *row_u = eo.d_u, *row_v = eo.d_v;
  DeviceBuffer rows_u(ids_given_ ? (size_t)rows * sizeof(int32_t) : 0), rows_v(ids_given_ ? (size_t)rows * sizeof(int32_t) : 0);
  if (ids_given_ && edges > 0) {
    size_t sort_bytes = 0;
    uint32_t *k32 = nullptr;
    int32_t *v32 = nullptr;
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, k32, k32, v32, v32, (int)n, 0, 32, s));
    const size_t col = linkage_align((size_t)n * sizeof(int32_t));
    char *ws = (char *)workspace(4 * col + sort_bytes);
    uint32_t *name = (uint32_t *)ws, *sorted_name = (uint32_t *)(ws + col);
    int32_t *row = (int32_t *)(ws + 2 * col), *sorted_row = (int32_t *)(ws + 3 * col);
    hipLaunchKernelGGL(hd_names_kernel, grid(n), block, 0, s, tv, name, row);
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(ws + 4 * col, sort_bytes, name, sorted_name, row, sorted_row, (int)n, 0, 32, s));
    hipLaunchKernelGGL(hd_rows_kernel, grid(edges), block, 0, s, (const int32_t *)eo.d_u, (int32_t)edges, (const uint32_t *)sorted_name, (const int32_t *)sorted_row, (int32_t)n,
                       (int32_t *)rows_u.p);
    hipLaunchKernelGGL(hd_rows_kernel, grid(edges), block, 0, s, (const int32_t *)eo.d_v, (int32_t)edges, (const uint32_t *)sorted_name, (const int32_t *)sorted_row, (int32_t)n,
                       (int32_t *)rows_v.p);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipStreamSynchronize(s));  // (the next call takes the workspace)
    row_u = (const int32_t *)rows_u.p, row_v = (const int32_t *)rows_v.p;
  }

  tknnHdbscanLabelsOptions lo;
  std::memset(&lo, 0, sizeof lo);
  lo.n = n, lo.edges = edges;
  lo.d_u = row_u, lo.d_v = row_v, lo.d_w = eo.d_w;
  lo.min_cluster_size = o.min_cluster_size, lo.max_rounds = o.max_rounds;
  lo.d_labels = o.d_labels;
  lo.d_parent = o.d_parent, lo.d_left = o.d_left, lo.d_right = o.d_right, lo.d_size = o.d_size;
  lo.d_lambda = o.d_lambda, lo.d_stability = o.d_stability;
  tknnHdbscanLabelsInfo labels_info;
  std::memset(&labels_info, 0, sizeof labels_info);
  // d_stability holds n - 1 entries here and is no linkage array: the entries behind the records head no cluster, which is a 0
  // (tknnHdbscanLabels writes the first `edges` of them)
  if (o.d_stability && edges < n - 1) {
    OWLMI_HIP(hipMemsetAsync(o.d_stability + edges, 0, (size_t)(n - 1 - edges) * sizeof(double), s));
  }
  hdbscan_labels(lo, &labels_info, s);
  t1.record(s);
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->labels = labels_info;
    info->labels.solve_ms = between(t0, t1);
    info->edges = edges;
    info->excluded = emst_info.excluded;
    info->knn_ms = knn_info.solve_ms;
    info->emst_ms = emst_info.solve_ms;
  }
}

}  // namespace owlmi
