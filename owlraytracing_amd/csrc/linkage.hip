// linkage.hip -- the single-linkage dendrogram of a sorted forest (tknnLinkage, include/owlknn_hdbscan.h) in contraction rounds.
// tests/hdbscan_spec.py contraction() restates this file in numpy, step for step, next to the sequential union-find it must equal.
//
// Record i has rank i.  State: sv[vertex] its supervertex (a vertex id), top[c] / ssize[c] of a supervertex c the dendrogram node
// of its latest merge (or the leaf itself) and its leaves, alive[record].  Invariant: a supervertex is a Kruskal cluster -- its
// inner records all rank below its top, every record that leaves it ranks above.  One round:
//   1. lk_min_kernel:       m[c] = the smallest alive rank at supervertex c.  A record is SELECTED if it is m of one of its ends.
//   2. lk_point_kernel:     c points to the other end of m[c]; ranks fall strictly along the pointers until a mutual pair, whose
//                           smaller id is the root.  lk_jump_kernel, launched jump_passes(n) times: g[c] = the root reached, the
//                           GROUP of c.  The selected records of a group are a tree with ranks rising away from the root record.
//   3. lk_threshold_kernel: T[g] = the smallest rank of an alive record that is NOT selected and has an end in group g.
//   4. lk_absorb_kernel:    the selected records below their group's T are absorbed: they are the next merges of Kruskal's
//                           algorithm in that group, a chain in rank order -- the root record joins two supervertices, each later
//                           one attaches the one supervertex that chose it to all that was absorbed before.  Their keys
//                           (group, rank) are sorted; lk_contrib_kernel and a segmented sum give size[], lk_link_kernel the
//                           parents: of the tops of the supervertices that chose the record, and of the record before it.
//   5. lk_tops_kernel, lk_relabel_kernel: the supervertices whose record was absorbed become their group, whose top and size are
//                           the chain's last record's.
// The root record of every group is absorbed, so every round makes progress; the host reads two words per round (absorbed, still
// alive).  A record whose ends lie in one supervertex (input that is no forest) dies in step 1.  After max_rounds rounds the alive
// records go to the host, where a sequential union-find over the supervertices finishes them (lk_gather_kernel, finish_on_host,
// lk_scatter_kernel).  Left and right children come from one pass over the parents at the end (lk_children_kernel).
// What a kernel reads was written by an earlier launch, except in lk_jump_kernel, which reads pointers other workgroups move
// forward meanwhile: every value a pointer ever holds is an ancestor in the same tree, so a stale one costs a step, no more;
// those loads and stores are relaxed atomics of agent scope.  No loop waits for another thread, every loop has a step count.
#include "linkage.h"
#include "trueknn_engine.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <unordered_map>
#include <vector>

namespace owlmi {

namespace {

constexpr int kLkBlock = 256;
constexpr uint32_t kLkNone = 0xffffffffu;
constexpr int kLkJumpSteps = 16;
// the call's words: [0] records absorbed this round (= keys appended), [1] records still alive, [2] roots, [3] records gathered
constexpr int kLkAbsorbed = 0, kLkAlive = 1, kLkRoots = 2, kLkGathered = 3, kLkWords = 4;

struct LkArgs {
  int32_t n, edges;
  const int32_t *u, *v;
  int32_t *sv, *top, *ssize;  // per vertex id
  uint32_t *m, *T;            // per vertex id, reset every round
  int32_t *g;                 // per vertex id: the pointer, then the group
  uint8_t *alive;             // per record
  unsigned long long *key;    // the absorbed records of the round: (group << 32) | rank, sorted
  int32_t *gkey, *contrib, *seg;  // per sorted key: its group, the leaves it adds, the leaves below its node
  LinkageArrays out;
  unsigned long long *words;
};

// one record of what the rounds left, for the host
struct LkRecord {
  int32_t e, a, b, top_a, size_a, top_b, size_b;
};

__device__ __forceinline__ uint32_t lk_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// table[at] = min(table[at], e), without the atomic when a load shows that it would change nothing: a supervertex of many records
// (a star) would queue them all at one word, and the threads come in ascending rank
__device__ __forceinline__ void lk_min(uint32_t *table, int32_t at, uint32_t e) {
  if (lk_load(table + at) > e) atomicMin(table + at, e);
}

// adds the lanes with `has` to words[which]: one atomic per wave
__device__ __forceinline__ unsigned long long lk_count(bool has, unsigned long long *word, int &rank_in_wave) {
  const unsigned long long mask = __ballot(has);
  const int lane = threadIdx.x & 63;
  rank_in_wave = __popcll(mask & ((1ull << lane) - 1ull));
  if (!mask) return 0;
  const int first = __ffsll((long long)mask) - 1;
  unsigned long long base = 0;
  if (lane == first) base = atomicAdd(word, (unsigned long long)__popcll(mask));
  return __shfl(base, first);
}

__global__ void __launch_bounds__(kLkBlock) lk_init_kernel(LkArgs a) {
  const int64_t t = (int64_t)blockIdx.x * kLkBlock + threadIdx.x;
  if (t < a.n) {
    a.sv[t] = (int32_t)t;
    a.top[t] = (int32_t)t;
    a.ssize[t] = 1;
  }
  if (t < (int64_t)a.n + a.edges) a.out.parent[t] = -1;
  if (t < a.edges) {
    const int32_t x = a.u[t], y = a.v[t];
    a.alive[t] = x >= 0 && x < a.n && y >= 0 && y < a.n && x != y;  // (a record out of range takes no part)
    a.out.left[t] = 0x7fffffff;
    a.out.right[t] = -1;
    a.out.size[t] = 0;
  }
}

// ---- 1. the smallest alive rank at every supervertex ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kLkBlock) lk_min_kernel(LkArgs a) {
  const int32_t e = blockIdx.x * kLkBlock + threadIdx.x;
  if (e >= a.edges || !a.alive[e]) return;
  const int32_t ca = a.sv[a.u[e]], cb = a.sv[a.v[e]];
  if (ca == cb) {  // (no forest: a record inside a supervertex)
    a.alive[e] = 0;
    return;
  }
  lk_min(a.m, ca, (uint32_t)e);
  lk_min(a.m, cb, (uint32_t)e);
}

// ---- 2. pointers and groups ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLkBlock) lk_point_kernel(LkArgs a) {
  const int32_t c = blockIdx.x * kLkBlock + threadIdx.x;
  if (c >= a.n) return;
  const uint32_t e = a.m[c];
  int32_t to = c;
  if (e != kLkNone) {
    const int32_t ca = a.sv[a.u[e]], cb = a.sv[a.v[e]];
    const int32_t other = ca == c ? cb : ca;
    to = a.m[other] == e && c < other ? c : other;  // of a mutual pair the smaller id is the root
  }
  a.g[c] = to;
}

__global__ void __launch_bounds__(kLkBlock) lk_jump_kernel(LkArgs a) {
  const int32_t c = blockIdx.x * kLkBlock + threadIdx.x;
  if (c >= a.n) return;
  uint32_t *g = (uint32_t *)a.g;
  int32_t r = (int32_t)lk_load(g + c);
  if (r == c) return;
#pragma unroll 1
  for (int step = 0; step < kLkJumpSteps; step++) {
    const int32_t up = (int32_t)lk_load(g + r);
    if (up == r) break;
    r = up;
  }
  __hip_atomic_store(g + c, (uint32_t)r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 3. the smallest record that leaves a group ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLkBlock) lk_threshold_kernel(LkArgs a) {
  const int32_t e = blockIdx.x * kLkBlock + threadIdx.x;
  if (e >= a.edges || !a.alive[e]) return;
  const int32_t ca = a.sv[a.u[e]], cb = a.sv[a.v[e]];
  if (a.m[ca] == (uint32_t)e || a.m[cb] == (uint32_t)e) return;  // selected
  lk_min(a.T, a.g[ca], (uint32_t)e);
  lk_min(a.T, a.g[cb], (uint32_t)e);
}

// ---- 4. the absorbed records ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLkBlock) lk_absorb_kernel(LkArgs a) {
  const int32_t e = blockIdx.x * kLkBlock + threadIdx.x;
  const bool alive = e < a.edges && a.alive[e];
  bool take = false;
  int32_t group = 0;
  if (alive) {
    const int32_t ca = a.sv[a.u[e]], cb = a.sv[a.v[e]];
    group = a.g[ca];  // (a selected record's ends are in one group)
    take = (a.m[ca] == (uint32_t)e || a.m[cb] == (uint32_t)e) && (uint32_t)e < a.T[group];
  }
  int rank;
  const unsigned long long base = lk_count(take, a.words + kLkAbsorbed, rank);
  if (take) {
    const unsigned long long at = base + rank;
    if (at < (unsigned long long)a.edges) a.key[at] = ((unsigned long long)(uint32_t)group << 32) | (uint32_t)e;  // (never false)
    a.alive[e] = 0;
  }
  int unused;
  lk_count(alive && !take, a.words + kLkAlive, unused);
}

struct LkSorted {
  int32_t e, group, ca, cb;
  bool chose_a, chose_b;
};
__device__ __forceinline__ LkSorted lk_sorted(const LkArgs &a, int32_t i) {
  LkSorted r;
  const unsigned long long key = a.key[i];
  r.e = (int32_t)(uint32_t)key;
  r.group = (int32_t)(uint32_t)(key >> 32);
  r.ca = a.sv[a.u[r.e]];
  r.cb = a.sv[a.v[r.e]];
  r.chose_a = a.m[r.ca] == (uint32_t)r.e;
  r.chose_b = a.m[r.cb] == (uint32_t)r.e;
  return r;
}

__global__ void __launch_bounds__(kLkBlock) lk_contrib_kernel(LkArgs a, int32_t count) {
  const int32_t i = blockIdx.x * kLkBlock + threadIdx.x;
  if (i >= count) return;
  const LkSorted r = lk_sorted(a, i);
  a.gkey[i] = r.group;
  a.contrib[i] = (r.chose_a ? a.ssize[r.ca] : 0) + (r.chose_b ? a.ssize[r.cb] : 0);
}

__global__ void __launch_bounds__(kLkBlock) lk_link_kernel(LkArgs a, int32_t count) {
  const int32_t i = blockIdx.x * kLkBlock + threadIdx.x;
  if (i >= count) return;
  const LkSorted r = lk_sorted(a, i);
  const int32_t node = a.n + r.e;
  a.out.size[r.e] = a.seg[i];
  if (r.chose_a) a.out.parent[a.top[r.ca]] = node;
  if (r.chose_b) a.out.parent[a.top[r.cb]] = node;
  if (i > 0 && a.gkey[i - 1] == r.group) a.out.parent[a.n + (int32_t)(uint32_t)a.key[i - 1]] = node;
}

// ---- 5. the new supervertices ----------------------------------------------------------------------------------------------------
// (a launch of its own: lk_link_kernel reads the tops this one writes)
__global__ void __launch_bounds__(kLkBlock) lk_tops_kernel(LkArgs a, int32_t count) {
  const int32_t i = blockIdx.x * kLkBlock + threadIdx.x;
  if (i >= count) return;
  const int32_t group = a.gkey[i];
  if (i + 1 < count && a.gkey[i + 1] == group) return;
  a.top[group] = a.n + (int32_t)(uint32_t)a.key[i];
  a.ssize[group] = a.seg[i];
}

__global__ void __launch_bounds__(kLkBlock) lk_relabel_kernel(LkArgs a) {
  const int32_t t = blockIdx.x * kLkBlock + threadIdx.x;
  if (t >= a.n) return;
  const int32_t c = a.sv[t];
  const uint32_t e = a.m[c];
  if (e != kLkNone && !a.alive[e]) a.sv[t] = a.g[c];
}

// ---- what max_rounds rounds left ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLkBlock) lk_gather_kernel(LkArgs a, LkRecord *records, int32_t capacity) {
  const int32_t e = blockIdx.x * kLkBlock + threadIdx.x;
  const bool alive = e < a.edges && a.alive[e];
  int rank;
  const unsigned long long base = lk_count(alive, a.words + kLkGathered, rank);
  if (!alive || base + rank >= (unsigned long long)capacity) return;
  const int32_t ca = a.sv[a.u[e]], cb = a.sv[a.v[e]];
  records[base + rank] = LkRecord{e, ca, cb, a.top[ca], a.ssize[ca], a.top[cb], a.ssize[cb]};
}

// table[at[i]] = value[i]; `limit`: the table's length
__global__ void __launch_bounds__(kLkBlock) lk_scatter_kernel(const int32_t *__restrict__ at, const int32_t *__restrict__ value, int32_t count, int32_t *table,
                                                             int32_t limit) {
  const int32_t i = blockIdx.x * kLkBlock + threadIdx.x;
  if (i < count && at[i] >= 0 && at[i] < limit) table[at[i]] = value[i];
}

// ---- after the rounds ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kLkBlock) lk_children_kernel(LkArgs a) {
  const int64_t x = (int64_t)blockIdx.x * kLkBlock + threadIdx.x;
  const bool in = x < (int64_t)a.n + a.edges;
  const int32_t p = in ? a.out.parent[x] : 0;
  if (in && p >= a.n && p < a.n + a.edges) {
    atomicMin(a.out.left + (p - a.n), (int32_t)x);
    atomicMax(a.out.right + (p - a.n), (int32_t)x);
  }
  int unused;
  lk_count(in && p < 0, a.words + kLkRoots, unused);
}

struct LkLayout {
  size_t words, col_n, col_e, col_nodes, wide_e, sort_bytes, scan_bytes, total;
  LkLayout(int64_t n, int64_t edges, hipStream_t s) {
    unsigned long long *k64 = nullptr;
    int32_t *k32 = nullptr;
    sort_bytes = scan_bytes = 0;
    const int items = (int)std::max<int64_t>(edges, 1);
    OWLMI_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, k64, k64, items, 0, 64, s));
    OWLMI_HIP(hipcub::DeviceScan::InclusiveSumByKey(nullptr, scan_bytes, k32, k32, k32, items, hipcub::Equality(), s));
    words = linkage_align(kLkWords * sizeof(unsigned long long));
    col_n = linkage_align((size_t)n * sizeof(int32_t));
    col_e = linkage_align((size_t)std::max<int64_t>(edges, 1) * sizeof(int32_t));
    col_nodes = linkage_align((size_t)(n + edges) * sizeof(int32_t));
    wide_e = 2 * col_e;
    // words | sv top ssize m T g | gkey contrib seg alive | key key_alt | the sort's and the scan's space
    total = words + 6 * col_n + 4 * col_e + 2 * wide_e + linkage_align(std::max(sort_bytes, scan_bytes));
  }
};

// Kruskal over the records the rounds left, on the supervertices: the parents of the tops and the sizes, as scatter lists
void finish_on_host(std::vector<LkRecord> &records, int32_t n, std::vector<int32_t> &parent_at, std::vector<int32_t> &parent_value, std::vector<int32_t> &size_at,
                    std::vector<int32_t> &size_value) {
  std::sort(records.begin(), records.end(), [](const LkRecord &x, const LkRecord &y) { return x.e < y.e; });
  struct Super {
    int32_t up, top, size;
  };
  std::unordered_map<int32_t, Super> uf;
  uf.reserve(records.size() * 2);
  for (const LkRecord &r : records) {
    uf.emplace(r.a, Super{r.a, r.top_a, r.size_a});
    uf.emplace(r.b, Super{r.b, r.top_b, r.size_b});
  }
  auto find = [&](int32_t x) {
    int32_t root = x;
    for (size_t step = 0; step <= uf.size() && uf[root].up != root; step++) root = uf[root].up;
    for (size_t step = 0; step <= uf.size() && uf[x].up != root && x != root; step++) {  // path compression
      const int32_t next = uf[x].up;
      uf[x].up = root;
      x = next;
    }
    return root;
  };
  for (const LkRecord &r : records) {
    const int32_t a = find(r.a), b = find(r.b);
    if (a == b) continue;  // (no forest)
    Super &sa = uf[a], &sb = uf[b];
    const int32_t node = n + r.e, size = sa.size + sb.size;
    parent_at.push_back(sa.top), parent_value.push_back(node);
    parent_at.push_back(sb.top), parent_value.push_back(node);
    size_at.push_back(r.e), size_value.push_back(size);
    Super &root = a < b ? sa : sb, &child = a < b ? sb : sa;
    child.up = a < b ? a : b;
    root.top = node;
    root.size = size;
  }
}

void scatter(const std::vector<int32_t> &at, const std::vector<int32_t> &value, int32_t *table, int32_t limit, hipStream_t s) {
  if (at.empty()) return;
  const size_t bytes = at.size() * sizeof(int32_t);
  DeviceBuffer d_at(bytes), d_value(bytes);
  OWLMI_HIP(hipMemcpyAsync(d_at.p, at.data(), bytes, hipMemcpyHostToDevice, s));
  OWLMI_HIP(hipMemcpyAsync(d_value.p, value.data(), bytes, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(lk_scatter_kernel, dim3((unsigned)((at.size() + kLkBlock - 1) / kLkBlock)), dim3(kLkBlock), 0, s, (const int32_t *)d_at.p,
                     (const int32_t *)d_value.p, (int32_t)at.size(), table, limit);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipStreamSynchronize(s));  // (the buffers are freed on return)
}

}  // namespace

size_t linkage_workspace_bytes(int64_t n, int64_t edges, hipStream_t s) { return LkLayout(n, edges, s).total; }

LinkageRun linkage_run(char *ws, int64_t n, int64_t edges, const int32_t *d_u, const int32_t *d_v, const LinkageArrays &out, int max_rounds,
                       unsigned long long *h, hipStream_t s) {
  const LkLayout lay(n, edges, s);
  LkArgs a;
  a.n = (int32_t)n;
  a.edges = (int32_t)edges;
  a.u = d_u;
  a.v = d_v;
  a.out = out;
  char *at = ws;
  auto take = [&](size_t bytes) {
    char *p = at;
    at += bytes;
    return p;
  };
  a.words = (unsigned long long *)take(lay.words);
  a.sv = (int32_t *)take(lay.col_n);
  a.top = (int32_t *)take(lay.col_n);
  a.ssize = (int32_t *)take(lay.col_n);
  a.m = (uint32_t *)take(lay.col_n);
  a.T = (uint32_t *)take(lay.col_n);  // (behind m: one memset resets both)
  a.g = (int32_t *)take(lay.col_n);
  a.gkey = (int32_t *)take(lay.col_e);
  a.contrib = (int32_t *)take(lay.col_e);
  a.seg = (int32_t *)take(lay.col_e);
  a.alive = (uint8_t *)take(lay.col_e);
  unsigned long long *key_in = (unsigned long long *)take(lay.wide_e);
  a.key = (unsigned long long *)take(lay.wide_e);
  void *tmp = take(linkage_align(std::max(lay.sort_bytes, lay.scan_bytes)));
  size_t sort_bytes = lay.sort_bytes, scan_bytes = lay.scan_bytes;

  const dim3 block(kLkBlock);
  auto grid = [](int64_t items) { return dim3((unsigned)((std::max<int64_t>(items, 1) + kLkBlock - 1) / kLkBlock)); };
  auto read_words = [&]() {
    OWLMI_HIP(hipMemcpyAsync(h, a.words, kLkWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
  };
  int key_bits = 1;
  while ((1ll << key_bits) < n) key_bits++;
  const int passes = jump_passes(n);
  if (max_rounds <= 0) max_rounds = 64;

  LinkageRun run;
  OWLMI_HIP(hipMemsetAsync(a.words, 0, kLkWords * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(lk_init_kernel, grid(n + edges), block, 0, s, a);
  OWLMI_HIP(hipGetLastError());
  int64_t alive = edges;
  while (alive > 0 && run.rounds < max_rounds) {
    OWLMI_HIP(hipMemsetAsync(a.words, 0, 2 * sizeof(unsigned long long), s));
    OWLMI_HIP(hipMemsetAsync(a.m, 0xff, 2 * lay.col_n, s));
    // the absorbed keys are appended to key_in and sorted into a.key
    LkArgs append = a;
    append.key = key_in;
    hipLaunchKernelGGL(lk_min_kernel, grid(edges), block, 0, s, a);
    hipLaunchKernelGGL(lk_point_kernel, grid(n), block, 0, s, a);
    for (int p = 0; p < passes; p++) hipLaunchKernelGGL(lk_jump_kernel, grid(n), block, 0, s, a);
    hipLaunchKernelGGL(lk_threshold_kernel, grid(edges), block, 0, s, a);
    hipLaunchKernelGGL(lk_absorb_kernel, grid(edges), block, 0, s, append);
    OWLMI_HIP(hipGetLastError());
    read_words();
    const int64_t count = std::min<int64_t>((int64_t)h[kLkAbsorbed], edges);
    alive = (int64_t)h[kLkAlive];
    run.rounds++;
    run.absorbed += count;
    if (count == 0) continue;  // (records inside a supervertex died; nothing to link)
    OWLMI_HIP(hipcub::DeviceRadixSort::SortKeys(tmp, sort_bytes, key_in, a.key, (int)count, 0, 32 + key_bits, s));
    hipLaunchKernelGGL(lk_contrib_kernel, grid(count), block, 0, s, a, (int32_t)count);
    OWLMI_HIP(hipcub::DeviceScan::InclusiveSumByKey(tmp, scan_bytes, a.gkey, a.contrib, a.seg, (int)count, hipcub::Equality(), s));
    hipLaunchKernelGGL(lk_link_kernel, grid(count), block, 0, s, a, (int32_t)count);
    hipLaunchKernelGGL(lk_tops_kernel, grid(count), block, 0, s, a, (int32_t)count);
    hipLaunchKernelGGL(lk_relabel_kernel, grid(n), block, 0, s, a);
    OWLMI_HIP(hipGetLastError());
  }
  if (alive > 0) {  // max_rounds rounds were not enough: the rest on the host
    DeviceBuffer d_records((size_t)alive * sizeof(LkRecord));
    hipLaunchKernelGGL(lk_gather_kernel, grid(edges), block, 0, s, a, (LkRecord *)d_records.p, (int32_t)alive);
    OWLMI_HIP(hipGetLastError());
    read_words();
    std::vector<LkRecord> records((size_t)std::min<int64_t>((int64_t)h[kLkGathered], alive));
    OWLMI_HIP(hipMemcpyAsync(records.data(), d_records.p, records.size() * sizeof(LkRecord), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
    std::vector<int32_t> parent_at, parent_value, size_at, size_value;
    finish_on_host(records, a.n, parent_at, parent_value, size_at, size_value);
    scatter(parent_at, parent_value, out.parent, (int32_t)(n + edges), s);
    scatter(size_at, size_value, out.size, (int32_t)edges, s);
    run.host_edges = (int64_t)records.size();
  }
  hipLaunchKernelGGL(lk_children_kernel, grid(n + edges), block, 0, s, a);
  OWLMI_HIP(hipGetLastError());
  read_words();
  run.roots = (int64_t)h[kLkRoots];
  return run;
}

void Engine::linkage(const tknnLinkageOptions &o, tknnLinkageInfo *info, hipStream_t s) {
  const int64_t n = o.n, edges = o.edges, nodes = n + edges;
  // what the caller does not want lies behind the solve's own workspace
  const size_t own = linkage_workspace_bytes(n, edges, s), col_nodes = linkage_align((size_t)nodes * sizeof(int32_t)),
               col_e = linkage_align((size_t)std::max<int64_t>(edges, 1) * sizeof(int32_t));
  char *ws = (char *)workspace(own + col_nodes + 3 * col_e);
  char *spare = ws + own;
  LinkageArrays out;
  out.parent = o.d_parent ? o.d_parent : (int32_t *)spare;
  out.left = o.d_left ? o.d_left : (int32_t *)(spare + col_nodes);
  out.right = o.d_right ? o.d_right : (int32_t *)(spare + col_nodes + col_e);
  out.size = o.d_size ? o.d_size : (int32_t *)(spare + col_nodes + 2 * col_e);
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  const LinkageRun run = linkage_run(ws, n, edges, o.d_u, o.d_v, out, o.max_rounds, h_counters_, s);
  OWLMI_HIP(hipEventRecord(ev_f_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->rounds = run.rounds;
    info->absorbed = run.absorbed;
    info->host_edges = run.host_edges;
    info->roots = run.roots;
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_f_));
  }
}

}  // namespace owlmi
