// emst.hip -- the minimum spanning forest of the tree's own points under the Euclidean or the mutual-reachability distance
// (tknnEmst, include/owlknn_emst.h), in Boruvka rounds over the curve-ordered LBVH.
//
// Edges are ordered by the strict key (bits of the fp32 weight, min name, max name), so the forest is unique and every choice
// below is a minimum under that key -- never under the weight alone.  A component is a set of the union-find over SORTED SLOTS
// (uf_find / uf_unite, db_device.h: the smaller slot stays root), named by its root; comp[slot] holds it between rounds, -1 for a
// point that is not eligible.  One round, every kernel one thread per slot, so that a wave's lanes are curve neighbours:
//   1. em_uniform_kernel: node_comp[node] = the component if every eligible point below the node is in it.  Every slot climbs
//      along split_owner; at a parent the first child to arrive leaves its value there and stops, the second combines both and
//      goes on (db_uniform_kernel's arrival, here from the leaves and with a value for "mixed", so both always arrive).
//   2. em_walk_kernel: a lane's nearest point in ANOTHER component, by the full key.  Its bound starts from the other fifteen
//      points of its block of 16 (real candidates, as knn_seed.hip's window) and from the best weight its component has so far
//      (one relaxed load); the walk climbs from the lane's leaf and at every ancestor walks the other child's subtree, near parts
//      of the tree first; it steps over a node that lies wholly in the lane's own component, that holds no eligible
//      point, or whose lower bound -- sqrt of the box distance, raised to the lane's core distance -- EXCEEDS the bound: a node
//      that can hold an equal weight is walked, a smaller pair of names may be in it.  The lane's weight then goes into its
//      component's minimum (em_group_min: lanes of one component reduce inside the wave first, and the atomic is left out when
//      a plain load shows a value that is not larger).
//   3. em_pair_kernel: the key has 94 bits; among the lanes whose weight is the component's minimum, the minimum of
//      (min name << 32) | max name.
//   4. em_merge_kernel: the one lane whose (weight, pair) is its component's runs uf_unite and appends the edge -- when the
//      other component chose the same edge, the lane that holds the smaller name does.
//   5. em_relabel_kernel: comp[slot] = uf_find, and the components' minima reset.
// The host reads one record per round (eligible points, edges so far) and stops when a round added nothing or one component is
// left; at most ceil(log2 n) + 1 rounds are run (every component with an outgoing edge merges in a round: they halve, and the
// one round more finds that nothing is left to merge in a forest).  No loop on the device waits for another thread.
// Afterwards the records are sorted by key (two stable radix sorts: the pair, then the weight bits), the tail filled, and the
// smallest row of every component found by the same grouped minimum.
#include "db_device.h"  // uf_find, uf_unite; knn_device.h, lane_walk.h
#include "trueknn_engine.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cfloat>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kEmBlock = 256;
constexpr uint32_t kEmNoWeight = 0x7f800000u;       // +inf: no edge
constexpr unsigned long long kEmNoPair = ~0ull;
constexpr int32_t kEmEmpty = (int32_t)0x80000000;    // arrive[node]: no child has arrived
constexpr int32_t kEmMixed = -1, kEmNeutral = -2;    // node_comp: more than one component / no eligible point
// the call's words: [0] eligible points [1] edges appended; from kEmStats on kEmStripes stripes of a cache line each:
// node tests, point tests, skipped subtrees (a wave adds to the stripe of its index, the host sums them)
constexpr int kEmEligible = 0, kEmEdges = 1, kEmStats = 8, kEmStripes = 32, kEmStripeWords = 8, kEmWords = kEmStats + kEmStripes * kEmStripeWords;

struct EmstArgs {
  LbvhView bvh;
  const int32_t *split_owner;
  const float *core_dist;         // by row, or null
  int32_t *parent, *comp;         // per slot
  float *core_s;                  // per slot: the point's core distance (0 without core distances)
  uint32_t *best_w;               // per slot: the lane's best weight this round (bits), kEmNoWeight: none
  int32_t *best_to;               // per slot: the slot at the other end
  uint32_t *comp_w;               // per slot, meaningful at roots: the component's smallest weight this round
  unsigned long long *comp_pair;  // ... and the smallest pair of names at that weight
  int32_t *arrive, *node_comp;    // per internal node
  unsigned long long *edge_pair;  // the edges appended so far: (u << 32) | v, u < v
  uint32_t *edge_w;
  unsigned long long *words;
};

__device__ __forceinline__ unsigned long long em_pair(int32_t a, int32_t b) {
  const uint32_t x = (uint32_t)a, y = (uint32_t)b;
  return x < y ? ((unsigned long long)x << 32) | y : ((unsigned long long)y << 32) | x;
}

// table[c] = min(table[c], v) for the lanes with `has`, every lane of the wave calling: the lanes of one component reduce among
// themselves, its first lane sends one atomic, and none when a plain load shows that it would change nothing.  A late round has
// a few huge components: without this their millions of lanes would queue at one word each.
template <typename T>
__device__ __forceinline__ void em_group_min(bool has, int32_t c, T v, T *table) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(has);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t lc = __shfl(c, leader);
    const bool mine = has && c == lc;
    const unsigned long long group = __ballot(mine);
    T m = mine ? v : (T)~(T)0;
    if (group & (group - 1)) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const T o = __shfl_xor(m, off);
        m = o < m ? o : m;
      }
    }
    if (lane == leader && __hip_atomic_load(table + lc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > m) atomicMin(table + lc, m);
    todo &= ~group;
  }
}

// ---- before the first round ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kEmBlock) em_init_kernel(EmstArgs a) {
  const int32_t n = a.bvh.n, t = blockIdx.x * kEmBlock + threadIdx.x;
  bool ok = false;
  if (t < n) {
    const LbvhPoint p = a.bvh.points[t];
    float core = a.core_dist ? a.core_dist[a.bvh.prim_id[t]] : 0.f;
    ok = t < lane_clean_end(a.bvh) && p.x == p.x && p.y == p.y && p.z == p.z && core >= 0.f && core <= FLT_MAX;  // (a NaN fails)
    a.parent[t] = t;
    a.comp[t] = ok ? t : -1;
    a.core_s[t] = ok && core > 0.f ? core : 0.f;  // (-0 is 0)
    a.comp_w[t] = kEmNoWeight;
    a.comp_pair[t] = kEmNoPair;
    if (t < n - 1) a.arrive[t] = kEmEmpty;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.words[kEmEligible], (unsigned long long)__popcll(m));
}

// ---- 1. uniform marks ------------------------------------------------------------------------------------------------------
// The value that climbs: a component, kEmNeutral (no eligible point below) or kEmMixed.  It travels inside the exchange, so the
// second child needs no fence to read what the first one left; it also puts the word back for the next round.
__global__ void __launch_bounds__(kEmBlock) em_uniform_kernel(EmstArgs a) {
  const LbvhView &bvh = a.bvh;
  const int32_t n = bvh.n, t = blockIdx.x * kEmBlock + threadIdx.x;
  if (t >= n) return;
  const int32_t c = a.comp[t];
  int32_t val = c >= 0 ? c : kEmNeutral;
  int32_t first = t, last = t, at = ~t;  // the subtree climbed so far: its slots, and its node (or ~slot)
  while (first != 0 || last != n - 1) {
    // parent: a left child ends where its parent splits, a right child begins right after
    int32_t up = -1;
    if (at >= 0) {
      up = a.split_owner[at == last ? at : at - 1];
    } else {
      if (first < n - 1) {
        const int32_t o = a.split_owner[first];
        if (lbvh_first(o, bvh.nodes[o].other) == first) up = o;
      }
      if (up < 0) up = a.split_owner[first - 1];
    }
    const int32_t old = atomicExch(a.arrive + up, val);
    if (old == kEmEmpty) break;  // the first to arrive: the other child goes on
    a.arrive[up] = kEmEmpty;
    val = old == kEmNeutral ? val : val == kEmNeutral || val == old ? old : kEmMixed;
    a.node_comp[up] = val;
    const int32_t other = bvh.nodes[up].other;
    at = up, first = lbvh_first(up, other), last = lbvh_last(up, other);
  }
}

// ---- 2. the nearest point in another component ---------------------------------------------------------------------------------
__global__ void __launch_bounds__(kEmBlock) em_walk_kernel(EmstArgs a) {
  const LbvhView &bvh = a.bvh;
  const int32_t n = bvh.n, t = blockIdx.x * kEmBlock + threadIdx.x;
  const bool in = t < n;
  const LbvhPoint q = in ? bvh.points[t] : LbvhPoint{0.f, 0.f, 0.f, -1};
  const int32_t c = in ? a.comp[t] : -1;
  const float cp = in ? a.core_s[t] : 0.f;
  // the lane's best edge so far, by the full key
  uint32_t bw = kEmNoWeight;
  unsigned long long bpair = kEmNoPair;
  int32_t bto = -1;
  float gate = __uint_as_float(kEmNoWeight);  // nothing heavier than this can be the component's edge
  auto offer = [&](float x, float y, float z, int32_t name, float core, int32_t slot) __attribute__((always_inline)) {
    const float d = knn_sqrt(knn_dist2(x, y, z, q.x, q.y, q.z));
    if (!(d <= FLT_MAX)) return;  // an overflowing (or undefined) distance is no edge
    const uint32_t wb = __float_as_uint(fmaxf(fmaxf(d, cp), core));
    const unsigned long long pair = em_pair(q.id, name);
    if (wb < bw || (wb == bw && pair < bpair)) {
      bw = wb, bpair = pair, bto = slot;
      gate = fminf(gate, __uint_as_float(wb));
    }
  };
  uint32_t node_tests = 0, point_tests = 0, skipped = 0;
  // the other fifteen points of my block of 16: curve neighbours, from the lanes beside me
#pragma unroll
  for (int j = 1; j < LBVH_BLOCK; j++) {
    const float ox = __shfl_xor(q.x, j), oy = __shfl_xor(q.y, j), oz = __shfl_xor(q.z, j), ocore = __shfl_xor(cp, j);
    const int32_t oname = __shfl_xor(q.id, j), oc = __shfl_xor(c, j);
    if (c >= 0 && oc >= 0 && oc != c) {
      point_tests++;
      offer(ox, oy, oz, oname, ocore, t ^ j);
    }
  }
  if (c >= 0) {
    gate = fminf(gate, __uint_as_float(__hip_atomic_load(a.comp_w + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
    auto at_node = [&](int32_t ref, const LbvhNode &nd, int32_t) {
      node_tests++;
      const int32_t nc = a.node_comp[ref];
      if (nc == c || nc == kEmNeutral) {
        skipped += nc == c;
        return lane_rope();
      }
      // every point of the node is at least this far (the margin: lane_counts_subtree's), and no edge of mine is lighter
      // than my core distance
      float far2, near2;
      lane_box_dist2(nd, q, far2, near2);
      const float lower = fmaxf(knn_sqrt(near2 * 0.999995f), cp);
      return lower > gate ? lane_rope() : lane_descend();
    };
    auto at_leaf = [&](int32_t slot, const LbvhPoint &p) {
      const int32_t oc = a.comp[slot];
      if (oc >= 0 && oc != c) {
        point_tests++;
        offer(p.x, p.y, p.z, p.id, a.core_s[slot], slot);
      }
      return lane_rope();
    };
    // From my leaf upwards: at every ancestor the subtree of the OTHER child is walked, so what lies near me on the curve comes
    // first and the bound is tight before the far parts of the tree are looked at (a walk from the root, left first, meets its
    // first foreign point anywhere).  A sibling that lies beyond the bound, or wholly in my component, costs its one node.
    int32_t at = ~t, first = t, last = t;  // the subtree done so far: its reference and its slots
    while (first != 0 || last != n - 1) {
      int32_t up = -1;  // the parent: a left child ends where its parent splits, a right child begins right after (em_uniform_kernel)
      if (at >= 0) {
        up = a.split_owner[at == last ? at : at - 1];
      } else {
        if (first < n - 1) {
          const int32_t o = a.split_owner[first];
          if (lbvh_first(o, bvh.nodes[o].other) == first) up = o;
        }
        if (up < 0) up = a.split_owner[first - 1];
      }
      const LbvhNode nd = bvh.nodes[up];
      const int32_t left = lbvh_left_ref(up, nd), right = lbvh_right_ref(up, nd);
      const bool from_left = at == left;
      const int32_t other = from_left ? right : left;
      // (the left child's rope is the right child; the right child's own rope ends its subtree)
      const int32_t until = !from_left ? at : other >= 0 ? bvh.rope_node[other] : bvh.rope_leaf[~other];
      lane_walk<LaneRope::kWithNode>(bvh, other, until, LBVH_END, LBVH_END, at_node, at_leaf);
      at = up, first = lbvh_first(up, nd.other), last = lbvh_last(up, nd.other);
    }
  }
  if (in) {
    a.best_w[t] = bw;
    a.best_to[t] = bto;
  }
  em_group_min(c >= 0 && bw != kEmNoWeight, c, bw, a.comp_w);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    node_tests += __shfl_xor(node_tests, off);
    point_tests += __shfl_xor(point_tests, off);
    skipped += __shfl_xor(skipped, off);
  }
  if ((threadIdx.x & 63) == 0 && node_tests + point_tests) {
    unsigned long long *st = a.words + kEmStats + ((blockIdx.x * (kEmBlock / 64) + (threadIdx.x >> 6)) & (kEmStripes - 1)) * kEmStripeWords;
    atomicAdd(&st[0], (unsigned long long)node_tests);
    atomicAdd(&st[1], (unsigned long long)point_tests);
    atomicAdd(&st[2], (unsigned long long)skipped);
  }
}

// ---- 3. the smallest pair among the lanes at the component's weight -----------------------------------------------------------
// what a lane offers its component: its edge's pair if the edge has the component's smallest weight
__device__ __forceinline__ bool em_at_minimum(const EmstArgs &a, int32_t t, int32_t &c, uint32_t &bw, int32_t &to, unsigned long long &pair) {
  c = -1, bw = kEmNoWeight, to = -1, pair = kEmNoPair;
  if (t >= a.bvh.n) return false;
  c = a.comp[t];
  bw = a.best_w[t];
  if (c < 0 || bw == kEmNoWeight || bw != a.comp_w[c]) return false;
  to = a.best_to[t];
  pair = em_pair(a.bvh.points[t].id, a.bvh.points[to].id);
  return true;
}

__global__ void __launch_bounds__(kEmBlock) em_pair_kernel(EmstArgs a) {
  int32_t c, to;
  uint32_t bw;
  unsigned long long pair;
  const bool has = em_at_minimum(a, blockIdx.x * kEmBlock + threadIdx.x, c, bw, to, pair);
  em_group_min(has, c, pair, a.comp_pair);
}

// ---- 4. unions and the edge list -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kEmBlock) em_merge_kernel(EmstArgs a) {
  const int32_t t = blockIdx.x * kEmBlock + threadIdx.x;
  int32_t c, to;
  uint32_t bw;
  unsigned long long pair;
  const bool chooser = em_at_minimum(a, t, c, bw, to, pair) && pair == a.comp_pair[c];  // one lane per component
  bool writes = false;
  if (chooser) {
    const int32_t oc = a.comp[to];
    const bool both = a.comp_w[oc] == bw && a.comp_pair[oc] == pair;  // the other component chose this edge too
    writes = !both || (uint32_t)a.bvh.points[t].id < (uint32_t)a.bvh.points[to].id;
    uf_unite(a.parent, c, oc);
  }
  const unsigned long long m = __ballot(writes);
  if (!m) return;
  const int lane = threadIdx.x & 63, first = __ffsll((long long)m) - 1;
  unsigned long long base = 0;
  if (lane == first) base = atomicAdd(&a.words[kEmEdges], (unsigned long long)__popcll(m));
  base = __shfl(base, first);
  if (writes) {
    const unsigned long long at = base + __popcll(m & ((1ull << lane) - 1ull));
    if (at < (unsigned long long)(a.bvh.n - 1)) {  // (a forest has fewer edges than points: never false)
      a.edge_pair[at] = pair;
      a.edge_w[at] = bw;
    }
  }
}

// ---- 5. the components' names for the next round -----------------------------------------------------------------------------
__global__ void __launch_bounds__(kEmBlock) em_relabel_kernel(EmstArgs a) {
  const int32_t t = blockIdx.x * kEmBlock + threadIdx.x;
  if (t >= a.bvh.n) return;
  if (a.comp[t] >= 0) a.comp[t] = uf_find(a.parent, t);
  a.comp_w[t] = kEmNoWeight;
  a.comp_pair[t] = kEmNoPair;
}

// ---- after the rounds ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kEmBlock) em_output_kernel(const unsigned long long *__restrict__ pair, const uint32_t *__restrict__ w, int32_t edges,
                                                            int32_t rows, int32_t *__restrict__ out_u, int32_t *__restrict__ out_v, float *__restrict__ out_w) {
  const int32_t i = blockIdx.x * kEmBlock + threadIdx.x;
  if (i >= rows) return;
  const bool edge = i < edges;
  const unsigned long long p = edge ? pair[i] : kEmNoPair;
  out_u[i] = edge ? (int32_t)(uint32_t)(p >> 32) : -1;
  out_v[i] = edge ? (int32_t)(uint32_t)p : -1;
  if (out_w) out_w[i] = __uint_as_float(edge ? w[i] : kEmNoWeight);
}

// min_row[component] = its smallest row (min_row: preset to all ones)
__global__ void __launch_bounds__(kEmBlock) em_min_row_kernel(EmstArgs a, uint32_t *min_row) {
  const int32_t t = blockIdx.x * kEmBlock + threadIdx.x;
  const bool in = t < a.bvh.n;
  const int32_t c = in ? a.comp[t] : -1;
  em_group_min(c >= 0, c, in ? (uint32_t)a.bvh.prim_id[t] : 0u, min_row);
}
__global__ void __launch_bounds__(kEmBlock) em_component_kernel(EmstArgs a, const uint32_t *__restrict__ min_row, int32_t *__restrict__ out) {
  const int32_t t = blockIdx.x * kEmBlock + threadIdx.x;
  if (t >= a.bvh.n) return;
  const int32_t c = a.comp[t];
  out[a.bvh.prim_id[t]] = c >= 0 ? (int32_t)min_row[c] : -1;
}

}  // namespace

void Engine::emst(const tknnEmstOptions &o, tknnEmstInfo *info, hipStream_t s) {
  const LbvhView tv = bvh_.view();
  const int64_t n = tv.n;
  int bound = 1;  // ceil(log2 n) + 1
  while ((1ll << (bound - 1)) < n) bound++;
  const int max_rounds = o.max_rounds > 0 ? std::min<int>(o.max_rounds, bound) : bound;

  // the call's workspace: words | nine columns of a word per slot | three of two words | the sorts' space
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t sort_bytes = 0, sort_bytes_w = 0;
  {
    unsigned long long *k64 = nullptr;
    uint32_t *k32 = nullptr;
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, k64, k64, k32, k32, (int)n, 0, 64, s));
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes_w, k32, k32, k64, k64, (int)n, 0, 32, s));
    sort_bytes = std::max(sort_bytes, sort_bytes_w);
  }
  const size_t words_b = align(kEmWords * sizeof(unsigned long long)), col_b = align((size_t)n * sizeof(uint32_t)), wide_b = align((size_t)n * sizeof(unsigned long long));
  char *ws = (char *)workspace(words_b + 10 * col_b + 3 * wide_b + align(sort_bytes));
  auto column = [&](int i) { return ws + words_b + (size_t)i * col_b; };
  auto wide = [&](int i) { return ws + words_b + 10 * col_b + (size_t)i * wide_b; };
  EmstArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = tv;
  a.split_owner = bvh_.split_owner_device();
  a.core_dist = o.d_core_dist;
  a.words = (unsigned long long *)ws;
  a.parent = (int32_t *)column(0);
  a.comp = (int32_t *)column(1);
  a.core_s = (float *)column(2);
  a.best_w = (uint32_t *)column(3);
  a.best_to = (int32_t *)column(4);
  a.comp_w = (uint32_t *)column(5);
  a.arrive = (int32_t *)column(6);
  a.node_comp = (int32_t *)column(7);
  a.edge_w = (uint32_t *)column(8);
  uint32_t *edge_w_alt = (uint32_t *)column(9);
  a.comp_pair = (unsigned long long *)wide(0);
  a.edge_pair = (unsigned long long *)wide(1);
  unsigned long long *edge_pair_alt = (unsigned long long *)wide(2);
  void *sort_tmp = wide(3);
  uint32_t *min_row = a.best_w;  // (free after the rounds)

  const dim3 grid((unsigned)((n + kEmBlock - 1) / kEmBlock)), block(kEmBlock);
  unsigned long long *h = h_counters_;
  auto read_record = [&]() {
    OWLMI_HIP(hipMemcpyAsync(h, a.words, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
  };
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(a.words, 0, kEmWords * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(em_init_kernel, grid, block, 0, s, a);
  OWLMI_HIP(hipGetLastError());
  read_record();
  const int64_t eligible = (int64_t)h[kEmEligible];

  int64_t edges = 0, added = 0;
  int rounds = 0;
  float walk_ms = 0, merge_ms = 0;
  while (eligible - edges > 1 && rounds < max_rounds) {
    OWLMI_HIP(hipEventRecord(ev_b_, s));
    if (n > 1) hipLaunchKernelGGL(em_uniform_kernel, grid, block, 0, s, a);
    OWLMI_HIP(hipEventRecord(ev_c_, s));
    hipLaunchKernelGGL(em_walk_kernel, grid, block, 0, s, a);
    OWLMI_HIP(hipEventRecord(ev_d_, s));
    hipLaunchKernelGGL(em_pair_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(em_merge_kernel, grid, block, 0, s, a);
    hipLaunchKernelGGL(em_relabel_kernel, grid, block, 0, s, a);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipEventRecord(ev_e_, s));
    read_record();
    float uniform = 0, walk = 0, merge = 0;
    OWLMI_HIP(hipEventElapsedTime(&uniform, ev_b_, ev_c_));
    OWLMI_HIP(hipEventElapsedTime(&walk, ev_c_, ev_d_));
    OWLMI_HIP(hipEventElapsedTime(&merge, ev_d_, ev_e_));
    walk_ms += walk;
    merge_ms += uniform + merge;
    rounds++;
    added = (int64_t)h[kEmEdges] - edges;
    edges = (int64_t)h[kEmEdges];
    if (added == 0) break;
  }
  const bool unfinished = eligible - edges > 1 && added > 0;  // the bound cut the rounds short

  OWLMI_HIP(hipEventRecord(ev_g_, s));
  if (!unfinished) {
    if (edges > 1) {
      OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, a.edge_pair, edge_pair_alt, a.edge_w, edge_w_alt, (int)edges, 0, 64, s));
      OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, edge_w_alt, a.edge_w, edge_pair_alt, a.edge_pair, (int)edges, 0, 32, s));
    }
    if (n > 1) {
      hipLaunchKernelGGL(em_output_kernel, dim3((unsigned)((n - 1 + kEmBlock - 1) / kEmBlock)), block, 0, s, (const unsigned long long *)a.edge_pair,
                         (const uint32_t *)a.edge_w, (int32_t)edges, (int32_t)(n - 1), o.d_u, o.d_v, o.d_w);
      OWLMI_HIP(hipGetLastError());
    }
    if (o.d_component) {
      OWLMI_HIP(hipMemsetAsync(min_row, 0xff, (size_t)n * sizeof(uint32_t), s));
      hipLaunchKernelGGL(em_min_row_kernel, grid, block, 0, s, a, min_row);
      hipLaunchKernelGGL(em_component_kernel, grid, block, 0, s, a, (const uint32_t *)min_row, o.d_component);
      OWLMI_HIP(hipGetLastError());
    }
  }
  OWLMI_HIP(hipMemcpyAsync(h, a.words + kEmStats, kEmStripes * kEmStripeWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipEventRecord(ev_f_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (info) {
    info->edges = edges;
    info->components = eligible - edges;
    info->excluded = n - eligible;
    for (int j = 0; j < kEmStripes; j++) {
      info->node_tests += (int64_t)h[j * kEmStripeWords];
      info->point_tests += (int64_t)h[j * kEmStripeWords + 1];
      info->skipped_subtrees += (int64_t)h[j * kEmStripeWords + 2];
    }
    info->rounds = rounds;
    info->walk_ms = walk_ms;
    info->merge_ms = merge_ms;
    OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_f_));
    OWLMI_HIP(hipEventElapsedTime(&info->sort_ms, ev_g_, ev_f_));
  }
  if (unfinished) throw RoundsExceeded{};
}

}  // namespace owlmi
