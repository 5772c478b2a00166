// dbscan_union.hip -- RT-DBSCAN's union passes: a walk per core point (db_union_kernel: the fallback, A/B measurements), or
// the group list and a walk per packet of 64 groups (db_group_union_kernel, twice, db_uniform_kernel between).  dbscan.hip
// has the algorithm and the map of the files.
#include "db_call.h"

namespace owlmi {
namespace {

// per-axis reach of a union pass's box prefilter from the pass's bound on the squared distance of nearest faces: at
// least its square root (sqrtf is correctly rounded; two parts in 10^6 cover that rounding and the squares' in near2)
inline float db_reach_of(float near_hi2) { return sqrtf(near_hi2) * 1.000002f; }

__device__ __forceinline__ void db_union_body(const DbArgs &a, int32_t t, unsigned long long *seen, int kPairs, uint32_t &node_tests,
                                              uint32_t &point_tests) {
  const LbvhView &bvh = a.bvh;
  const LbvhPoint q = bvh.points[t];
  // the first tight node on my own root path: its core points are one cluster, held together by its
  // first core point, which also stands for me in the unions below
  int32_t mine = t;
  int32_t node = bvh.root;
  while (node >= 0) {
    const LbvhNode nd = bvh.nodes[node];
    node_tests++;
    if (node_is_tight(nd, a.eps_in2)) {
      const int32_t s = a.next_core[lbvh_first(node, nd.other)];  // <= t: I am core and inside
      if (s != t) {
        mine = s;
        uf_unite(a.parent, t, mine);
      }
      break;
    }
    node = t <= nd.split ? lbvh_left_ref(node, nd) : lbvh_right_ref(node, nd);
  }
  auto slot_of = [&](int32_t other, unsigned long long &key) -> unsigned long long * {
    const uint32_t lo = (uint32_t)min(mine, other), hi = (uint32_t)max(mine, other);
    key = ((unsigned long long)hi << 32) | lo;
    const uint32_t h = (lo * 0x9e3779b1u) ^ (hi * 0x85ebca6bu);
    return seen + ((h >> 11) & (kPairs - 1));
  };
  int32_t my_root = uf_find(a.parent, mine);
  for_each_core_group(
      a, q, t,
      [&](int32_t other) -> bool {  // is that group in my set already?  (then there is nothing to find out)
        if (other == mine) return true;
        unsigned long long key;
        unsigned long long *slot = slot_of(other, key);
        if (*(volatile unsigned long long *)slot == key) return true;
        if (uf_find(a.parent, other) != my_root) {
          my_root = uf_find(a.parent, my_root);  // my root may have been hooked under another meanwhile
          if (uf_find(a.parent, other) != my_root) return false;
        }
        *(volatile unsigned long long *)slot = key;
        return true;
      },
      [&](int32_t other) {
        if (other == mine || other == t) return;
        unsigned long long key;
        unsigned long long *slot = slot_of(other, key);
        if (*(volatile unsigned long long *)slot == key) return;
        *(volatile unsigned long long *)slot = key;
        uf_unite(a.parent, mine, other);
        my_root = uf_find(a.parent, mine);
      },
      node_tests, point_tests);
}

__global__ void __launch_bounds__(kDbBlock) db_union_kernel(DbArgs a) {
  // The 256 curve-consecutive points of a workgroup mostly share a tight node and meet the same
  // neighbouring tight nodes: every (my group, other group) pair would be united hundreds of times,
  // each a pair of union-find walks through global atomics.  A direct-mapped LDS table of the pairs
  // this workgroup has already taken care of drops the repeats (a stale or raced entry only costs a
  // redundant unite; the pair that set an entry is united by the lane that set it).
  constexpr int kPairs = 2048;
  __shared__ unsigned long long seen[kPairs];
  __shared__ unsigned long long blk_stats[2];
  for (int i = threadIdx.x; i < kPairs; i += kDbBlock) seen[i] = ~0ull;
  if (threadIdx.x < 2) blk_stats[threadIdx.x] = 0ull;
  __syncthreads();
  uint32_t node_tests = 0, point_tests = 0;
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  if (t < a.bvh.n && a.core_sorted[t]) db_union_body(a, t, seen, kPairs, node_tests, point_tests);
  db_add_stats(a.stats + kDbStatUnion, blk_stats, node_tests, point_tests);
}

// ---- unions by GROUP: one walk per maximal tight node ------------------------------------------------------------------
// Every point lies in exactly one maximal tight node (a node whose box diagonal is below eps and whose parent's is not;
// a leaf under a non-tight parent is one by itself): a GROUP.  A group's core points are one cluster, so the clusters are
// the components of the graph of groups with an edge (A, B) iff some core point of A lies within eps of some core point
// of B.  The per-point walk above pays a tree descent per POINT to the same ~100 neighbouring groups every other point of
// its group reaches too (BASELINE config 3: 500 node tests per point, 40 of the call's 44 ms).  Here each group walks once,
// box against tree, and only over the slots AFTER its own (the rope of its node is where a depth-first walk continues
// behind it): a pair of groups is looked at exactly once, from its earlier end.
//   group kernel: every point finds its group on its own root path; core points unite with the group's first core point;
//                 the point at the group's first slot lists the group if it has a core point.
//   union kernel: one lane per listed group.  A later group B in reach: no box point within eps (nearest faces) -> nothing;
//                 same set already -> nothing; farthest corners within eps -> unite; otherwise PROBE: core points of A that
//                 are within eps of B's box against B's core points, by the spec's distance arithmetic, until the first hit.
__device__ __forceinline__ void box_box_dist2(const float *alo, const float *ahi, const float *blo, const float *bhi, float &far2,
                                              float &near2) {
  float f = 0.f, g = 0.f;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float fa = fmaxf(fabsf(ahi[c] - blo[c]), fabsf(bhi[c] - alo[c]));
    const float ne = fmaxf(fmaxf(blo[c] - ahi[c], alo[c] - bhi[c]), 0.f);
    f += fa * fa;
    g += ne * ne;
  }
  far2 = f;
  near2 = g;
}

// per slot: the group's reference (node, or ~slot of a single point) at the group's first slot if the group has a core
// point, LBVH_END everywhere else -- compacted into the list, in slot order, in three steps: this kernel counts each
// workgroup's entries, an exclusive sum over those n / 256 counts gives the workgroups' places, db_group_list_kernel writes
// the entries (a library select over the n slots took 0.09 ms of a 3 ms call).  The core-flag
// kernel has left every point's group in group_of (it walks the point's root path anyway).
// (The kernel also fills, as it streams by, what later launches want filled: a fill is a launch of its own otherwise.)
__global__ void __launch_bounds__(kDbBlock) db_group_kernel(DbArgs a, int32_t *group_at, int32_t *fill_uni, int32_t *fill_min_row,
                                                            int32_t *block_count) {
  __shared__ int32_t wave_count[kDbBlock / 64];
  const LbvhView &bvh = a.bvh;
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  int32_t out = LBVH_END;
  if (t < bvh.n) {
    fill_uni[t] = -1;              // db_uniform_kernel: nobody has arrived
    fill_min_row[t] = 0x7f7f7f7f;  // db_flatten_kernel: above every row
    const int32_t g = a.group_of[t];
    const bool leads = g >= 0 || g == ~t;
    const int32_t first = leads ? t : ~g;
    const int32_t s = a.next_core[first];
    // s < t, both core, one group: united by a plain store -- these are the call's first unions, every slot is still its
    // own root, s stays one throughout this kernel (only later slots are hooked, under it), and parent[t] is written by
    // nobody else
    if (a.core_sorted[t] && s != t && !(a.diag & 4)) a.parent[t] = s;
    if (leads) {
      const int32_t last = g >= 0 ? lbvh_last(g, bvh.nodes[g].other) : t;
      if (s <= last) out = g;
    }
    group_at[t] = out;
  }
  const unsigned long long m = __ballot(out != LBVH_END);
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t c = 0;
    for (int w = 0; w < kDbBlock / 64; w++) c += wave_count[w];
    block_count[blockIdx.x] = c;
  }
}
__global__ void __launch_bounds__(kDbBlock) db_group_list_kernel(DbArgs a, const int32_t *group_at, const int32_t *block_place, int32_t *groups,
                                                                 unsigned long long *total) {
  __shared__ int32_t wave_count[kDbBlock / 64];
  const int32_t t = blockIdx.x * kDbBlock + threadIdx.x;
  const int32_t g = t < a.bvh.n ? group_at[t] : LBVH_END;
  const unsigned long long m = __ballot(g != LBVH_END);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_count[wave] = __popcll(m);
  __syncthreads();
  int32_t place = block_place[blockIdx.x];
  for (int w = 0; w < wave; w++) place += wave_count[w];
  if (g != LBVH_END) groups[place + __popcll(m & ((1ull << lane) - 1ull))] = g;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == kDbBlock - 1) *total = (unsigned long long)(place + __popcll(m));  // the list's length
}

// Between the two passes of the group-union kernel: which tree nodes hold core points of ONE set only?  After the first pass
// (pairs of groups that nearly touch) a cluster's dense part is one set, and the second pass, which walks the tree with the
// full reach, would still go down to every group around a packet only to find it in the packet's own set.  One lane per
// listed group climbs from the group towards the root: a parent whose other child has no core point inherits the set; at a
// parent with two children that have some, the first to arrive leaves its set there and stops, the second goes on if both
// sets are the same (a side that is not one set never arrives, and the parent stays "not known").  Roots do not move
// during this kernel (no unions), so two lanes of one set see the same root.
//   uni[node]: -1 nobody arrived; <= -2: one child arrived with set -2 - value; >= 0: one set, this root
__global__ void __launch_bounds__(kDbBlock) db_uniform_kernel(DbArgs a, const int32_t *groups, const unsigned long long *n_groups) {
  const LbvhView &bvh = a.bvh;
  const long long g = (long long)blockIdx.x * kDbBlock + threadIdx.x;
  if (g >= (long long)*n_groups) return;
  const int32_t G = groups[g];
  int32_t first, last, at = G;  // the subtree climbed so far: its slots, and its node (or ~slot)
  if (G >= 0) {
    const int32_t other = bvh.nodes[G].other;
    first = lbvh_first(G, other), last = lbvh_last(G, other);
  } else {
    first = last = ~G;
  }
  const int32_t set = uf_find(a.parent, a.next_core[first]);
  if (G >= 0)
    a.uni[G] = set;
  else
    a.uni_leaf[first] = set;
  const int32_t n = bvh.n;
  while (first != 0 || last != n - 1) {
    // parent: a left child ends where its parent splits, a right child begins right after
    int32_t up = -1;
    bool is_left = false;
    if (at >= 0) {
      is_left = at == last;
      up = a.split_owner[is_left ? at : at - 1];
    } else {
      if (first < n - 1) {
        const int32_t o = a.split_owner[first];
        if (lbvh_first(o, bvh.nodes[o].other) == first) up = o, is_left = true;
      }
      if (up < 0) up = a.split_owner[first - 1];
    }
    const LbvhNode nd = bvh.nodes[up];
    const int32_t up_first = lbvh_first(up, nd.other), up_last = lbvh_last(up, nd.other);
    const int32_t sib_first = is_left ? nd.split + 1 : up_first, sib_last = is_left ? up_last : nd.split;
    if (a.next_core[sib_first] <= sib_last) {  // the other child has core points: both must arrive, with one set
      const int32_t old = atomicExch(a.uni + up, -2 - set);
      if (old == -1 || -2 - old != set) break;
    }
    a.uni[up] = set;
    at = up, first = up_first, last = up_last;
  }
}

// Persistent waves, each working on one PACKET of 64 consecutive groups of the list at a time (curve neighbours: they
// meet the same nodes).  The wave walks the tree ONCE for the packet, in two alternating roles:
//   lanes = nodes: up to 64 references are popped from the wave's LDS stack and their boxes (a leaf's is its point)
//                  loaded at once and put into LDS;
//   lanes = groups: every popped box, read from LDS by all lanes, is tested against each lane's own group widened by the
//                  reach.  A node no group reaches is dropped.  A tight node (the walk only descends through nodes that are
//                  not: it is maximal, a group) or a core leaf is collected, in the lane's own LDS column, by every group
//                  that has it in reach (nearest faces within eps) and lies before it; when a lane has kDbBuf waiting, the
//                  wave settles what all lanes have collected: first core slots, rows and parent pointers fetched for all
//                  at once, then one after the other.
//   lanes = nodes: the nodes some group reaches that are not tight push their children.
// (History, BASELINE config 3, union pass: a walk per POINT 40 ms; a walk per group, one lane each, 5 ms -- 320 node visits
// per group, each a 64-byte sector from memory because 8 000 waves at different places of a 320 MB tree share nothing in a
// 4 MB L2: 15 GB per launch; one rope walk per packet, wave-uniform, 1.8 ms per launch -- 1 300 dependent loads in a row;
// the stack walk needs some 40 rounds of loads per packet; with the popped nodes tested against the packet's bounding box
// instead of its 64 groups, a packet across a jump of the Z-curve walked half the tree: one wave, 4 ms.)
#ifndef TKNN_DB_BUF
#define TKNN_DB_BUF 8
#endif
constexpr int kDbBuf = TKNN_DB_BUF;
#ifndef TKNN_DB_BOXES
#define TKNN_DB_BOXES 2
#endif
constexpr int kDbBoxes = TKNN_DB_BOXES;  // bounding boxes per packet for the prefilter of popped nodes (64 / kDbBoxes lanes each)
#ifndef TKNN_DB_UNION_BLOCK
#define TKNN_DB_UNION_BLOCK 128  // threads per workgroup of the group-union kernel (its waves are independent)
#define TKNN_DB_WAVES 5          // waves per SIMD its register allocation aims at
#endif
constexpr int kDbUnionBlock = TKNN_DB_UNION_BLOCK;
#ifndef TKNN_DB_STACK
#define TKNN_DB_STACK 512  // (a build with 320 exercises the depth-first mode and the overflow fallback: tests)
#endif
constexpr int kDbStack = TKNN_DB_STACK;  // references per wave; popped one at a time (depth first) when fewer than 256 places are left
constexpr int kDbCand = 64;     // the boxes popped in one round, per wave
struct DbCand {
  float lo[3];
  int32_t ref;    // node, or ~slot of a single point
  float hi[3];
  int32_t other;  // the other end of the node's slot range (a leaf: its slot)
};
__device__ __forceinline__ void db_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__global__ void __launch_bounds__(kDbUnionBlock) __attribute__((amdgpu_waves_per_eu(TKNN_DB_WAVES))) db_group_union_kernel(DbArgs a, const int32_t *groups, const unsigned long long *n_groups,
                                                                  unsigned long long *next_packet, unsigned long long *overflow) {
  __shared__ int32_t buf_ref[kDbBuf * kDbUnionBlock];    // [entry][thread]: the group's node (or ~slot of a single point)
  __shared__ int32_t buf_other[kDbBuf * kDbUnionBlock];  // the other end of its slot range | far-corners-within-eps << 31
  __shared__ int32_t stack_all[(kDbUnionBlock / 64) * kDbStack];
  __shared__ __align__(16) DbCand cand_all[(kDbUnionBlock / 64) * kDbCand];
  int32_t *stack = stack_all + (threadIdx.x >> 6) * kDbStack;
  DbCand *cand = cand_all + (threadIdx.x >> 6) * kDbCand;
  const LbvhView &bvh = a.bvh;
  uint32_t node_tests = 0, point_tests = 0;
  if ((a.diag & 16) && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(overflow, 1ull);  // diagnostic library: take the host's fallback
  const long long total = (long long)*n_groups;
  const long long packets = (total + 63) / 64;
  const int lane = threadIdx.x & 63;
  int32_t *my_ref = buf_ref + threadIdx.x, *my_other = buf_other + threadIdx.x;
  const float r = a.reach;
  typedef float t_f4 __attribute__((ext_vector_type(4)));
  const int xcc = (int)__builtin_amdgcn_s_getreg(6164 /* hwreg(HW_REG_XCC_ID, 0, 4) */) & 7;
  const long long chunk = a.chunk;  // packets per chunk dealt to an XCD
  uint32_t seg_empty = 0;           // XCDs whose chunks are used up (wave-uniform)
  float alo[3], ahi[3];
  int32_t a_last = 0, a_core = 0, mine = 0, my_root = 0;
  // B = a tight node or a single leaf with box blo..bhi, first core slot b_core, last slot b_last: an edge?
  // A scan: my core points that are within eps of B's box against B's core points, until the first hit.  With a budget
  // (steps of either loop) it is the first thing tried -- between neighbouring groups of a dense region the first pairs
  // looked at are within eps -- and gives up undecided (-1) when the budget is spent; without one it is exact (1 / 0).
  auto probe = [&](const float *blo, const float *bhi, int32_t b_core, int32_t b_last, int budget) -> int {
    for (int32_t i = a_core; i <= a_last; i = a.next_core[i + 1]) {
      if (budget-- == 0) return -1;
      const LbvhPoint p = bvh.points[i];
      const float bx = fmaxf(fmaxf(blo[0] - p.x, p.x - bhi[0]), 0.f), by = fmaxf(fmaxf(blo[1] - p.y, p.y - bhi[1]), 0.f),
                  bz = fmaxf(fmaxf(blo[2] - p.z, p.z - bhi[2]), 0.f);
      if (bx * bx + by * by + bz * bz > a.eps_out2) continue;  // nothing of B within eps of p
      for (int32_t j = b_core; j <= b_last; j = a.next_core[j + 1]) {
        if (budget-- == 0) return -1;
        const LbvhPoint q = bvh.points[j];
        point_tests++;
        if (knn_sqrt(knn_dist2(q.x, q.y, q.z, p.x, p.y, p.z)) <= a.eps) return 1;
      }
    }
    return 0;
  };
  // The same question answered down the two groups' own subtrees: a pair of sub-nodes is dropped when its nearest
  // faces are beyond eps or one side has no core point, settles the question when its farthest corners are within eps,
  // and is split otherwise (the side with the longer diagonal) -- a few dozen steps where the scan above may look at
  // every point of a group of thousands before it meets one near the other group (50 M heavy-tailed 2-D points with
  // duplicates: 21 ms for the union pass with the scan alone).  1 / 0: edge / none; -1: the stack is full, scan instead.
  int32_t a_ref = 0;
  auto tree_probe = [&](int32_t b_ref) -> int {
    constexpr int kDepth = 24;
    volatile int32_t sx[kDepth], sy[kDepth];  // (volatile: private memory, not 48 registers)
    int top = 0;
    sx[top] = a_ref, sy[top] = b_ref, top++;
    while (top > 0) {
      top--;
      const int32_t x = sx[top], y = sy[top];
      float xlo[3], xhi[3], ylo[3], yhi[3];
      int32_t x_first, x_last, y_first, y_last, x_split = 0, y_split = 0;
      if (x >= 0) {
        const LbvhNode nd = bvh.nodes[x];
        for (int c = 0; c < 3; c++) xlo[c] = nd.lo[c], xhi[c] = nd.hi[c];
        x_first = lbvh_first(x, nd.other), x_last = lbvh_last(x, nd.other), x_split = nd.split;
      } else {
        const LbvhPoint q = bvh.points[~x];
        xlo[0] = xhi[0] = q.x, xlo[1] = xhi[1] = q.y, xlo[2] = xhi[2] = q.z;
        x_first = x_last = ~x;
      }
      if (y >= 0) {
        const LbvhNode nd = bvh.nodes[y];
        for (int c = 0; c < 3; c++) ylo[c] = nd.lo[c], yhi[c] = nd.hi[c];
        y_first = lbvh_first(y, nd.other), y_last = lbvh_last(y, nd.other), y_split = nd.split;
      } else {
        const LbvhPoint q = bvh.points[~y];
        ylo[0] = yhi[0] = q.x, ylo[1] = yhi[1] = q.y, ylo[2] = yhi[2] = q.z;
        y_first = y_last = ~y;
      }
      if (a.next_core[x_first] > x_last || a.next_core[y_first] > y_last) continue;  // a side without a core point
      float far2, near2;
      box_box_dist2(xlo, xhi, ylo, yhi, far2, near2);
      if (near2 > a.eps_out2) continue;
      if (far2 <= a.eps_in2) return 1;
      if (x < 0 && y < 0) {  // two core points within rounding of eps: the spec's arithmetic decides
        point_tests++;
        if (knn_sqrt(knn_dist2(ylo[0], ylo[1], ylo[2], xlo[0], xlo[1], xlo[2])) <= a.eps) return 1;
        continue;
      }
      if (top + 2 > kDepth) return -1;
      const float dx = (xhi[0] - xlo[0]) * (xhi[0] - xlo[0]) + (xhi[1] - xlo[1]) * (xhi[1] - xlo[1]) + (xhi[2] - xlo[2]) * (xhi[2] - xlo[2]);
      const float dy = (yhi[0] - ylo[0]) * (yhi[0] - ylo[0]) + (yhi[1] - ylo[1]) * (yhi[1] - ylo[1]) + (yhi[2] - ylo[2]) * (yhi[2] - ylo[2]);
      if (x >= 0 && (y < 0 || dx >= dy)) {
        sx[top] = x_first == x_split ? ~x_split : x_split, sy[top] = y, top++;
        sx[top] = x_last == x_split + 1 ? ~(x_split + 1) : x_split + 1, sy[top] = y, top++;
      } else {
        sx[top] = x, sy[top] = y_first == y_split ? ~y_split : y_split, top++;
        sx[top] = x, sy[top] = y_last == y_split + 1 ? ~(y_split + 1) : y_split + 1, top++;
      }
    }
    return 0;
  };
  int waiting = 0;
  [[maybe_unused]] uint32_t pk_long = 0;  // (timing) entries of this packet that went the long way, over the lanes: summed at the end
  [[maybe_unused]] unsigned long long tm[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tm_mark = 0;
  const bool timing = TKNN_DIAG_BUILD && (a.diag & 512) && !((a.diag & 2048) && a.near_lo2 < 0.f) && !((a.diag & 4096) && a.near_lo2 >= 0.f);  // 2048 / 4096: the second / first pass only
#define DB_LAP(i)                                                  \
  do {                                                             \
    if (timing) {                                                  \
      const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
      tm[i] += now_ - tm_mark;                                     \
      tm_mark = now_;                                              \
    }                                                              \
  } while (0)
  // what the lanes have collected: two rounds of loads for all of it, then one group after the other
  auto settle = [&]() {
    DB_LAP(1);
    if (timing) tm[6]++;
    // (every load of a round is issued whether its entry exists or not, from a place that does: a load under a condition is
    // waited for before the next one is issued -- eight round trips to memory instead of one)
    int32_t b_core[kDbBuf], b_last[kDbBuf], par[kDbBuf], at[kDbBuf];
#pragma unroll
    for (int w = 0; w < kDbBuf; w++) {
      const int32_t x = my_ref[w * kDbUnionBlock], o = my_other[w * kDbUnionBlock] & 0x7fffffff;
      const int32_t end = x >= 0 ? x : ~x;
      const bool is = w < waiting;
      b_last[w] = is ? max(end, o) : -1;
      at[w] = is ? min(end, o) : 0;
    }
#pragma unroll
    for (int w = 0; w < kDbBuf; w++) b_core[w] = a.next_core[at[w]];
#pragma unroll
    for (int w = 0; w < kDbBuf; w++) {
      if (!(w < waiting)) b_core[w] = 0x7fffffff;
      at[w] = b_core[w] <= b_last[w] ? b_core[w] : 0;
    }
#pragma unroll
    for (int w = 0; w < kDbBuf; w++) par[w] = uf_load(a.parent + at[w]);
    const int32_t my_up = uf_load(a.parent + my_root);  // (my root may have been hooked under another since I last looked)
#pragma unroll
    for (int w = 0; w < kDbBuf; w++) at[w] = par[w];  // >= 0: parents of places that exist
    // a third round: the parents' parents -- with path halving a slot is rarely more than two steps below its root, and a
    // group whose ROOT is mine needs no look at all (most of what a lane collects in the second pass, where the sets have
    // grown together but the first core slots still point at roots of the first pass)
#pragma unroll
    for (int w = 0; w < kDbBuf; w++) par[w] = uf_load(a.parent + at[w]);
    if (my_up != my_root) my_root = uf_find(a.parent, my_up);
    uint32_t todo = 0;  // collected groups that have a core point and are not in my set as far as these loads can tell
#pragma unroll
    for (int w = 0; w < kDbBuf; w++) {
      if (!(b_core[w] <= b_last[w])) continue;  // no core point in it (or no entry)
      if (par[w] != at[w]) par[w] = uf_find(a.parent, par[w]);  // (more than two steps: the chain, rarely)
      if (par[w] != my_root) todo |= 1u << w;  // par[w]: the group's root
    }
    if (a.diag & 2) todo = 0;
    // The short way first: if the farthest corners are within eps the edge is known, and one compare-and-swap hooks the
    // larger root under the smaller.  (A root read here may be hooked under another by a different wave by now: the swap then
    // fails, or hooks under a slot that is no root any more but IS in my set; the first is left to the long way below, the
    // second is fine.)  Tried and dropped: deciding the other pairs here too by ONE distance, first core point against first
    // core point -- in the first pass that is an edge for half of them, and the pass got 0.3 ms SLOWER (2.13 against 1.82 ms
    // for both).
#pragma unroll
    for (int w = 0; w < kDbBuf; w++) {
      if (!(todo & (1u << w)) || !a.short_way || my_other[w * kDbUnionBlock] >= 0) continue;
      const int32_t ro = par[w];
      if (ro == my_root) {  // (joined by an earlier entry of this very loop)
        todo &= ~(1u << w);
        continue;
      }
      const int32_t lo = min(ro, my_root), hi = max(ro, my_root);
      if (atomicCAS(a.parent + hi, hi, lo) == hi) {
        todo &= ~(1u << w);
        my_root = lo;
      }
    }
    // the rest one after the other (not unrolled: the probe's private stack would be kept once per copy)
    while (todo) {
      const int w = __ffs((int)todo) - 1;
      todo &= todo - 1u;
      if (timing) pk_long++;
      const int32_t B = my_ref[w * kDbUnionBlock], packed = my_other[w * kDbUnionBlock];
      const int32_t end = B >= 0 ? B : ~B, o = packed & 0x7fffffff;
      const int32_t other_last = max(end, o), other = a.next_core[min(end, o)];  // its first core slot stands for the group
      if (uf_find(a.parent, other) == my_root) continue;
      my_root = uf_find(a.parent, my_root);  // my root may have been hooked under another meanwhile
      if (uf_find(a.parent, other) == my_root) continue;
      bool edge = packed < 0;
      if (!edge && !(a.diag & 1)) {
        // a few pairs by scanning, then down the two subtrees, and the whole scan if that runs out of stack
        float blo[3], bhi[3];
        if (B >= 0) {
          const LbvhNode nd = bvh.nodes[B];
          for (int c = 0; c < 3; c++) blo[c] = nd.lo[c], bhi[c] = nd.hi[c];
        } else {
          const LbvhPoint q = bvh.points[~B];
          blo[0] = bhi[0] = q.x, blo[1] = bhi[1] = q.y, blo[2] = bhi[2] = q.z;
        }
        int found = probe(blo, bhi, other, other_last, a.scan_budget);
        if (found < 0 && !(a.diag & 32)) found = tree_probe(B);
        if (found < 0) found = probe(blo, bhi, other, other_last, -1);
        edge = found > 0;
      }
      if (edge) {
        uf_unite(a.parent, mine, other);
        my_root = uf_find(a.parent, mine);
      }
    }
    waiting = 0;
    DB_LAP(2);
  };
  if (timing) tm_mark = __builtin_amdgcn_s_memtime();
  [[maybe_unused]] const unsigned long long wave_t0 = tm_mark;
  for (;;) {
    // ---- take a packet.  Each XCD has its own L2: the list is dealt to the XCDs in chunks of packets, a wave takes from
    // the chunks of the XCD it runs on and from the others' when those are used up.
    long long packet = -1;
    for (int t = 0; t < 8 && packet < 0; t++) {
      const int from = (xcc + t) & 7;
      if (seg_empty & (1u << from)) continue;
      unsigned long long v = 0;
      if (t > 0) {  // another XCD's packets (mine are used up): a look before the turn -- cursors only grow, a load does not queue
        if (lane == 0) v = __hip_atomic_load(next_packet + from * kDbCursorStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        v = __shfl(v, 0);
        if ((((long long)v / chunk) * 8 + from) * chunk + (long long)v % chunk >= packets) {
          seg_empty |= 1u << from;
          continue;
        }
      }
      if (lane == 0) v = atomicAdd(next_packet + from * kDbCursorStride, 1ull);
      v = __shfl(v, 0);
      const long long p = (((long long)v / chunk) * 8 + from) * chunk + (long long)v % chunk;
      if (p < packets)
        packet = p;
      else
        seg_empty |= 1u << from;  // places only grow: this XCD's chunks are used up
    }
    if (packet < 0) break;
    [[maybe_unused]] const unsigned long long packet_t0 = timing ? __builtin_amdgcn_s_memtime() : 0ull;
    [[maybe_unused]] const unsigned long long pk_rounds0 = tm[5], pk_settles0 = tm[6], pk_settle_t0 = tm[2];
    [[maybe_unused]] const uint32_t pk_points0 = point_tests;
    pk_long = 0;
    // ---- lanes = the packet's groups
    const long long g = packet * 64 + lane;
    const bool have = g < total;
    int32_t a_first = 0x7fffffff;
    a_last = 0x7fffffff;  // a lane without a group: nothing lies after it
    alo[0] = alo[1] = alo[2] = ahi[0] = ahi[1] = ahi[2] = 0.f;
    if (have) {
      const int32_t G = groups[g];
      a_ref = G;
      if (G >= 0) {
        const LbvhNode nd = bvh.nodes[G];
        for (int c = 0; c < 3; c++) alo[c] = nd.lo[c], ahi[c] = nd.hi[c];
        a_first = lbvh_first(G, nd.other);
        a_last = lbvh_last(G, nd.other);
      } else {
        const LbvhPoint p = bvh.points[~G];
        alo[0] = ahi[0] = p.x, alo[1] = ahi[1] = p.y, alo[2] = ahi[2] = p.z;
        a_first = a_last = ~G;
      }
      a_core = a.next_core[a_first];  // <= a_last: listed groups have a core point
      mine = a_core;
      my_root = uf_find(a.parent, mine);
    }
    // second pass: the one set all the packet's groups were in when the first pass had ended, if they were (the inside of
    // a cluster): a node whose core points were all in that set (a.uni) has nothing to offer to any of them.  Both sides
    // of the comparison are names of that moment (db_uniform_kernel) -- the roots move while this pass unites sets.
    int32_t pk_root = -1;
    if (a.uni) {
      const int32_t set0 = !have ? -1 : a_ref >= 0 ? a.uni[a_ref] : a.uni_leaf[~a_ref];
      const int32_t r0 = __builtin_amdgcn_readfirstlane(set0);
      if (__ballot(have && set0 != r0) == 0ull) pk_root = r0;
      if (TKNN_DIAG_BUILD && (a.diag & 1024) && lane == 0) atomicAdd(&a.diag_out[pk_root >= 0 ? 8 : 9], 1ull);
    }
    // nothing before the packet's earliest group end can lie after any of its groups
    int32_t low = a_last;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) low = min(low, __shfl_xor(low, off));
    // Bounding boxes of the packet's groups, one per 32 lanes (curve neighbours; two boxes hug a packet that lies across
    // a jump of the Z curve better than one), widened by the reach: a popped node that meets neither can be reached by no
    // group and is dropped where it is popped -- 64 nodes per instruction -- instead of costing a turn of the test loop
    // below, which deals with one node at a time (47 % of the kernel's wave time, half of it on nodes no group reaches).
    float u_lo[kDbBoxes][3], u_hi[kDbBoxes][3];
    {
      float l[3], h[3];
      for (int c = 0; c < 3; c++) {
        // (a margin of a millionth of the magnitudes involved: fl(e.lo - r) <= a.hi, the groups' own test, and
        // e.lo <= fl(a.hi + r) can differ in the last place; the prefilter must never drop what a group would take)
        const float slack = 1e-6f * (fabsf(alo[c]) + fabsf(ahi[c]) + r);
        l[c] = have ? (alo[c] - r) - slack : INFINITY;
        h[c] = have ? (ahi[c] + r) + slack : -INFINITY;
#pragma unroll
        for (int off = 32 / kDbBoxes; off > 0; off >>= 1) {
          l[c] = fminf(l[c], __shfl_xor(l[c], off));
          h[c] = fmaxf(h[c], __shfl_xor(h[c], off));
        }
#pragma unroll
        for (int half = 0; half < kDbBoxes; half++) {
          u_lo[half][c] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(l[c]), (64 / kDbBoxes) * half));
          u_hi[half][c] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(h[c]), (64 / kDbBoxes) * half));
        }
      }
    }
    // ---- the packet's walk
    const unsigned long long below = (1ull << lane) - 1ull;
    int top = 1;
    if (lane == 0) stack[0] = bvh.root;
    db_wave_sync();
    DB_LAP(4);
    if (timing) tm[7]++;
    while (top > 0) {
      if (timing) tm[5]++;
      // lanes = nodes: pop, load, stage
      const int width = top > kDbStack - 256 ? 1 : 64;
      const int n_pop = min(top, width);
      const bool valid = lane < n_pop;
      const int32_t ref = valid ? stack[top - 1 - lane] : bvh.root;
      top -= n_pop;
      const bool is_node = ref >= 0;
      const int32_t slot = is_node ? 0 : ~ref;
      const t_f4 *src = is_node ? (const t_f4 *)(bvh.nodes + ref) : (const t_f4 *)(bvh.points + slot);
      const t_f4 v0 = src[0], v1 = src[is_node ? 1 : 0];
      // (loads that only some lanes or some packets need are issued all the same, beside the boxes: under a condition they
      // would be a second and a third round trip to memory in every round)
      const uint8_t leaf_core = a.core_sorted[slot];
      int32_t node_set = -1;
      if (a.uni) node_set = (is_node ? a.uni : a.uni_leaf)[is_node ? ref : slot];  // (a leaf that is not core: whatever is there)
      const bool any_core = is_node || leaf_core != 0;
      if (valid) node_tests++;
      const int32_t split = __float_as_int(v0.w), b_other = is_node ? __float_as_int(v1.w) : slot;
      const int32_t my_end = is_node ? ref : slot;
      const int32_t b_first = min(my_end, b_other), b_last = max(my_end, b_other);
      const float ex = v1.x - v0.x, ey = v1.y - v0.y, ez = v1.z - v0.z;
      const bool tight = !is_node || ex * ex + ey * ey + ez * ez <= a.eps_in2;  // node_is_tight
      {
        DbCand &e = cand[lane];
        e.lo[0] = v0.x, e.lo[1] = v0.y, e.lo[2] = v0.z;
        e.ref = ref;
        e.hi[0] = v1.x, e.hi[1] = v1.y, e.hi[2] = v1.z;
        e.other = b_other;
      }
      // nodes nothing can come of: past the packet's last use, a leaf that is not core, out of every group's reach
      bool near_packet = false;
#pragma unroll
      for (int half = 0; half < kDbBoxes; half++)
        near_packet |= (v0.x <= u_hi[half][0]) & (u_lo[half][0] <= v1.x) & (v0.y <= u_hi[half][1]) & (u_lo[half][1] <= v1.y) &
                       (v0.z <= u_hi[half][2]) & (u_lo[half][2] <= v1.z);
      if (TKNN_DIAG_BUILD && (a.diag & 1024) && a.uni) {
        const unsigned long long sk = __ballot(valid && pk_root >= 0 && node_set == pk_root), al = __ballot(valid), un = __ballot(valid && is_node && a.uni[ref] >= 0);
        if (lane == 0) atomicAdd(&a.diag_out[10], (unsigned long long)__popcll(sk)), atomicAdd(&a.diag_out[11], (unsigned long long)__popcll(al)), atomicAdd(&a.diag_out[12], (unsigned long long)__popcll(un));
      }
      const unsigned long long m_live = __ballot(valid && any_core && b_last > low && near_packet && !(pk_root >= 0 && node_set == pk_root)), m_tight = __ballot(tight);
      db_wave_sync();
      DB_LAP(0);
      // lanes = groups
      unsigned long long m_open = 0ull;  // nodes some group reaches and that are not tight
      for (unsigned long long todo = m_live; todo;) {
        const int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const DbCand e = cand[j];
        // (the staged node is the same in every lane: its slot range as scalars)
        const int32_t e_ref = __builtin_amdgcn_readfirstlane(e.ref), e_other = __builtin_amdgcn_readfirstlane(e.other);
        const int32_t e_end = e_ref >= 0 ? e_ref : ~e_ref;
        const int32_t e_first = min(e_end, e_other), e_last = max(e_end, e_other);
        // within reach along every axis: the largest separation of the two boxes against r -- subtractions and maxima instead
        // of six compares and their mask operations (a third of this loop's slow instructions; as conservative as
        // fl(e.lo - r) <= a.hi: a difference that is <= r before rounding is <= r after it)
        const float sx = fmaxf(e.lo[0] - ahi[0], alo[0] - e.hi[0]), sy = fmaxf(e.lo[1] - ahi[1], alo[1] - e.hi[1]),
                    sz = fmaxf(e.lo[2] - ahi[2], alo[2] - e.hi[2]);
        const bool hit = (fmaxf(fmaxf(sx, sy), sz) <= r) & (e_last > a_last);
        if (__ballot(hit) == 0ull) continue;
        if (!((m_tight >> j) & 1ull)) {
          m_open |= 1ull << j;
          continue;
        }
        float far2, near2;
        box_box_dist2(alo, ahi, e.lo, e.hi, far2, near2);
        if (hit && e_first > a_last && near2 <= a.near_hi2 && near2 > a.near_lo2) {
          my_ref[waiting * kDbUnionBlock] = e.ref;
          my_other[waiting * kDbUnionBlock] = e.other | (far2 <= a.eps_in2 ? (int32_t)0x80000000 : 0);
          waiting++;
        }
        if (__ballot(waiting == kDbBuf) != 0ull) settle();
      }
      DB_LAP(1);
      // lanes = nodes: children (the left one only if it reaches past the packet's earliest group)
      const bool kids = (m_open >> lane) & 1ull;
      const bool left_too = kids && split > low;
      const unsigned long long m_left = __ballot(left_too);
      const int n_left = __popcll(m_left), n_right = __popcll(m_open);
      if (top + n_left + n_right > kDbStack) {  // (cannot happen below a tree depth of some 250 levels; the host then falls back)
        if (lane == 0) atomicAdd(overflow, 1ull);
        top = 0;
        break;
      }
      if (left_too) stack[top + __popcll(m_left & below)] = b_first == split ? ~split : split;                              // lbvh_left_ref
      if (kids) stack[top + n_left + __popcll(m_open & below)] = b_last == split + 1 ? ~(split + 1) : split + 1;  // lbvh_right_ref
      top += n_left + n_right;
      db_wave_sync();
      DB_LAP(3);
    }
    if (__ballot(waiting > 0) != 0ull) settle();
    if (timing && lane == 0 && a.pk_diag) {
      float ext = 0.f;
      for (int c = 0; c < 3; c++) ext = fmaxf(ext, fmaxf(u_hi[0][c], u_hi[kDbBoxes - 1][c]) - fminf(u_lo[0][c], u_lo[kDbBoxes - 1][c]));
      int32_t *d = a.pk_diag + packet * 4;
      d[0] = (int32_t)(__builtin_amdgcn_s_memtime() - packet_t0), d[1] = (int32_t)(ext * 1e6f), d[2] = (int32_t)(tm[5] - pk_rounds0), d[3] = (int32_t)(tm[6] - pk_settles0);
    }
    if (timing && lane == 0) {  // the longest packet, and how many take more than twice / four times 2^20 ticks
      const unsigned long long el = __builtin_amdgcn_s_memtime() - packet_t0;
      atomicMax(&a.diag_out[12], el);
      if (el > (1ull << 20)) atomicAdd(&a.diag_out[10], 1ull);
      if (el > (1ull << 21)) atomicAdd(&a.diag_out[11], 1ull);
    }
    if (timing) {
      uint32_t lw = pk_long, pt = point_tests - pk_points0;
      for (int off = 32; off > 0; off >>= 1) lw += __shfl_xor(lw, off), pt += __shfl_xor(pt, off);
      const unsigned long long el = __builtin_amdgcn_s_memtime() - packet_t0;
      if (lane == 0 && el > (1ull << 21)) {
        atomicAdd(&a.diag_out[16], tm[5] - pk_rounds0), atomicAdd(&a.diag_out[17], tm[6] - pk_settles0);
        atomicAdd(&a.diag_out[18], (unsigned long long)lw), atomicAdd(&a.diag_out[19], (unsigned long long)pt);
        atomicAdd(&a.diag_out[9], tm[2] - pk_settle_t0);
      }
    }
  }
  if (timing && lane == 0) {
    for (int i = 0; i < 8; i++) atomicAdd(&a.diag_out[i], tm[i]);
    const unsigned long long el = __builtin_amdgcn_s_memtime() - wave_t0;  // how evenly the packets fill the waves: mean / longest wave
    atomicAdd(&a.diag_out[13], el), atomicMax(&a.diag_out[14], el), atomicAdd(&a.diag_out[15], 1ull);
  }
#undef DB_LAP
  if (a.diag & 8) {  // most walk steps of a wave, their sum
    if (lane == 0) {
      atomicMax(&a.stats[kDbStatLongestWalk], (unsigned long long)node_tests);
      atomicAdd(&a.stats[kDbStatWalkSum], (unsigned long long)node_tests);
    }
  }
  db_add_stats_wave(a.stats + kDbStatUnion, node_tests, point_tests);  // (no LDS words: 16 384 bytes per workgroup are ten workgroups per CU, 16 400 are nine)
}

}  // namespace

void Engine::DbCall::unions() {
  OWLMI_HIP(hipEventRecord(e.ev_d_, s));
  hipLaunchKernelGGL(db_union_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a);
  OWLMI_HIP(hipEventRecord(e.ev_e_, s));
  OWLMI_HIP(hipMemsetAsync(a.min_row, 0x7f, (size_t)n * sizeof(int32_t), s));  // 0x7f7f7f7f: above every row (group_unions: db_group_kernel)
}
void Engine::DbCall::group_unions() {
  // per-slot group references where the ranks go afterwards, the list itself (slot order = curve order: neighbours in
  // the list are neighbours in space) where the root flags go (db_workspace.h); its length, the stack overflows and the
  // XCDs' cursors in the counter array, all zero since the call's first memset
  int32_t *group_at = a.rank, *groups = roots;
  unsigned long long *n_groups = e.counters_ + kDbGroups, *overflows = e.counters_ + kDbOverflows, *cursors = e.counters_ + kDbCursors;
  a.chunk = knobs.chunk, a.short_way = knobs.short_way, a.scan_budget = knobs.scan_budget;
  hipLaunchKernelGGL(db_group_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, group_at, uni, a.min_row, block_places);
  exclusive_sum(block_places, block_places + blocks, (int)blocks);
  hipLaunchKernelGGL(db_group_list_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, group_at, block_places + blocks, groups, n_groups);
  // persistent lanes: as many workgroups as the device holds at once (the list's length is known on the device only)
  // (per engine: the CU count and the occupancy are those of THIS engine's device)
  if (e.db_union_resident_ == 0) {
    int per_cu = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, e.device_) != hipSuccess) {
      e.db_union_resident_ = 256 * 4;
    } else {
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void *)db_group_union_kernel, kDbUnionBlock, 0) != hipSuccess) per_cu = 4;
      // nine workgroups = 18 waves per CU are what fits (16 KB of LDS per workgroup = 13 granules of 1 280 bytes: the occupancy
      // query says ten).  BASELINE config 3, both passes, since the packet cursors have cache lines of their own (round 4):
      // 1.46 / 1.34 / 1.25 ms with seven / eight / nine; ten (a build with seven buffered unions per lane: 12 granules) 1.27
      // (TKNN_DB_PER_CU: measurements)
      e.db_union_resident_ = prop.multiProcessorCount * std::max(1, std::min(per_cu, getenv("TKNN_DB_PER_CU") ? atoi(getenv("TKNN_DB_PER_CU")) : 9));
    }
  }
  const unsigned resident = (unsigned)e.db_union_resident_;
  const unsigned grid = (unsigned)std::max(1, std::min((int)(blocks < resident ? blocks : resident), knobs.grid));
  // Two passes: first the pairs of groups that (nearly) touch -- in a dense region their probes hit at once, and when the
  // pass is over a cluster's groups are one set --, then the pairs further apart, nearly all of which then are in one
  // set already and cost a parent read instead of a probe that would have to look at many point pairs to find one close
  // enough (or none).  One pass settles everything as soon as it is met: 4 times the point tests, 14 ms instead of 4.
  const float split = knobs.split;
  // ONE number bounds both passes: pass 1 takes near2 <= near_hi2, pass 2 near2 > that same value, and the per-axis
  // reach of a pass's box prefilter is derived from its near_hi2 (>= its square root, DbArgs), so that no pair whose
  // faces are between split * eps_wide and sqrt(near_hi2) apart along one axis falls between the passes
  // (reach = split * eps (1 + 1e-6) against near2 <= split^2 eps^2 (1 + 1e-5) left a 34-ulp window).
  if (a.pk_diag) OWLMI_HIP(hipMemsetAsync(a.pk_diag, 0, DbClusterWs::max_packets((size_t)n) * 16, s));
  a.near_lo2 = -1.f;
  a.near_hi2 = split * split * a.eps_out2;
  a.reach = db_reach_of(a.near_hi2);
  OWLMI_HIP(hipEventRecord(e.ev_d_, s));
  if (split < 1.f) {
    union_launches = 2;
    hipLaunchKernelGGL(db_group_union_kernel, dim3(grid), dim3(kDbUnionBlock), 0, s, a, groups, n_groups, cursors, overflows);
    OWLMI_HIP(hipMemsetAsync(cursors, 0, 8 * kDbCursorStride * sizeof(unsigned long long), s));
    a.near_lo2 = a.near_hi2;
    OWLMI_HIP(hipEventRecord(e.ev_g_, s));
    between_passes = true;  // ev_g_ .. ev_h_: the cursors' reset and db_uniform_kernel, not part of union_ms
    if (n > 1 && knobs.uniform) {
      // which nodes hold one set only, now that the groups that touch are united
      a.uni = uni;          // (filled by db_group_kernel)
      a.uni_leaf = a.rank;  // (the list kernel has used the per-slot group references up)
      a.split_owner = e.bvh_.split_owner_device();
      hipLaunchKernelGGL(db_uniform_kernel, dim3(blocks), dim3(kDbBlock), 0, s, a, groups, n_groups);
    }
    OWLMI_HIP(hipEventRecord(e.ev_h_, s));
  }
  a.near_hi2 = a.eps_out2;
  a.reach = db_reach_of(a.near_hi2);
  hipLaunchKernelGGL(db_group_union_kernel, dim3(grid), dim3(kDbUnionBlock), 0, s, a, groups, n_groups, cursors, overflows);
  OWLMI_HIP(hipEventRecord(e.ev_e_, s));
}
// the waves of db_group_union_kernel the device holds at once (print_diagnostics)
int Engine::DbCall::union_waves() const { return e.db_union_resident_ * (kDbUnionBlock / 64); }
}  // namespace owlmi
