// orient.hip -- consistent orientation of the built set's normals without a viewpoint (tknnOrientNormals,
// include/owlknn_orient.h): the minimum spanning forest of an EXPLICIT edge list under the strict key (bits of the fp32 weight,
// min name, max name), with the sign parity of the path to the root carried through the merges.  tests/orient_spec.py is the
// same in numpy.
//
// Vertices are the caller's ROWS.  The graph comes from the engine's own calls: the own-points rows of tknnKnn at k and, unless
// switched off, the records of the Euclidean tknnEmst (both name their points; or_row_of turns a name into a row).
//   or_prepare_kernel:   per sorted slot: the row's name, whether it is eligible, its root key t, and the round state.
//   or_emit_kernel:      one candidate per kNN entry and per EMST record: (lo name << 32 | hi name, bits of w); an entry that is
//                        no edge gets the key that sorts last.
//   two stable radix sorts (the pair, then the weight bits: emst.hip's order of its records), or_flag_kernel, a scan,
//   or_rank_kernel:      the place of an edge among the distinct edges of the sorted list is its RANK in the key.  From here on an
//                        edge is its rank: comparing two edges is comparing two uint32, and the 94-bit key never has to fit an
//                        atomic.  Per rank: both rows, the sign bit s in the top bit of the second, its place in the sorted list.
// One Boruvka round over the list of the ranks still alive:
//   or_min_kernel:       an edge whose ends lie in two components offers its rank to both (atomicMin); one inside a component is
//                        dead and flagged for the next order-preserving select (run when a quarter of the list has died).
//   or_hook_kernel:      every representative with a best edge hooks onto the component at the other end; of a mutual pair --
//                        under a strict order the only cycles there are -- the smaller representative stays.  The hooking
//                        component records the edge, so it is recorded once.
//   or_jump_kernel:      pointer jumping over the representatives' links.
//   or_relabel_kernel:   comp[v] and sigma[v] take the link of v's old representative, together.
// PARITY.  sigma[v] is the parity of the s bits on the tree path from v to its representative.  A hook of c through the edge
// (a, b), a in c, gives c the offset sigma[a] ^ s ^ sigma[b] -- the path from c's representative to a, the edge, b to its
// representative.  A link is ONE word, (target << 1) | offset: whatever a jump reads is a true (ancestor, parity to it) of its
// moment, a stale one costs a step and no more, and composing two is an XOR.  No rooted tree is ever built.
// The finish: the root of a component is its arg-max of t in two 32-bit passes (atomicMax of the order-preserving bits, then
// atomicMin of the row among those that hold the maximum), flip[v] = sigma[v] ^ sigma[root] ^ rootflip; the recorded ranks are
// selected in order, which is the key's, and written with the tail filled.
// Nothing the caller can see is written before the rounds have ended.  32-bit integer atomics only; no loop waits for a thread.
#include "linkage.h"  // DeviceBuffer, jump_passes
#include "trueknn_engine.h"
#include "owlknn_orient.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kOrBlock = 256;
constexpr int kOrJumpSteps = 16;
constexpr uint32_t kOrNone = 0xffffffffu;            // best[c]: no edge; a dropped candidate's weight
constexpr unsigned long long kOrNoPair = ~0ull;
constexpr uint32_t kOrSign = 0x80000000u;
// the call's words (uint32), in kOrStripes stripes of kOrStripeWords: eligible points, edges recorded so far, edges found dead over
// all rounds, flipped rows (a wave adds to the stripe of its index, the host sums them: a round's million waves do not queue at one
// word); in the first stripe alone the distinct edges and the selects' counts
constexpr int kOrEligible = 0, kOrEdges = 1, kOrDead = 2, kOrFlipped = 3, kOrDistinct = 4, kOrSelected = 5, kOrStripeWords = 8, kOrStripes = 32,
              kOrWords = kOrStripes * kOrStripeWords;
static_assert(kHostCounterWords * sizeof(unsigned long long) >= kOrWords * sizeof(uint32_t), "the host's copy of the counters holds the call's words");

struct OrientArgs {
  LbvhView bvh;
  int32_t n, k, ids;
  int64_t knn_slots, slots;  // n * k; with the EMST's records
  float dx, dy, dz;
  const float *normals;
  const int32_t *knn_idx, *emst_u, *emst_v;
  // per row
  int32_t *name;
  const uint32_t *sorted_name;  // with ids: the names ascending, and their rows
  const int32_t *sorted_row;
  uint8_t *elig, *sigma;
  int32_t *comp;
  uint32_t *link, *best, *tbits, *tmax, *root_row, *min_row, *base;
  // per candidate
  unsigned long long *pair;
  uint32_t *w;
  int32_t *flag, *rank;
  // per rank
  int32_t *eu;
  uint32_t *ev;   // the second row | s << 31
  uint32_t *pos;  // the edge's place in the sorted list
  uint8_t *in_tree;
  // the list of the ranks alive
  uint32_t *alive;
  uint8_t *keep;
  uint32_t *words;
};

__device__ __forceinline__ unsigned long long or_pair(int32_t a, int32_t b) {
  const uint32_t x = (uint32_t)a, y = (uint32_t)b;
  return x < y ? ((unsigned long long)x << 32) | y : ((unsigned long long)y << 32) | x;
}

__device__ __forceinline__ uint32_t or_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the row of the point named `name`, -1 if there is none
__device__ __forceinline__ int32_t or_row_of(const OrientArgs &a, int32_t name) {
  if (!a.ids) return name >= 0 && name < a.n ? name : -1;
  const uint32_t want = (uint32_t)name;
  int32_t lo = 0, hi = a.n;  // the first entry >= want
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    if (a.sorted_name[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo < a.n && a.sorted_name[lo] == want ? a.sorted_row[lo] : -1;
}

// c of the rows i and j (this file is compiled without contraction)
__device__ __forceinline__ float or_dot(const float *__restrict__ nrm, int32_t i, int32_t j) {
  const float *p = nrm + (size_t)i * 3, *q = nrm + (size_t)j * 3;
  return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2];
}

// order-preserving bits of a float that is no NaN; -0 counts as +0
__device__ __forceinline__ uint32_t or_ordered(float t) {
  const uint32_t u = __float_as_uint(t == 0.f ? 0.f : t);
  return (u & kOrSign) ? ~u : (u | kOrSign);
}

// words[at] += the lanes of the wave with `on` (every lane calls)
__device__ __forceinline__ void or_count(bool on, uint32_t *words, int at) {
  const unsigned long long m = __ballot(on);
  if ((threadIdx.x & 63) == 0 && m)
    atomicAdd(words + ((blockIdx.x * (kOrBlock / 64) + (threadIdx.x >> 6)) & (kOrStripes - 1)) * kOrStripeWords + at, (uint32_t)__popcll(m));
}

// ---- before the sort ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kOrBlock) or_prepare_kernel(OrientArgs a, uint32_t *__restrict__ name_key, int32_t *__restrict__ row_val) {
  const int32_t t = blockIdx.x * kOrBlock + threadIdx.x;
  bool ok = false;
  if (t < a.n) {
    const LbvhPoint p = a.bvh.points[t];
    const int32_t row = a.bvh.prim_id[t];
    const float *nr = a.normals + (size_t)row * 3;
    const float inf = __uint_as_float(0x7f800000u);
    ok = p.x == p.x && p.y == p.y && p.z == p.z && fabsf(nr[0]) < inf && fabsf(nr[1]) < inf && fabsf(nr[2]) < inf;  // (a NaN fails)
    float key = (p.x * a.dx + p.y * a.dy) + p.z * a.dz;
    if (!(key == key)) key = -inf;
    a.name[row] = p.id;
    if (name_key) name_key[t] = (uint32_t)p.id, row_val[t] = row;
    a.elig[row] = ok;
    a.sigma[row] = 0;
    a.comp[row] = ok ? row : -1;
    a.link[row] = (uint32_t)row << 1;
    a.best[row] = kOrNone;
    a.tbits[row] = or_ordered(key);
  }
  or_count(ok, a.words, kOrEligible);
}

__global__ void __launch_bounds__(kOrBlock) or_emit_kernel(OrientArgs a) {
  const int64_t e = (int64_t)blockIdx.x * kOrBlock + threadIdx.x;
  if (e >= a.slots) return;
  int32_t i = -1, j = -1, ni = -1, nj = -1;
  if (e < a.knn_slots) {
    i = (int32_t)(e / a.k);
    ni = a.name[i];
    nj = a.knn_idx[e];
    j = nj >= 0 ? or_row_of(a, nj) : -1;
  } else {
    const int64_t r = e - a.knn_slots;
    ni = a.emst_u[r], nj = a.emst_v[r];
    i = ni >= 0 ? or_row_of(a, ni) : -1;
    j = nj >= 0 ? or_row_of(a, nj) : -1;
  }
  unsigned long long pair = kOrNoPair;
  uint32_t wb = kOrNone;
  if (i >= 0 && j >= 0 && i != j && a.elig[i] && a.elig[j]) {
    const float c = or_dot(a.normals, i, j);
    wb = __float_as_uint(fmaxf(1.0f - fabsf(c), 0.0f)) & ~kOrSign;  // (never negative: the mask turns a -0 into +0)
    pair = or_pair(ni, nj);
  }
  a.pair[e] = pair;
  a.w[e] = wb;
}

// ---- after the sort: distinct edges and their ranks -------------------------------------------------------------------------------
__global__ void __launch_bounds__(kOrBlock) or_flag_kernel(OrientArgs a) {
  const int64_t e = (int64_t)blockIdx.x * kOrBlock + threadIdx.x;
  if (e >= a.slots) return;
  // (one pair has one weight -- c is bitwise symmetric --, so its copies lie side by side)
  a.flag[e] = a.w[e] != kOrNone && (e == 0 || a.pair[e - 1] != a.pair[e]);
}

__global__ void __launch_bounds__(kOrBlock) or_rank_kernel(OrientArgs a, uint32_t *__restrict__ alive) {
  const int64_t e = (int64_t)blockIdx.x * kOrBlock + threadIdx.x;
  if (e >= a.slots) return;
  if (e == a.slots - 1) a.words[kOrDistinct] = (uint32_t)(a.rank[e] + a.flag[e]);
  if (!a.flag[e]) return;
  const int32_t r = a.rank[e];
  const unsigned long long pair = a.pair[e];
  const int32_t i = or_row_of(a, (int32_t)(uint32_t)(pair >> 32)), j = or_row_of(a, (int32_t)(uint32_t)pair);  // (both there: or_emit_kernel found them)
  const uint32_t s = or_dot(a.normals, i, j) < 0.f;
  a.eu[r] = i;
  a.ev[r] = (uint32_t)j | (s << 31);
  a.pos[r] = (uint32_t)e;
  a.in_tree[r] = 0;
  alive[r] = (uint32_t)r;
}

// ---- one round ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kOrBlock) or_min_kernel(OrientArgs a, int32_t count) {
  const int32_t t = blockIdx.x * kOrBlock + threadIdx.x;
  bool dead = false;
  if (t < count) {
    const uint32_t r = a.alive[t];
    const int32_t cu = a.comp[a.eu[r]], cv = a.comp[a.ev[r] & ~kOrSign];
    dead = cu == cv;
    a.keep[t] = !dead;
    if (!dead) {
      // (a late round has few components: the plain load spares most of the atomics that would queue at one word)
      if (or_load(a.best + cu) > r) atomicMin(a.best + cu, r);
      if (or_load(a.best + cv) > r) atomicMin(a.best + cv, r);
    }
  }
  or_count(dead, a.words, kOrDead);
}

__global__ void __launch_bounds__(kOrBlock) or_hook_kernel(OrientArgs a) {
  const int32_t v = blockIdx.x * kOrBlock + threadIdx.x;
  bool hooks = false;
  if (v < a.n && a.comp[v] == v) {
    const uint32_t r = a.best[v];
    if (r != kOrNone) {
      const int32_t p = a.eu[r];
      const uint32_t qs = a.ev[r];
      const int32_t q = (int32_t)(qs & ~kOrSign), cp = a.comp[p], cq = a.comp[q];
      const int32_t other = cp == v ? cq : cp;
      hooks = a.best[other] != r || v > other;  // of a mutual pair the smaller representative stays
      if (hooks) {
        a.link[v] = ((uint32_t)other << 1) | (((uint32_t)(a.sigma[p] ^ a.sigma[q]) & 1u) ^ (qs >> 31));
        a.in_tree[r] = 1;
      }
    }
  }
  or_count(hooks, a.words, kOrEdges);
}

// link[v] = the link of the farthest ancestor reached in kOrJumpSteps steps, parities composed.  In place: a link read here is a
// (target, parity) that was true when it was written, and every target is an ancestor on v's chain.
__global__ void __launch_bounds__(kOrBlock) or_jump_kernel(OrientArgs a) {
  const int32_t v = blockIdx.x * kOrBlock + threadIdx.x;
  if (v >= a.n || a.comp[v] != v) return;
  uint32_t l = or_load(a.link + v);
  if ((l >> 1) == (uint32_t)v) return;
#pragma unroll 1
  for (int step = 0; step < kOrJumpSteps; step++) {
    const uint32_t up = or_load(a.link + (l >> 1));
    if ((up >> 1) == (l >> 1)) break;
    l = (up & ~1u) | ((l ^ up) & 1u);
  }
  __hip_atomic_store(a.link + v, l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kOrBlock) or_relabel_kernel(OrientArgs a) {
  const int32_t v = blockIdx.x * kOrBlock + threadIdx.x;
  if (v >= a.n) return;
  const int32_t c = a.comp[v];
  a.best[v] = kOrNone;
  if (c < 0) return;
  const uint32_t l = a.link[c];  // (c's link ends at a representative that stayed: no kernel of this launch writes links)
  a.comp[v] = (int32_t)(l >> 1);
  a.sigma[v] ^= (uint8_t)(l & 1u);
}

// ---- the finish --------------------------------------------------------------------------------------------------------------------
// table[c] = max (kMax) or min of itself and v, for the lanes with `has`, every lane of the wave calling: the lanes of one component
// reduce among themselves and their first lane sends one atomic, none when a plain load shows that it would change nothing
// (emst.hip's em_group_min).  At the finish a connected set is ONE component: without this every row would queue at one word.
template <bool kMax>
__device__ __forceinline__ void or_group_best(bool has, int32_t c, uint32_t v, uint32_t *table) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(has);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int32_t lc = __shfl(c, leader);
    const bool mine = has && c == lc;
    const unsigned long long group = __ballot(mine);
    uint32_t m = mine ? v : (kMax ? 0u : kOrNone);
    if (group & (group - 1)) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(m, off);
        m = kMax ? (o > m ? o : m) : (o < m ? o : m);
      }
    }
    if (lane == leader) {
      const uint32_t now = or_load(table + lc);
      if (kMax ? now < m : now > m) kMax ? atomicMax(table + lc, m) : atomicMin(table + lc, m);
    }
    todo &= ~group;
  }
}

__global__ void __launch_bounds__(kOrBlock) or_tmax_kernel(OrientArgs a) {
  const int32_t v = blockIdx.x * kOrBlock + threadIdx.x;
  const int32_t c = v < a.n ? a.comp[v] : -1;
  or_group_best<true>(c >= 0, c, c >= 0 ? a.tbits[v] : 0u, a.tmax);
}
__global__ void __launch_bounds__(kOrBlock) or_root_kernel(OrientArgs a) {
  const int32_t v = blockIdx.x * kOrBlock + threadIdx.x;
  const int32_t c = v < a.n ? a.comp[v] : -1;
  or_group_best<false>(c >= 0, c, (uint32_t)v, a.min_row);
  or_group_best<false>(c >= 0 && a.tbits[v] == a.tmax[c], c, (uint32_t)v, a.root_row);
}
// base[c] = sigma[root] ^ rootflip, read from the INPUT normals before any is rewritten (the output may lie over them)
__global__ void __launch_bounds__(kOrBlock) or_base_kernel(OrientArgs a) {
  const int32_t v = blockIdx.x * kOrBlock + threadIdx.x;
  if (v >= a.n) return;
  const int32_t c = a.comp[v];
  if (c < 0 || a.root_row[c] != (uint32_t)v) return;
  const float *nr = a.normals + (size_t)v * 3;
  const uint32_t rootflip = (nr[0] * a.dx + nr[1] * a.dy) + nr[2] * a.dz < 0.f;
  a.base[c] = (uint32_t)a.sigma[v] ^ rootflip;
}
__global__ void __launch_bounds__(kOrBlock) or_apply_kernel(OrientArgs a, float *out_normals, uint8_t *__restrict__ out_flip, int32_t *__restrict__ out_component) {
  const int32_t v = blockIdx.x * kOrBlock + threadIdx.x;
  bool flip = false;
  if (v < a.n) {
    const int32_t c = a.comp[v];
    flip = c >= 0 && (((uint32_t)a.sigma[v] ^ a.base[c]) & 1u);
    if (out_flip) out_flip[v] = flip;
    if (out_component) out_component[v] = c >= 0 ? (int32_t)a.min_row[c] : -1;
    if (out_normals) {  // (this row's three words are read and written by this lane alone: in place is the same)
      const uint32_t *in = (const uint32_t *)a.normals + (size_t)v * 3;
      uint32_t *out = (uint32_t *)out_normals + (size_t)v * 3;
      const uint32_t toggle = flip ? kOrSign : 0u, x = in[0], y = in[1], z = in[2];
      out[0] = x ^ toggle, out[1] = y ^ toggle, out[2] = z ^ toggle;
    }
  }
  or_count(flip, a.words, kOrFlipped);
}

// T's records in key order: the selected ranks ascend
__global__ void __launch_bounds__(kOrBlock) or_output_kernel(OrientArgs a, const uint32_t *__restrict__ selected, int32_t edges, int32_t rows, int32_t *__restrict__ out_u,
                                                            int32_t *__restrict__ out_v, float *__restrict__ out_w) {
  const int32_t i = blockIdx.x * kOrBlock + threadIdx.x;
  if (i >= rows) return;
  const bool edge = i < edges;
  const uint32_t at = edge ? a.pos[selected[i]] : 0u;
  const unsigned long long p = edge ? a.pair[at] : kOrNoPair;
  if (out_u) out_u[i] = edge ? (int32_t)(uint32_t)(p >> 32) : -1;
  if (out_v) out_v[i] = edge ? (int32_t)(uint32_t)p : -1;
  if (out_w) out_w[i] = __uint_as_float(edge ? a.w[at] : 0x7f800000u);
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

}  // namespace

void Engine::orient_normals(const tknnOrientOptions &o, tknnOrientInfo *info, hipStream_t s) {
  const LbvhView tv = bvh_.view();
  const int64_t n = tv.n, k = o.k;
  const bool with_emst = !(o.flags & TKNN_ORIENT_NO_EMST);
  const int64_t knn_slots = n * k, slots = knn_slots + (with_emst ? n - 1 : 0);
  int bound = 1;  // ceil(log2 n) + 1
  while ((1ll << (bound - 1)) < n) bound++;
  const int max_rounds = o.max_rounds > 0 ? std::min<int>(o.max_rounds, bound) : bound;
  const dim3 block(kOrBlock);
  auto grid = [](int64_t items) { return dim3((unsigned)((std::max<int64_t>(items, 1) + kOrBlock - 1) / kOrBlock)); };
  tknnOrientInfo out;
  std::memset(&out, 0, sizeof out);
  Event t0, t1, t2, t3, t4;
  t0.record(s);

  // ---- 1. the two inner calls.  They take the engine's workspace, so what must outlive them is allocated for this call.
  DeviceBuffer knn_idx((size_t)knn_slots * sizeof(int32_t)), emst_u((size_t)(with_emst ? n - 1 : 0) * sizeof(int32_t)),
      emst_v((size_t)(with_emst ? n - 1 : 0) * sizeof(int32_t));
  {
    tknnKnnOptions ko;
    std::memset(&ko, 0, sizeof ko);
    ko.m = n, ko.k = (int32_t)k;
    ko.d_idx = (int32_t *)knn_idx.p;
    tknnKnnInfo knn_info;
    std::memset(&knn_info, 0, sizeof knn_info);
    knn(ko, &knn_info, s);
    out.knn_ms = knn_info.solve_ms;
  }
  if (with_emst && n > 1) {
    tknnEmstOptions eo;
    std::memset(&eo, 0, sizeof eo);
    eo.d_u = (int32_t *)emst_u.p, eo.d_v = (int32_t *)emst_v.p;
    tknnEmstInfo emst_info;
    std::memset(&emst_info, 0, sizeof emst_info);
    emst(eo, &emst_info, s);
    out.emst_ms = emst_info.solve_ms;
  }
  OWLMI_HIP(hipStreamSynchronize(s));  // (the workspace is laid out anew below)
  t1.record(s);

  // ---- the call's workspace: words | columns of a word per row | bytes per row | per candidate | per rank | the sorts' space
  auto align = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t tmp_bytes = 0;
  {
    size_t b = 0;
    unsigned long long *k64 = nullptr;
    uint32_t *k32 = nullptr;
    int32_t *i32 = nullptr;
    uint8_t *f8 = nullptr;
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, b, k64, k64, k32, k32, (int)slots, 0, 64, s));
    tmp_bytes = std::max(tmp_bytes, b);
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, b, k32, k32, k64, k64, (int)slots, 0, 32, s));
    tmp_bytes = std::max(tmp_bytes, b);
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, b, k32, k32, i32, i32, (int)n, 0, 32, s));
    tmp_bytes = std::max(tmp_bytes, b);
    OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, b, i32, i32, (int)slots, s));
    tmp_bytes = std::max(tmp_bytes, b);
    OWLMI_HIP(hipcub::DeviceSelect::Flagged(nullptr, b, k32, f8, k32, k32, (int)slots, s));
    tmp_bytes = std::max(tmp_bytes, b);
    OWLMI_HIP(hipcub::DeviceSelect::Flagged(nullptr, b, hipcub::CountingInputIterator<uint32_t>(0u), f8, k32, k32, (int)slots, s));
    tmp_bytes = std::max(tmp_bytes, b);
  }
  const size_t words_b = align(kOrWords * sizeof(uint32_t)), col_b = align((size_t)n * sizeof(uint32_t)), byte_b = align((size_t)n),
               cand_b = align((size_t)slots * sizeof(uint32_t)), wide_b = align((size_t)slots * sizeof(unsigned long long)), cbyte_b = align((size_t)slots);
  constexpr int kCols = 13;
  char *ws = (char *)workspace(words_b + kCols * col_b + 2 * byte_b + 2 * wide_b + 5 * cand_b + 2 * cbyte_b + align(tmp_bytes));
  char *at = ws;
  auto take = [&](size_t bytes) {
    char *p = at;
    at += bytes;
    return p;
  };
  OrientArgs a;
  std::memset(&a, 0, sizeof a);
  a.bvh = tv;
  a.n = (int32_t)n, a.k = (int32_t)k, a.ids = ids_given_;
  a.knn_slots = knn_slots, a.slots = slots;
  a.dx = o.direction[0], a.dy = o.direction[1], a.dz = o.direction[2];
  a.normals = o.d_normals;
  a.knn_idx = (const int32_t *)knn_idx.p, a.emst_u = (const int32_t *)emst_u.p, a.emst_v = (const int32_t *)emst_v.p;
  a.words = (uint32_t *)take(words_b);
  a.name = (int32_t *)take(col_b);
  uint32_t *name_key = (uint32_t *)take(col_b), *sorted_name = (uint32_t *)take(col_b);
  int32_t *row_val = (int32_t *)take(col_b), *sorted_row = (int32_t *)take(col_b);
  a.sorted_name = sorted_name, a.sorted_row = sorted_row;
  a.comp = (int32_t *)take(col_b);
  a.link = (uint32_t *)take(col_b);
  a.best = (uint32_t *)take(col_b);
  a.tbits = (uint32_t *)take(col_b);
  a.tmax = (uint32_t *)take(col_b);
  a.root_row = (uint32_t *)take(col_b);
  a.min_row = (uint32_t *)take(col_b);
  a.base = (uint32_t *)take(col_b);
  a.elig = (uint8_t *)take(byte_b);
  a.sigma = (uint8_t *)take(byte_b);
  unsigned long long *pair_a = (unsigned long long *)take(wide_b), *pair_b = (unsigned long long *)take(wide_b);
  uint32_t *w_a = (uint32_t *)take(cand_b), *w_b = (uint32_t *)take(cand_b);
  a.eu = (int32_t *)take(cand_b);
  a.ev = (uint32_t *)take(cand_b);
  a.pos = (uint32_t *)take(cand_b);
  a.in_tree = (uint8_t *)take(cbyte_b);
  a.keep = (uint8_t *)take(cbyte_b);
  void *tmp = take(align(tmp_bytes));
  a.pair = pair_a, a.w = w_a;
  // once the sorts are done their second buffers are free: the flags lie in w_b, the scan in the lower half of pair_b and the
  // first list of ranks in its upper half; the second list takes w_b when the flags are done with, the selected ranks the scan's
  a.flag = (int32_t *)w_b;
  a.rank = (int32_t *)pair_b;
  uint32_t *alive_a = (uint32_t *)pair_b + slots, *alive_b = w_b, *selected = (uint32_t *)pair_b;

  uint32_t *h = (uint32_t *)h_counters_;
  auto read_words = [&]() {
    OWLMI_HIP(hipMemcpyAsync(h, a.words, kOrWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
  };
  auto sum = [&](int at) {
    int64_t total = 0;
    for (int j = 0; j < kOrStripes; j++) total += h[j * kOrStripeWords + at];
    return total;
  };

  // ---- 2., 3. candidates, the sort, ranks
  OWLMI_HIP(hipMemsetAsync(a.words, 0, kOrWords * sizeof(uint32_t), s));
  hipLaunchKernelGGL(or_prepare_kernel, grid(n), block, 0, s, a, ids_given_ ? name_key : (uint32_t *)nullptr, row_val);
  if (ids_given_) OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, name_key, sorted_name, row_val, sorted_row, (int)n, 0, 32, s));
  hipLaunchKernelGGL(or_emit_kernel, grid(slots), block, 0, s, a);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, pair_a, pair_b, w_a, w_b, (int)slots, 0, 64, s));
  OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, w_b, w_a, pair_b, pair_a, (int)slots, 0, 32, s));
  hipLaunchKernelGGL(or_flag_kernel, grid(slots), block, 0, s, a);
  OWLMI_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tmp_bytes, a.flag, a.rank, (int)slots, s));
  hipLaunchKernelGGL(or_rank_kernel, grid(slots), block, 0, s, a, alive_a);
  OWLMI_HIP(hipGetLastError());
  read_words();
  const int64_t eligible = sum(kOrEligible), distinct = h[kOrDistinct];
  t2.record(s);

  // ---- 4., 5. the rounds
  int64_t edges = 0, added = 0, alive = distinct, dead = 0, dead_before = 0;  // dead: in the last round; dead_before: over all rounds
  int rounds = 0;
  a.alive = alive_a;
  uint32_t *spare_list = alive_b;
  while (eligible - edges > 1 && alive > 0 && rounds < max_rounds) {
    if (dead * 4 >= alive) {  // the flags of the round before: what was dead then stays dead
      OWLMI_HIP(hipcub::DeviceSelect::Flagged(tmp, tmp_bytes, a.alive, a.keep, spare_list, a.words + kOrSelected, (int)alive, s));
      std::swap(spare_list, a.alive);
      alive -= dead;
      if (alive == 0) break;
    }
    hipLaunchKernelGGL(or_min_kernel, grid(alive), block, 0, s, a, (int32_t)alive);
    hipLaunchKernelGGL(or_hook_kernel, grid(n), block, 0, s, a);
    for (int p = 0, passes = jump_passes(eligible - edges); p < passes; p++) hipLaunchKernelGGL(or_jump_kernel, grid(n), block, 0, s, a);
    hipLaunchKernelGGL(or_relabel_kernel, grid(n), block, 0, s, a);
    OWLMI_HIP(hipGetLastError());
    read_words();
    rounds++;
    added = sum(kOrEdges) - edges;
    edges += added;
    dead = sum(kOrDead) - dead_before;
    dead_before += dead;
    if (added == 0) break;
  }
  const bool unfinished = eligible - edges > 1 && alive > 0 && added > 0 && rounds >= max_rounds;  // the bound cut the rounds short
  t3.record(s);
  if (unfinished) throw RoundsExceeded{};

  // ---- 6. the finish
  OWLMI_HIP(hipMemsetAsync(a.tmax, 0, (size_t)n * sizeof(uint32_t), s));
  OWLMI_HIP(hipMemsetAsync(a.root_row, 0xff, (size_t)n * sizeof(uint32_t), s));
  OWLMI_HIP(hipMemsetAsync(a.min_row, 0xff, (size_t)n * sizeof(uint32_t), s));
  hipLaunchKernelGGL(or_tmax_kernel, grid(n), block, 0, s, a);
  hipLaunchKernelGGL(or_root_kernel, grid(n), block, 0, s, a);
  hipLaunchKernelGGL(or_base_kernel, grid(n), block, 0, s, a);
  hipLaunchKernelGGL(or_apply_kernel, grid(n), block, 0, s, a, o.d_out_normals, o.d_flip, o.d_component);
  OWLMI_HIP(hipGetLastError());
  if (n > 1 && (o.d_u || o.d_v || o.d_w)) {
    if (edges > 0)
      OWLMI_HIP(hipcub::DeviceSelect::Flagged(tmp, tmp_bytes, hipcub::CountingInputIterator<uint32_t>(0u), a.in_tree, selected, a.words + kOrSelected, (int)distinct, s));
    hipLaunchKernelGGL(or_output_kernel, grid(n - 1), block, 0, s, a, (const uint32_t *)selected, (int32_t)edges, (int32_t)(n - 1), o.d_u, o.d_v, o.d_w);
    OWLMI_HIP(hipGetLastError());
  }
  t4.record(s);
  read_words();
  out.candidates = slots;
  out.tree_edges = edges;
  out.components = eligible - edges;
  out.excluded = n - eligible;
  out.flipped = sum(kOrFlipped);
  out.rounds = rounds;
  out.solve_ms = between(t0, t4);
  out.sort_ms = between(t1, t2);
  out.forest_ms = between(t2, t3);
  out.apply_ms = between(t3, t4);
  if (info) *info = out;
}

}  // namespace owlmi
