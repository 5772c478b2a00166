// team_lanes.h -- what a 16-lane team of the TrueKNN kernels is made of: the lane exchanges, the sorting networks and the
// merge of buffered candidates into a team's sorted register list.  Shared by the team kernels (trueknn_team.hip, trueknn_tail.hip, trueknn_bigk.hip) and the
// kernel for query points that are not in the tree (trueknn_query.hip); every function is inlined into its caller.  What a
// team does with these lanes when it walks the box pyramid for one query is team_walk.h, on top of this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "knn_device.h"
#include "owl/lbvh_device.h"

namespace owlmi {

namespace {

// per team (every list size since round 3): candidates that passed the gate since the last merge into the team's sorted list, as
// 64-bit (dist, index) keys, and how many there are.  At most 16 when a block is tested, so 32 hold any block.
constexpr int kCandCapacity = 32;

__device__ __forceinline__ void t_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ float t_bcast(float v, int lane) {
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), lane));
}
__device__ __forceinline__ float t_wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ unsigned long long t_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int t_rank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
// value of lane `src` (any lane of the wave, may differ per lane) -- LDS crossbar, no LDS memory
__device__ __forceinline__ uint32_t t_lane_read(uint32_t v, int src) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v);
}
// sum over the 16 lanes of my team (row), result in every lane of the team
__device__ __forceinline__ uint32_t t_team_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x128 /*row_ror:8*/, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x124 /*row_ror:4*/, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x122 /*row_ror:2*/, 0xf, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x121 /*row_ror:1*/, 0xf, 0xf, false);
  return v;
}
// the same for a float (lane 0 of the team reads it; the order of the additions differs by lane)
__device__ __forceinline__ float t_team_sum(float v) {
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128 /*row_ror:8*/, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124 /*row_ror:4*/, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122 /*row_ror:2*/, 0xf, 0xf, false));
  v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121 /*row_ror:1*/, 0xf, 0xf, false));
  return v;
}
// min / max over the 16 lanes of my team, result in every lane of the team
__device__ __forceinline__ float t_team_min(float v) {
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128 /*row_ror:8*/, 0xf, 0xf, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124 /*row_ror:4*/, 0xf, 0xf, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122 /*row_ror:2*/, 0xf, 0xf, false)));
  v = fminf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121 /*row_ror:1*/, 0xf, 0xf, false)));
  return v;
}
__device__ __forceinline__ float t_team_max(float v) {
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128 /*row_ror:8*/, 0xf, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124 /*row_ror:4*/, 0xf, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x122 /*row_ror:2*/, 0xf, 0xf, false)));
  v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121 /*row_ror:1*/, 0xf, 0xf, false)));
  return v;
}
// value of another lane of my row through DPP (quad permutes, mirrors) -- no LDS, no address register
template <int CTRL>
__device__ __forceinline__ uint32_t t_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
// value of lane (mine ^ 4): lanes 0-3 and 8-11 of a row read four lanes up, the others four lanes down -- two
// DPP moves with complementary bank masks (a ds_swizzle does it in one instruction, but through the LDS
// crossbar: 24 cycles of the LDS pipe and its latency, scripts/microbench/issue_rate.hip)
__device__ __forceinline__ uint32_t t_xor4(uint32_t v) {
  const int up = __builtin_amdgcn_update_dpp(0, (int)v, 0x104 /*row_shl:4*/, 0xf, 0x5, false);
  return (uint32_t)__builtin_amdgcn_update_dpp(up, (int)v, 0x114 /*row_shr:4*/, 0xf, 0xa, false);
}

// my left neighbour's value inside the team (lane 0 of a team gets 0: bound_ctrl)
__device__ __forceinline__ uint32_t t_team_shr1(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111 /*row_shr:1*/, 0xf, 0xf, true);
}

// acc + (my bit of the wave mask) as ONE add-with-carry on the compare mask (the compiler's select + add is two)
__device__ __forceinline__ uint32_t t_count(uint32_t acc, unsigned long long mask) {
  uint32_t out;
  asm("v_addc_co_u32_e64 %0, vcc, 0, %1, %2" : "=v"(out) : "v"(acc), "s"(mask) : "vcc");
  return out;
}

// the same, and `keep` stays live (in its register) up to here at no cost: the COUNT pass never reads a
// block's id word, and the allocator would reuse the fourth register of a load's destination tuple as a
// temporary while the load is in flight -- a write-after-write hazard the compiler covers with
// s_waitcnt vmcnt(0), which drains the whole ring
__device__ __forceinline__ uint32_t t_count_keep(uint32_t acc, unsigned long long mask, int32_t keep) {
  uint32_t out;
  asm("v_addc_co_u32_e64 %0, vcc, 0, %1, %2" : "=v"(out) : "v"(acc), "s"(mask), "v"(keep) : "vcc");
  return out;
}

// squared distance from the three differences: knn_dist2's expression ((x*x) + (y*y)) + (z*z),
// x and y squared in one packed instruction
typedef float t_point4 __attribute__((ext_vector_type(4)));
// knn_dist2's expression ((x*x) + (y*y)) + (z*z), every operation rounded on its own.  Plain instructions: a
// packed v_pk_mul_f32 issues in 6.3 cycles against 2.4 for each of the two multiplies it replaces
// (scripts/microbench/issue_rate.hip); the file is compiled with -fno-slp-vectorize for the same reason.
__device__ __forceinline__ float t_dist2(float dx, float dy, float dz) {
#pragma clang fp contract(off)
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}

// one leaf block = LBVH_BLOCK sorted points, 16 bytes each; lane tl of a team reads point tl.
// The sorted arrays are padded with NaN sentinels to whole blocks and followed by one all-NaN block
// (lbvh.hip), so there is no bounds test and "no block" is an ordinary entry.
// Without a halo tree an entry is resolved to the block's BYTE offset when the entry registers are
// filled, and the load is "uniform base + 32-bit lane offset" (saddr form): one add per block
// instead of a mask, a 64-bit shift and a 64-bit add.  (Blocks < 2^24, i.e. n < 2^28: solve_team checks.)
template <bool HALO>
__device__ __forceinline__ LbvhPoint load_block_point(const LbvhPoint *own, const LbvhPoint *halo, int32_t entry,
                                                      const LbvhPoint *own_base, uint32_t lane_bytes) {
  if (!HALO) return *(const LbvhPoint *)((const char *)own_base + ((uint32_t)entry + lane_bytes));
  const LbvhPoint *base = entry < 0 ? halo : own;
  return base[(int64_t)(entry & 0x7fffffff) * LBVH_BLOCK];
}
template <bool HALO>
__device__ __forceinline__ int32_t resolve_entry(int32_t e) {
  return HALO ? e : (int32_t)((uint32_t)e * (uint32_t)(LBVH_BLOCK * sizeof(LbvhPoint)));
}

// ---- a team's sorted list and its candidate buffer ---------------------------------------------------------------------
// One compare-exchange with the lane whose key is (pd, pi): the lower lane keeps the smaller key.
__device__ __forceinline__ void t_exchange(uint32_t &kd, uint32_t &ki, uint32_t pd, uint32_t pi, bool upper) {
  const uint64_t mine_k = ((uint64_t)kd << 32) | ki, other = ((uint64_t)pd << 32) | pi;
  const bool take = (other < mine_k) != upper;  // lower lane: the smaller key; upper lane: the larger (equal: either)
  kd = take ? pd : kd;
  ki = take ? pi : ki;
}
// 16 keys of a team, one per lane, into ascending order: a bitonic network written so that every exchange
// keeps the smaller key in the lower lane -- mirror within 2, 4, 8, 16 lanes followed by xor 4 / 2 / 1
// steps; ten exchanges of DPP moves (quad permutes, mirrors, row shifts) and a 64-bit compare each.
__device__ __forceinline__ void t_sort16(uint32_t &kd, uint32_t &ki, int tl) {
  const bool up1 = (tl & 1) != 0, up2 = (tl & 2) != 0, up4 = (tl & 4) != 0, up8 = (tl & 8) != 0;
  t_exchange(kd, ki, t_dpp<0xb1>(kd), t_dpp<0xb1>(ki), up1);    // pairs
  t_exchange(kd, ki, t_dpp<0x1b>(kd), t_dpp<0x1b>(ki), up2);    // mirror within 4
  t_exchange(kd, ki, t_dpp<0xb1>(kd), t_dpp<0xb1>(ki), up1);
  t_exchange(kd, ki, t_dpp<0x141>(kd), t_dpp<0x141>(ki), up4);  // mirror within 8 (row_half_mirror)
  t_exchange(kd, ki, t_dpp<0x4e>(kd), t_dpp<0x4e>(ki), up2);    // xor 2
  t_exchange(kd, ki, t_dpp<0xb1>(kd), t_dpp<0xb1>(ki), up1);
  t_exchange(kd, ki, t_dpp<0x140>(kd), t_dpp<0x140>(ki), up8);  // mirror within 16 (row_mirror)
  t_exchange(kd, ki, t_xor4(kd), t_xor4(ki), up4);
  t_exchange(kd, ki, t_dpp<0x4e>(kd), t_dpp<0x4e>(ki), up2);
  t_exchange(kd, ki, t_dpp<0xb1>(kd), t_dpp<0xb1>(ki), up1);
}
// four half-cleaners: a bitonic sequence of sixteen keys, one per lane of the team, into ascending order
__device__ __forceinline__ void t_clean16(uint32_t &kd, uint32_t &ki, int tl) {
  const bool up1 = (tl & 1) != 0, up2 = (tl & 2) != 0, up4 = (tl & 4) != 0, up8 = (tl & 8) != 0;
  t_exchange(kd, ki, t_dpp<0x128>(kd), t_dpp<0x128>(ki), up8);  // xor 8 (row_ror:8)
  t_exchange(kd, ki, t_xor4(kd), t_xor4(ki), up4);
  t_exchange(kd, ki, t_dpp<0x4e>(kd), t_dpp<0x4e>(ki), up2);
  t_exchange(kd, ki, t_dpp<0xb1>(kd), t_dpp<0xb1>(ki), up1);
}
// ---- the same network on ONE 32-bit word per lane (round 4) ------------------------------------------------------------
// A 64-bit exchange is two DPP moves, a 64-bit compare, a mask xor and two selects -- six slow instructions and their wait
// states, ten times per sort: the sorting networks were a fifth of the packet kernel's vector time.  On one word the
// exchange is a DPP move and ONE v_med3_u32: med3(a, b, 0) = min(a, b) for the lower lane of a pair, med3(a, b, ~0) =
// max(a, b) for the upper one (the third operand is a constant of the lane).  The word is the key's order WITHOUT its last
// four bits, which carry the lane the key came from; the caller fetches the exact key from there afterwards and checks that
// the dropped bits could not have mattered (t_sorted_row).
__device__ __forceinline__ uint32_t t_med3_u32(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t out;
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(out) : "v"(a), "v"(b), "v"(c));
  return out;
}
// partner lane ^ 4, lower lane keeps the smaller word: the two halves as one masked min and one masked max (bank = four
// consecutive lanes of a row; row_shl:4 reads four lanes up, row_shr:4 four lanes down).  s_nop: a DPP operand written by the
// instruction before it needs two wait states, and the compiler does not look into inline assembly for that.
__device__ __forceinline__ uint32_t t_exchange_xor4_u32(uint32_t v) {
  uint32_t out;
  asm("s_nop 1\n\t"
      "v_min_u32_dpp %0, %1, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
      "v_max_u32_dpp %0, %1, %1 row_shr:4 row_mask:0xf bank_mask:0xa"
      : "=&v"(out)
      : "v"(v));
  return out;
}
__device__ __forceinline__ void t_sort16_u32(uint32_t &v, int tl) {
  const uint32_t c1 = 0u - ((uint32_t)tl & 1u), c2 = 0u - (((uint32_t)tl >> 1) & 1u), c4 = 0u - (((uint32_t)tl >> 2) & 1u),
                 c8 = 0u - (((uint32_t)tl >> 3) & 1u);
  v = t_med3_u32(v, t_dpp<0xb1>(v), c1);   // pairs
  v = t_med3_u32(v, t_dpp<0x1b>(v), c2);   // mirror within 4
  v = t_med3_u32(v, t_dpp<0xb1>(v), c1);
  v = t_med3_u32(v, t_dpp<0x141>(v), c4);  // mirror within 8
  v = t_med3_u32(v, t_dpp<0x4e>(v), c2);   // xor 2
  v = t_med3_u32(v, t_dpp<0xb1>(v), c1);
  v = t_med3_u32(v, t_dpp<0x140>(v), c8);  // mirror within 16
  v = t_exchange_xor4_u32(v);
  v = t_med3_u32(v, t_dpp<0x4e>(v), c2);
  v = t_med3_u32(v, t_dpp<0xb1>(v), c1);
}
// Sixteen (squared distance, index) keys, one per lane of a team (`have`: my lane has one), as the sorted row of
// (IEEE distance, index) keys the lists take -- KNN_EMPTY_KEY past the last.  `fetch(lane)` returns the key lane `lane` of
// my team came with.  The sort runs on (bits of d2 without their last four | lane); it is the order of the full keys unless
// two neighbours of the outcome are closer than that can tell -- their truncated words equal or one apart, which covers
// d2 values less than sixteen ulps apart: exact duplicates, the ties of quantised data, and the pairs of different squares
// whose ROUNDED roots coincide (the pre-image of one rounded root spans three floats), for which the index decides -- or a
// square overflowed to infinity (its root is beyond the empty key, which the word order does not know).  Then the exact
// network runs instead (uniform 10 M points: once in 10^4 rows).
template <typename Fetch>
__device__ __forceinline__ void t_sorted_row(uint32_t d2_bits, uint32_t id, bool have, int tl, Fetch fetch, uint32_t &kd, uint32_t &ki) {
  uint32_t w = have ? ((d2_bits & ~15u) | (uint32_t)tl) : (0xfffffff0u | (uint32_t)tl);
  t_sort16_u32(w, tl);
  const uint32_t before = t_team_shr1(w);
  const bool real = w < 0xfffffff0u;
  const bool unsure = real & (((tl > 0) & ((w >> 4) - (before >> 4) <= 1u)) | (w >= 0x7f7ffff0u));
  if (__builtin_expect(__ballot(unsure) == 0ull, 1)) {
    const unsigned long long key = fetch((int)(w & 15u));
    const float dist = knn_sqrt(__uint_as_float((uint32_t)(key >> 32)));
    kd = real ? __float_as_uint(dist) : 0x7f7fffffu;
    ki = real ? (uint32_t)key : 0u;
  } else {
    const float dist = knn_sqrt(__uint_as_float(d2_bits));
    kd = have ? __float_as_uint(dist) : 0x7f7fffffu;
    ki = have ? id : 0u;
    t_sort16(kd, ki, tl);
  }
}

// Candidates that pass a team's gate are not inserted one lock-step round each: they wait in the team's LDS buffer as
// (squared distance, index) and are MERGED into the sorted list sixteen at a time.  `buf`: my team's buffer, `fill`: how
// many wait (the same in the team's lanes).  Per row of sixteen: the IEEE root (sixteen instructions, once per row and not
// per block step), the sorting network, then the row meets the list one register (sixteen sorted entries, all of them
// below the next register's) at a time: mirrored, lane j against the row's key 15 - j, the sixteen smallest of both stay
// in the register and the sixteen largest travel on as the row for the next register -- both come out as bitonic
// sequences, four half-cleaners each.  A register no key of the row gets into is left as it is.  What comes out of the
// last register has fallen out of the list (`left_out`, tracked if `full`: its smallest distance, team minimum taken by
// the caller).  Some 80 vector instructions per row for k <= 16, 250 for k <= 64, whatever the number of candidates.
template <int NREG>
__device__ __forceinline__ void t_merge_rows(uint32_t (&bd)[NREG], uint32_t (&bi)[NREG], uint32_t &left_out, bool full,
                                             const unsigned long long *buf, uint32_t fill, int tl) {
#pragma unroll
  for (int row = 0; row < kCandCapacity / 16; row++) {
    if (row > 0 && __ballot(fill > 16u * (uint32_t)row) == 0ull) break;
    const uint32_t at = 16u * (uint32_t)row + (uint32_t)tl;
    const bool have = at < fill;
    const unsigned long long key = have ? buf[at] : 0ull;
    uint32_t kd, ki;  // the row, sorted: (IEEE distance, index), KNN_EMPTY_KEY past the end
    t_sorted_row((uint32_t)(key >> 32), (uint32_t)key, have, tl, [&](int from) { return buf[16 * row + from]; }, kd, ki);
#pragma unroll
    for (int j = 0; j < NREG; j++) {
      const uint32_t od = t_dpp<0x140>(kd), oi = t_dpp<0x140>(ki);  // the row's key 15 - tl
      const uint64_t mine_k = ((uint64_t)bd[j] << 32) | bi[j], other = ((uint64_t)od << 32) | oi;
      const bool take = other < mine_k;
      if (NREG > 1 && __ballot(take) == 0ull) {  // every key of the row is larger than this whole register: on to the next
        if (full && j == NREG - 1) left_out = min(left_out, kd);
        continue;
      }
      const uint32_t hd = take ? bd[j] : od, hi_i = take ? bi[j] : oi;  // the larger of the pair: travels on (or falls out)
      bd[j] = take ? od : bd[j];
      bi[j] = take ? oi : bi[j];
      t_clean16(bd[j], bi[j], tl);
      if (j == NREG - 1) {
        if (full) left_out = min(left_out, hd);
      } else {
        kd = hd, ki = hi_i;
        t_clean16(kd, ki, tl);
      }
    }
  }
}

// Can two candidates of one query at the same fp32 distance d have become candidates in DIFFERENT
// rounds?  A candidate's Chebyshev distance t obeys d / sqrt(3) <= t <= d (sqrt(2) for points in a
// plane z = const, as the reference's 2-D inputs are: `span`), and round l takes it iff
// t <= r_l (up to the rounding margin M of the box test, see team_kernel).  Going up the radii: if
// d is safely below r_l, every candidate at distance d passes round l -- and none passed an earlier
// round, or the loop would have stopped there; if not, but d / sqrt(3) can be below r_l, some may
// pass and others not.  Exact duplicates (d = 0) and the other ties of quantised data mostly are of
// the first kind and need no second look.  qmax = max |q|, r_last = the radius the query finished with.
__device__ __forceinline__ bool tie_may_straddle(float d, float r0, float r_last, float qmax, float span) {
  for (float r = r0;; r = r * 2.0f) {
    const float mg = (qmax + 2.0f * r) * 4.76837158203125e-07f;  // 2^-21
    if (d <= (r - mg) * 0.99999f) return false;
    if (d <= (r + mg) * span) return true;  // t >= d / span > r + M otherwise: certainly not a candidate of round l
    if (!(r < r_last)) return true;  // (a listed candidate passes the last round's test: not reached)
  }
}

}  // namespace

}  // namespace owlmi
