// feature_match.hip -- nearest and second-nearest target row of every source row in D <= 64 dimensions (tknnFeatureMatch,
// include/owlknn_global.h): dense brute force, every pair and channel in literal fp32 (t = a - b; acc = acc + t*t), no tree.
//
//   1. match_flag_kernel, once per side: a byte per row, 1 where an entry is not finite, and their count;
//   2. match_kernel<DP, R>: a workgroup of 256 lanes holds 256 * R source rows, R per lane in registers at the compile-time width
//      DP (D padded up to a multiple of 4 with zeros: a padded channel adds +0.0 to a sum that is never -0.0), and streams one
//      chunk of the target through LDS in tiles of kTile rows.  Every lane reads the same address of the tile, so a ds_read_b128
//      broadcasts 4 channels that feed 4 * R pair-channels, 12 * R VALU operations.  R = 2 (measured).  grid.y is the chunk: small m still fills
//      the chip.  Each (chunk, source row) writes a partial: best d2, best row, second d2;
//   3. match_merge_kernel: one lane per source row folds the partials in chunk order.  The rule -- smaller d2, then smaller row;
//      the second is the smallest of what did not win -- is associative, so the result does not depend on the chunks.
// No float atomic and no packed 64-bit minimum: the second-best could ride on neither.
// The call's workspace (Engine::workspace): counters | flags of the source rows | flags of the target rows | partials, three
// columns of chunks * m words.
#include "owlknn_global.h"
#include "trueknn_engine.h"

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kMatchBlock = 256;
constexpr int kMatchTile = 64;          // target rows per LDS tile: at DP = 64 the tile is 16 KiB
constexpr int kMatchBlocksPerCu = 4;    // the grid the chunks are cut for
constexpr int32_t kNoRow = 0x7fffffff;  // "no row yet": above every row, so that an acc of +inf still takes the smaller row
enum { kMatchBadSource = 0, kMatchBadTarget = 1, kMatchWords = 2 };

size_t match_align(size_t b) { return (b + 255) & ~(size_t)255; }

__global__ void __launch_bounds__(kMatchBlock) match_flag_kernel(const float *__restrict__ rows, int32_t count, int D, uint8_t *__restrict__ bad,
                                                               unsigned long long *__restrict__ counter) {
  const int64_t i = (int64_t)blockIdx.x * kMatchBlock + threadIdx.x;  // (64 bits: count may be within a block of 2^31)
  if (i >= count) return;
  bool b = false;
  for (int c = 0; c < D; c++) b |= !(fabsf(rows[i * D + c]) <= FLT_MAX);
  bad[i] = b ? 1 : 0;
  if (b) atomicAdd(counter, 1ull);
}

// (d2, row) takes the place of the best when it is smaller, the row deciding a tie; what loses is a candidate for the second
__device__ __forceinline__ void match_take(float d2, int32_t row, float &b1, int32_t &r1, float &b2) {
  if (d2 < b1 || (d2 == b1 && row < r1)) {
    b2 = b1;
    b1 = d2;
    r1 = row;
  } else {
    b2 = fminf(b2, d2);
  }
}

struct MatchArgs {
  const float *source, *target;
  const uint8_t *bad_target;
  int32_t m, n, D;
  int32_t chunk;  // target rows per chunk
  float *part_d2, *part_second;
  int32_t *part_row;  // [chunk][m]
};

template <int DP, int R>
__global__ void __launch_bounds__(kMatchBlock) match_kernel(MatchArgs a) {
#pragma clang fp contract(off)
  __shared__ float4 tile[kMatchTile][DP / 4];
  __shared__ int tile_ok[kMatchTile];
  float src[R][DP];
  float b1[R], b2[R];
  int32_t r1[R];
  const int64_t row0 = (int64_t)blockIdx.x * (kMatchBlock * R) + threadIdx.x;  // (64 bits: the last block's rows may pass 2^31)
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int64_t row = row0 + r * kMatchBlock;
#pragma unroll
    for (int c = 0; c < DP; c++) src[r][c] = (c < a.D && row < a.m) ? a.source[row * a.D + c] : 0.f;
    b1[r] = b2[r] = __builtin_inff();
    r1[r] = kNoRow;
  }
  const int64_t lo64 = (int64_t)blockIdx.y * a.chunk, hi64 = lo64 + a.chunk;
  const int32_t lo = (int32_t)(lo64 < a.n ? lo64 : a.n), hi = (int32_t)(hi64 < a.n ? hi64 : a.n);
  for (int32_t base = lo; base < hi; base += kMatchTile) {
    const int rows = min(kMatchTile, hi - base);
    __syncthreads();  // the tile before is read
    for (int i = threadIdx.x; i < kMatchTile * DP; i += kMatchBlock) {
      const int j = i / DP, c = i % DP;
      ((float *)&tile[j][0])[c] = (j < rows && c < a.D) ? a.target[(int64_t)(base + j) * a.D + c] : 0.f;
    }
    if (threadIdx.x < kMatchTile) tile_ok[threadIdx.x] = (int)threadIdx.x < rows && !a.bad_target[base + threadIdx.x];
    __syncthreads();
    for (int j = 0; j < rows; j++) {
      if (!tile_ok[j]) continue;  // (uniform)
      float acc[R];
#pragma unroll
      for (int r = 0; r < R; r++) acc[r] = 0.f;
#pragma unroll
      for (int c4 = 0; c4 < DP / 4; c4++) {
        const float4 b = tile[j][c4];
#pragma unroll
        for (int r = 0; r < R; r++) {
          float t = src[r][4 * c4] - b.x;
          acc[r] = acc[r] + t * t;
          t = src[r][4 * c4 + 1] - b.y;
          acc[r] = acc[r] + t * t;
          t = src[r][4 * c4 + 2] - b.z;
          acc[r] = acc[r] + t * t;
          t = src[r][4 * c4 + 3] - b.w;
          acc[r] = acc[r] + t * t;
        }
      }
#pragma unroll
      for (int r = 0; r < R; r++) match_take(acc[r], base + j, b1[r], r1[r], b2[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int64_t row = row0 + r * kMatchBlock;
    if (row >= a.m) continue;
    const int64_t at = (int64_t)blockIdx.y * a.m + row;
    a.part_d2[at] = b1[r];
    a.part_row[at] = r1[r];
    a.part_second[at] = b2[r];
  }
}

__global__ void __launch_bounds__(kMatchBlock) match_merge_kernel(const float *__restrict__ part_d2, const int32_t *__restrict__ part_row,
                                                                const float *__restrict__ part_second, int32_t chunks, int32_t m,
                                                                const uint8_t *__restrict__ bad_source, int32_t *__restrict__ best,
                                                                float *__restrict__ best_d2, float *__restrict__ second_d2) {
  const int64_t i = (int64_t)blockIdx.x * kMatchBlock + threadIdx.x;
  if (i >= m) return;
  float b1 = __builtin_inff(), b2 = __builtin_inff();
  int32_t r1 = kNoRow;
  if (!bad_source[i])
    for (int32_t c = 0; c < chunks; c++) {
      const int64_t at = (int64_t)c * m + i;
      match_take(part_d2[at], part_row[at], b1, r1, b2);
      b2 = fminf(b2, part_second[at]);
    }
  if (r1 == kNoRow) b1 = b2 = __builtin_inff();
  if (best) best[i] = r1 == kNoRow ? -1 : r1;
  if (best_d2) best_d2[i] = b1;
  if (second_d2) second_d2[i] = b2;
}

// R rows per lane: 2; 4 is instantiated up to the width an FPFH has for the measurement (the source rows alone are R * DP registers)
template <int DP>
void match_launch(const MatchArgs &a, int rows_per_lane, int32_t chunks, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)a.m + kMatchBlock * rows_per_lane - 1) / (kMatchBlock * rows_per_lane)), (unsigned)chunks);
  if constexpr (DP <= 36) {
    if (rows_per_lane == 4) {
      hipLaunchKernelGGL((match_kernel<DP, 4>), grid, dim3(kMatchBlock), 0, s, a);
      return;
    }
  }
  hipLaunchKernelGGL((match_kernel<DP, 2>), grid, dim3(kMatchBlock), 0, s, a);
}

template <int... DP>
void match_dispatch(int dp, const MatchArgs &a, int rows_per_lane, int32_t chunks, hipStream_t s, std::integer_sequence<int, DP...>) {
  (void)((dp == 4 * (DP + 1) ? (match_launch<4 * (DP + 1)>(a, rows_per_lane, chunks, s), true) : false) || ...);
}

int env_int(const char *name, int otherwise) {
  const char *e = getenv(name);
  return e && atoi(e) > 0 ? atoi(e) : otherwise;
}

}  // namespace

void Engine::feature_match(const tknnFeatureMatchOptions &o, tknnFeatureMatchInfo *info, hipStream_t s) {
  const int32_t m = (int32_t)o.m, n = (int32_t)o.n;
  const int dp = (o.D + 3) & ~3;
  // R = 2: measured at D = 33, four rows per lane are 11 - 38 % slower there; TKNN_MATCH_ROWS=4 repeats the
  // measurement up to DP = 36.  Widths above 36 run R = 2 unmeasured.  Neither it nor the chunk changes a result.
  const int rows_per_lane = env_int("TKNN_MATCH_ROWS", 2) == 4 && dp <= 36 ? 4 : 2;
  const int64_t source_blocks = ((int64_t)m + kMatchBlock * rows_per_lane - 1) / (kMatchBlock * rows_per_lane);
  // the chunks: enough of them that source blocks x chunks is kMatchBlocksPerCu workgroups per compute unit, whole tiles each
  int64_t chunk = env_int("TKNN_MATCH_CHUNK", 0);
  if (chunk == 0) {
    const int64_t want = std::max<int64_t>(1, ((int64_t)cu_count_ * kMatchBlocksPerCu + source_blocks - 1) / source_blocks);
    chunk = ((int64_t)n + want - 1) / want;
    chunk = std::max<int64_t>(kMatchTile, (chunk + kMatchTile - 1) / kMatchTile * kMatchTile);
  }
  chunk = std::max(chunk, ((int64_t)n + 65534) / 65535);  // (grid.y)
  const int32_t chunks = (int32_t)(((int64_t)n + chunk - 1) / chunk);  // (n = 0: none)
  const size_t col_counters = match_align(kMatchWords * sizeof(unsigned long long)), col_bad_s = match_align((size_t)m), col_bad_t = match_align((size_t)std::max(n, 1)),
               col_part = match_align((size_t)std::max(chunks, 1) * m * sizeof(float));
  char *ws = (char *)workspace(col_counters + col_bad_s + col_bad_t + 3 * col_part);
  unsigned long long *counters = (unsigned long long *)ws;
  uint8_t *bad_s = (uint8_t *)(ws + col_counters), *bad_t = bad_s + col_bad_s;
  MatchArgs a;
  std::memset(&a, 0, sizeof a);
  a.source = o.d_source, a.target = o.d_target, a.bad_target = bad_t;
  a.m = m, a.n = n, a.D = o.D, a.chunk = (int32_t)std::min<int64_t>(chunk, 0x7fffffff);
  a.part_d2 = (float *)(bad_t + col_bad_t);
  a.part_second = (float *)((char *)a.part_d2 + col_part);
  a.part_row = (int32_t *)((char *)a.part_d2 + 2 * col_part);

  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(counters, 0, kMatchWords * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(match_flag_kernel, dim3((unsigned)(((int64_t)m + kMatchBlock - 1) / kMatchBlock)), dim3(kMatchBlock), 0, s, o.d_source, m, (int)o.D, bad_s, counters + kMatchBadSource);
  OWLMI_HIP(hipGetLastError());
  if (n > 0) {
    hipLaunchKernelGGL(match_flag_kernel, dim3((unsigned)(((int64_t)n + kMatchBlock - 1) / kMatchBlock)), dim3(kMatchBlock), 0, s, o.d_target, n, (int)o.D, bad_t, counters + kMatchBadTarget);
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  if (chunks > 0) {
    match_dispatch(dp, a, rows_per_lane, chunks, s, std::make_integer_sequence<int, TKNN_MATCH_MAX_D / 4>{});
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  hipLaunchKernelGGL(match_merge_kernel, dim3((unsigned)(((int64_t)m + kMatchBlock - 1) / kMatchBlock)), dim3(kMatchBlock), 0, s, (const float *)a.part_d2, (const int32_t *)a.part_row,
                     (const float *)a.part_second, chunks, m, (const uint8_t *)bad_s, o.d_best, o.d_best_d2, o.d_second_d2);
  OWLMI_HIP(hipGetLastError());
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipMemcpyAsync(h_counters_, counters, kMatchWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  info->bad_source_rows = (int64_t)h_counters_[kMatchBadSource];
  info->bad_target_rows = (int64_t)h_counters_[kMatchBadTarget];
  info->pair_tests = ((int64_t)m - info->bad_source_rows) * ((int64_t)n - info->bad_target_rows);
  info->chunks = chunks;
  OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_d_));
  OWLMI_HIP(hipEventElapsedTime(&info->match_ms, ev_b_, ev_c_));
  OWLMI_HIP(hipEventElapsedTime(&info->merge_ms, ev_c_, ev_d_));
}

}  // namespace owlmi
