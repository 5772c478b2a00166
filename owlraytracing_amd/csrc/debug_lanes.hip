// debug_lanes.hip -- the lane harness behind tknnDebugTeamLanes (include/owlknn_debug.h): ONE helper of team_lanes.h,
// team_walk.h or bigk_keys.h on lanes the caller filled, called as the kernels call it -- no helper is written a second time in
// here.  One wave per workgroup, four teams per wave; the lanes of a wave's missing teams run the helper too (the helpers hold
// wave-wide ballots and barriers) on zero words and store nothing.  Built like the team files (-fno-slp-vectorize).
#include "bigk_keys.h"
#include "owlknn_debug.h"
#include "team_lanes.h"
#include "team_walk.h"
#include "trueknn_engine.h"

namespace owlmi {

namespace {

// words per lane in and out (the table of include/owlknn_debug.h)
__host__ __device__ constexpr int lanes_win(int op, int nreg) {
  return op == TKNN_LANES_SORT16 || op == TKNN_LANES_CLEAN16  ? 2
         : op == TKNN_LANES_SORT16_U32                        ? 1
         : op == TKNN_LANES_SORTED_ROW                        ? 3
         : op == TKNN_LANES_MERGE                             ? 2 * nreg + 7
         : op == TKNN_LANES_KTH                               ? nreg + 1
         : op == TKNN_LANES_ROW_TIES                          ? nreg + 10
         : op == TKNN_LANES_STRADDLE                          ? 5
         : op == TKNN_LANES_FIRST_LEVEL                       ? 8
         : op == TKNN_LANES_REDUCE                            ? 1
         : op == TKNN_LANES_MOVES                             ? 4
                                                              : 3;  // SORT16_3, CLEAN16_3
}
__host__ __device__ constexpr int lanes_wout(int op, int nreg) {
  return op == TKNN_LANES_SORT16 || op == TKNN_LANES_CLEAN16 || op == TKNN_LANES_SORTED_ROW ? 2
         : op == TKNN_LANES_SORT16_U32                                                      ? 1
         : op == TKNN_LANES_MERGE                                                           ? 2 * nreg + 1
         : op == TKNN_LANES_KTH || op == TKNN_LANES_STRADDLE || op == TKNN_LANES_FIRST_LEVEL ? 1
         : op == TKNN_LANES_ROW_TIES                                                        ? 2
         : op == TKNN_LANES_REDUCE                                                          ? 8
         : op == TKNN_LANES_MOVES                                                           ? 15
                                                                                            : 3;
}

template <int OP, int NREG>
__global__ void __launch_bounds__(64) lanes_kernel(const uint32_t *in, uint32_t *out, int64_t teams, int variant) {
  constexpr int WIN = lanes_win(OP, NREG), WOUT = lanes_wout(OP, NREG);
  __shared__ unsigned long long cand_mem[4 * kCandCapacity];  // per team: t_sorted_row's fetch, t_merge_rows's buf
  const int lane = threadIdx.x & 63, team = lane >> 4, tl = lane & 15;
  const int64_t t = (int64_t)blockIdx.x * 4 + team;
  const bool present = t < teams;
  uint32_t x[WIN], y[WOUT];
#pragma unroll
  for (int w = 0; w < WIN; w++) x[w] = present ? in[(t * WIN + w) * 16 + tl] : 0u;
#pragma unroll
  for (int w = 0; w < WOUT; w++) y[w] = 0u;
  unsigned long long *my_buf = cand_mem + team * kCandCapacity;

  if constexpr (OP == TKNN_LANES_SORT16) {
    t_sort16(x[0], x[1], tl);
    y[0] = x[0], y[1] = x[1];
  } else if constexpr (OP == TKNN_LANES_CLEAN16) {
    t_clean16(x[0], x[1], tl);
    y[0] = x[0], y[1] = x[1];
  } else if constexpr (OP == TKNN_LANES_SORT16_U32) {
    t_sort16_u32(x[0], tl);
    y[0] = x[0];
  } else if constexpr (OP == TKNN_LANES_SORTED_ROW) {
    my_buf[tl] = ((unsigned long long)x[0] << 32) | x[1];
    t_wave_sync();
    t_sorted_row(x[0], x[1], x[2] != 0u, tl, [&](int from) { return my_buf[from]; }, y[0], y[1]);
  } else if constexpr (OP == TKNN_LANES_MERGE) {
    uint32_t bd[NREG], bi[NREG];
#pragma unroll
    for (int j = 0; j < NREG; j++) {
      bd[j] = present ? x[j] : 0x7f7fffffu;  // a missing team: the empty list
      bi[j] = x[NREG + j];
    }
    my_buf[tl] = ((unsigned long long)x[2 * NREG] << 32) | x[2 * NREG + 1];
    my_buf[16 + tl] = ((unsigned long long)x[2 * NREG + 2] << 32) | x[2 * NREG + 3];
    const uint32_t fill = x[2 * NREG + 4];
    uint32_t left_out = present ? x[2 * NREG + 5] : 0xffffffffu;
    const bool full = x[2 * NREG + 6] != 0u;
    t_wave_sync();
    t_merge_rows<NREG>(bd, bi, left_out, full, my_buf, fill, tl);
    left_out = t_team_min_u32(left_out);
#pragma unroll
    for (int j = 0; j < NREG; j++) y[j] = bd[j], y[NREG + j] = bi[j];
    y[2 * NREG] = left_out;
  } else if constexpr (OP == TKNN_LANES_KTH) {
    uint32_t bd[NREG];
#pragma unroll
    for (int j = 0; j < NREG; j++) bd[j] = x[j];
    const int k = present ? (int)x[NREG] : 1;
    y[0] = __float_as_uint(t_kth_dist<NREG>(bd, k, team));
  } else if constexpr (OP == TKNN_LANES_ROW_TIES) {
    uint32_t bd[NREG];
#pragma unroll
    for (int j = 0; j < NREG; j++) bd[j] = x[j];
    const LbvhPoint q{__uint_as_float(x[NREG + 3]), __uint_as_float(x[NREG + 4]), __uint_as_float(x[NREG + 5]), 0};
    const float r0 = __uint_as_float(x[NREG + 6]);
    const bool bounded = r0 > 0.f;  // tie_may_straddle doubles r0 until it passes d
    bool tie, edge;
    t_row_ties<NREG>(bd, x[NREG], x[NREG + 1] != 0u, present ? (int)x[NREG + 2] : 1, tl, q, bounded ? r0 : 1.f, __uint_as_float(x[NREG + 7]),
                     __uint_as_float(x[NREG + 8]), x[NREG + 9] != 0u, tie, edge);
    y[0] = bounded ? (tie ? 1u : 0u) : 0xffffffffu;
    y[1] = bounded ? (edge ? 1u : 0u) : 0xffffffffu;
  } else if constexpr (OP == TKNN_LANES_STRADDLE) {
    const float r0 = __uint_as_float(x[1]);
    const bool bounded = r0 > 0.f;
    const bool s = tie_may_straddle(__uint_as_float(x[0]), bounded ? r0 : 1.f, __uint_as_float(x[2]), __uint_as_float(x[3]), __uint_as_float(x[4]));
    y[0] = bounded ? (s ? 1u : 0u) : 0xffffffffu;
  } else if constexpr (OP == TKNN_LANES_FIRST_LEVEL) {
    const LbvhPoint p{__uint_as_float(x[0]), __uint_as_float(x[1]), __uint_as_float(x[2]), 0};
    const LbvhPoint q{__uint_as_float(x[3]), __uint_as_float(x[4]), __uint_as_float(x[5]), 0};
    y[0] = first_level(p, q, __uint_as_float(x[6]), min(max((int)x[7], 0), 64));
  } else if constexpr (OP == TKNN_LANES_REDUCE) {
    const float f = __uint_as_float(x[0]);
    y[0] = t_team_sum(x[0]);
    y[1] = __float_as_uint(t_team_sum(f));
    y[2] = __float_as_uint(t_team_min(f));
    y[3] = __float_as_uint(t_team_max(f));
    y[4] = t_team_min_u32(x[0]);
    y[5] = __float_as_uint(t_wave_max(f));
    const unsigned long long ws = t_wave_sum((unsigned long long)x[0]);
    y[6] = (uint32_t)ws, y[7] = (uint32_t)(ws >> 32);
  } else if constexpr (OP == TKNN_LANES_MOVES) {
    const uint32_t v = x[0];
    const bool bit = x[2] != 0u;
    const unsigned long long m = __ballot(bit);
    y[0] = t_xor4(v);
    y[1] = t_team_shr1(v);
    y[2] = t_dpp<0xb1>(v);
    y[3] = t_dpp<0x1b>(v);
    y[4] = t_dpp<0x4e>(v);
    y[5] = t_dpp<0x141>(v);
    y[6] = t_dpp<0x140>(v);
    y[7] = t_dpp<0x128>(v);
    y[8] = t_dpp<0x121>(v);
    y[9] = t_lane_read(v, (team << 4) + (int)(x[1] & 15u));
    y[10] = (uint32_t)t_rank(m);
    y[11] = t_count(x[3], m);
    y[12] = t_count_keep(x[3], m, (int32_t)v);
    y[13] = t_team_any(bit, team) ? 1u : 0u;
    y[14] = __float_as_uint(t_bcast(__uint_as_float(v), variant));
  } else if constexpr (OP == TKNN_LANES_SORT16_3) {
    t_sort16_3(x[0], x[1], x[2], tl);
    y[0] = x[0], y[1] = x[1], y[2] = x[2];
  } else {
    static_assert(OP == TKNN_LANES_CLEAN16_3, "an op without a body");
    t_clean16_3(x[0], x[1], x[2], tl);
    y[0] = x[0], y[1] = x[1], y[2] = x[2];
  }

  if (present) {
#pragma unroll
    for (int w = 0; w < WOUT; w++) out[(t * WOUT + w) * 16 + tl] = y[w];
  }
}

bool lanes_has_nreg(int op) { return op == TKNN_LANES_MERGE || op == TKNN_LANES_KTH || op == TKNN_LANES_ROW_TIES; }

template <int OP, int NREG>
void lanes_launch(const uint32_t *d_in, uint32_t *d_out, int64_t teams, int variant, hipStream_t s) {
  hipLaunchKernelGGL((lanes_kernel<OP, NREG>), dim3((unsigned)((teams + 3) / 4)), dim3(64), 0, s, d_in, d_out, teams, variant);
}
template <int OP>
void lanes_launch_nreg(const uint32_t *d_in, uint32_t *d_out, int64_t teams, int variant, hipStream_t s) {
  switch (variant) {
    case 1: return lanes_launch<OP, 1>(d_in, d_out, teams, variant, s);
    case 2: return lanes_launch<OP, 2>(d_in, d_out, teams, variant, s);
    case 3: return lanes_launch<OP, 3>(d_in, d_out, teams, variant, s);
    default: return lanes_launch<OP, 4>(d_in, d_out, teams, variant, s);
  }
}

}  // namespace

bool debug_team_lanes_words(int op, int variant, int *win, int *wout) {
  if (op < 0 || op >= TKNN_LANES_OPS) return false;
  const bool ok = lanes_has_nreg(op) ? (variant >= 1 && variant <= 4) : op == TKNN_LANES_MOVES ? (variant >= 0 && variant <= 63) : variant == 0;
  if (!ok) return false;
  if (win) *win = lanes_win(op, variant);
  if (wout) *wout = lanes_wout(op, variant);
  return true;
}

void debug_team_lanes(int op, int variant, const uint32_t *d_in, uint32_t *d_out, int64_t teams, hipStream_t s) {
  if (teams <= 0) return;
  switch (op) {
    case TKNN_LANES_SORT16: lanes_launch<TKNN_LANES_SORT16, 1>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_CLEAN16: lanes_launch<TKNN_LANES_CLEAN16, 1>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_SORT16_U32: lanes_launch<TKNN_LANES_SORT16_U32, 1>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_SORTED_ROW: lanes_launch<TKNN_LANES_SORTED_ROW, 1>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_MERGE: lanes_launch_nreg<TKNN_LANES_MERGE>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_KTH: lanes_launch_nreg<TKNN_LANES_KTH>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_ROW_TIES: lanes_launch_nreg<TKNN_LANES_ROW_TIES>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_STRADDLE: lanes_launch<TKNN_LANES_STRADDLE, 1>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_FIRST_LEVEL: lanes_launch<TKNN_LANES_FIRST_LEVEL, 1>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_REDUCE: lanes_launch<TKNN_LANES_REDUCE, 1>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_MOVES: lanes_launch<TKNN_LANES_MOVES, 1>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_SORT16_3: lanes_launch<TKNN_LANES_SORT16_3, 1>(d_in, d_out, teams, variant, s); break;
    case TKNN_LANES_CLEAN16_3: lanes_launch<TKNN_LANES_CLEAN16_3, 1>(d_in, d_out, teams, variant, s); break;
    default: throw ArgError{TKNN_E_ARG, "tknnDebugTeamLanes: no such op"};
  }
  OWLMI_HIP(hipGetLastError());
}

}  // namespace owlmi
