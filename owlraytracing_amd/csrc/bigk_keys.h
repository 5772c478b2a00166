// bigk_keys.h -- the three-word keys of the k > 64 kernel (trueknn_bigk.hip) and their sorting network on a 16-lane team: the
// network of team_lanes.h with (distance, first level, index) in place of (distance, index).  In a header so that the lane
// harness (debug_lanes.hip, tknnDebugTeamLanes) runs the very functions the kernel inlines.
#pragma once
#include "team_lanes.h"

namespace owlmi {

namespace {

// Keys carry THREE words, (distance, level at which the neighbour first was a candidate, index): the reference's order of
// bit-identical distances (section 1 of DESIGN.md; tie_fix_kernel's key), so rows come out final and no tie pass follows.
struct BigKey {
  uint32_t d, l, i, pad;
};

__device__ __forceinline__ bool t_less3(uint32_t ad, uint32_t al, uint32_t ai, uint32_t bd, uint32_t bl, uint32_t bi) {
  const uint64_t ah = ((uint64_t)ad << 32) | al, bh = ((uint64_t)bd << 32) | bl;
  return (ah < bh) | ((ah == bh) & (ai < bi));
}
// one compare-exchange of three-word keys with the lane whose key is (pd, pl, pi): the lower lane keeps the smaller key
__device__ __forceinline__ void t_exchange3(uint32_t &kd, uint32_t &kl, uint32_t &ki, uint32_t pd, uint32_t pl, uint32_t pi, bool upper) {
  const bool take = t_less3(pd, pl, pi, kd, kl, ki) != upper;
  kd = take ? pd : kd;
  kl = take ? pl : kl;
  ki = take ? pi : ki;
}
#define T_EX3(CTRL, UP) t_exchange3(kd, kl, ki, t_dpp<CTRL>(kd), t_dpp<CTRL>(kl), t_dpp<CTRL>(ki), UP)
__device__ __forceinline__ void t_sort16_3(uint32_t &kd, uint32_t &kl, uint32_t &ki, int tl) {
  const bool up1 = (tl & 1) != 0, up2 = (tl & 2) != 0, up4 = (tl & 4) != 0, up8 = (tl & 8) != 0;
  T_EX3(0xb1, up1);
  T_EX3(0x1b, up2);
  T_EX3(0xb1, up1);
  T_EX3(0x141, up4);
  T_EX3(0x4e, up2);
  T_EX3(0xb1, up1);
  T_EX3(0x140, up8);
  t_exchange3(kd, kl, ki, t_xor4(kd), t_xor4(kl), t_xor4(ki), up4);
  T_EX3(0x4e, up2);
  T_EX3(0xb1, up1);
}
__device__ __forceinline__ void t_clean16_3(uint32_t &kd, uint32_t &kl, uint32_t &ki, int tl) {
  const bool up1 = (tl & 1) != 0, up2 = (tl & 2) != 0, up4 = (tl & 4) != 0, up8 = (tl & 8) != 0;
  T_EX3(0x128, up8);
  t_exchange3(kd, kl, ki, t_xor4(kd), t_xor4(kl), t_xor4(ki), up4);
  T_EX3(0x4e, up2);
  T_EX3(0xb1, up1);
}
#undef T_EX3

}  // namespace

}  // namespace owlmi
