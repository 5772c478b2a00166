/*
 * owlknn_debug.h -- test hooks of libowl_mi355x.so on top of the C ABI of owlknn.h: one on an engine's scratch memory
 * (tknnDebugPoison) and one that runs a single 16-lane team helper of the TrueKNN kernels on caller-supplied lanes
 * (tknnDebugTeamLanes).  Plain C99; link and load as owlknn.h says.  Nothing a product needs is in here.
 */
#pragma once
#include <stddef.h>

#include "owlknn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- poison: what one call leaves behind must not matter to the next ------------------------------------------------------------
 * Every call of an engine carves its scratch out of one workspace that only grows and is never cleared, and shares one block of
 * device counters, its host copy and a few lists with every other call.  A call is right only if every word it reads of them has
 * been written by that same call first ("State that carries from one call to the next", lists the exceptions).
 * tknnDebugPoison fills the parts named in `what` with `byte`, so that a test can show a call gives the same result whatever
 * was there:
 *   TKNN_POISON_WORKSPACE  the workspace, first grown to at least min_workspace_bytes (a fresh engine has none), all of it
 *   TKNN_POISON_COUNTERS   the device counters, all of them, and the whole of their pinned host copy
 *   TKNN_POISON_LISTS      the list of handed-over slots with its length, the list of tie slots, the halo pass's block masks and
 *                          cursors -- each as far as it is allocated
 *   TKNN_POISON_SOLVE      the per-slot solve state: done, intersections, next level, tie flags -- as far as allocated (at a
 *                          boundary between a phase-1 and a phase-2 solve this state is LIVE: do not poison it there)
 * `stream` is first made to wait for a DBSCAN side launch that no stream has waited for yet.  The device fills are asynchronous
 * fills on `stream`; the host copy is filled after the stream has been synchronised, so the call returns with everything done.
 * The trees, the batch layout, the boundary marks and every host flag are never touched.  *poisoned_bytes (optional): the bytes
 * filled, device and host together.
 * Errors, in this order: NULL engine: TKNN_E_ARG; a bit in `what` that no part has, byte outside 0 .. 255: TKNN_E_ARG.  A refused
 * call writes nothing. */
#define TKNN_POISON_WORKSPACE 1u
#define TKNN_POISON_COUNTERS 2u
#define TKNN_POISON_LISTS 4u
#define TKNN_POISON_SOLVE 8u
#define TKNN_POISON_ALL 15u
TKNN_API int tknnDebugPoison(tknnEngine e, unsigned what, int byte, size_t min_workspace_bytes, int64_t *poisoned_bytes, void *stream);

/* ---- team lanes: one helper of team_lanes.h / team_walk.h / bigk_keys.h on lanes the caller fills ------------------------------
 * Every k <= 64 result is made by helpers that sixteen lanes (a "team", four to a wave) run in lock step: lane exchanges, the
 * sorting networks, the merge of a candidate row into the sorted register list, the tie flags.  tknnDebugTeamLanes runs ONE of
 * them, exactly as the kernels call it, on `teams` teams whose lanes the caller has filled, and returns every lane's outcome, so
 * that a test can compare a helper with its specification on inputs no solve produces on demand.
 *
 * The kernel: one wave per workgroup, team t = lanes 16 (t & 3) .. + 15 of workgroup t >> 2.  When `teams` is no multiple of
 * four the lanes of the missing teams run the helper too (it holds wave-wide ballots and barriers), on zero input words -- for
 * MERGE an empty list, fill 0, not full -- and store nothing.
 *
 * Layout: op takes WIN 32-bit words per lane and returns WOUT: word w of lane tl of team t is d_in[(t * WIN + w) * 16 + tl] and
 * d_out[(t * WOUT + w) * 16 + tl].  A word that is one value per TEAM (fill, full, k, ...) is read by each lane from its own
 * copy: give all sixteen lanes the same.  NREG = `variant` (1 .. 4): the registers per lane of a list of up to 16 NREG entries,
 * entry 16 j + tl in register j of lane tl.  Keys are (distance word, index word), the distance word first; a floating-point
 * word is the bits of a float.
 *
 *   op                    variant  in words (WIN)                                        out words (WOUT)
 *   TKNN_LANES_SORT16     0        kd, ki (2)                                            t_sort16: kd, ki (2)
 *   TKNN_LANES_CLEAN16    0        kd, ki: a bitonic sequence over the lanes (2)         t_clean16: kd, ki (2)
 *   TKNN_LANES_SORT16_U32 0        v (1)                                                 t_sort16_u32: v (1)
 *   TKNN_LANES_SORTED_ROW 0        bits of d2, id, have (0 / 1: my bit of the mask) (3)  t_sorted_row: kd, ki (2).  The keys go
 *                                  through the team's LDS buffer as in the packet kernel's sort_first: lanes without `have` too
 *   TKNN_LANES_MERGE      NREG     list kd[NREG], list ki[NREG]; candidate row 0: d2, id; row 1: d2, id (lane tl holds
 *                                  candidate 16 row + tl); fill (0 .. 32); left_out; full (0 / 1)  (2 NREG + 7)
 *                                                                                        t_merge_rows: kd[NREG], ki[NREG],
 *                                                                                        t_team_min_u32(left_out)  (2 NREG + 1)
 *   TKNN_LANES_KTH        NREG     kd[NREG], k (1 .. 16 NREG)  (NREG + 1)                bits of t_kth_dist (1)
 *   TKNN_LANES_ROW_TIES   NREG     kd[NREG], left_out, full, k, q.x, q.y, q.z, r0, r, span, look (0 / 1)  (NREG + 10)
 *                                                                                        t_row_ties: tie, edge (0 / 1: my bits of
 *                                                                                        the team's two lane masks) (2)
 *   TKNN_LANES_STRADDLE   0        d, r0, r_last, qmax, span (5)                         tie_may_straddle: 0 / 1 (1)
 *   TKNN_LANES_FIRST_LEVEL 0       p.x, p.y, p.z, q.x, q.y, q.z, q_r0, level (8)         first_level (1)
 *   TKNN_LANES_REDUCE     0        v (1)                                                 t_team_sum(u32), t_team_sum(float),
 *                                  t_team_min, t_team_max, t_team_min_u32, t_wave_max, t_wave_sum(v as u64): low, high  (8).
 *                                  The two wave-wide ones see the zero words of missing teams
 *   TKNN_LANES_MOVES      lane     v, src (0 .. 15: a lane of my team), bit (0 / 1), acc (4)
 *                         0 .. 63                                                        t_xor4, t_team_shr1, t_dpp<0xb1>, <0x1b>,
 *                                  <0x4e>, <0x141>, <0x140>, <0x128>, <0x121>, t_lane_read(v, 16 team + src), t_rank(m),
 *                                  t_count(acc, m), t_count_keep(acc, m, v), t_team_any(bit), t_bcast(v, variant)  (15), with
 *                                  m = the wave's ballot of `bit`; t_bcast's lane is wave-uniform, hence the variant
 *   TKNN_LANES_SORT16_3   0        kd, kl, ki (3)                                        t_sort16_3: kd, kl, ki (3)
 *   TKNN_LANES_CLEAN16_3  0        kd, kl, ki: bitonic over the lanes (3)                t_clean16_3: kd, kl, ki (3)
 *
 * Two loops of the helpers run as long as their input says, so the harness bounds it: a lane whose r0 is not > 0
 * (tie_may_straddle doubles it until it passes d) is given r0 = 1 and returns 0xffffffff in every out word of STRADDLE and
 * ROW_TIES; first_level's `level` is taken as min(max(level, 0), 64).
 * The call needs no engine, runs on the current device and returns with `stream` synchronised.  teams == 0 succeeds and launches
 * nothing.  Errors, all TKNN_E_ARG, decided in this order before any device call, and a refused call writes nothing: d_in or
 * d_out NULL; teams < 0 or > TKNN_LANES_MAX_TEAMS; an op that is none of the above; a variant the op does not have. */
#define TKNN_LANES_SORT16 0
#define TKNN_LANES_CLEAN16 1
#define TKNN_LANES_SORT16_U32 2
#define TKNN_LANES_SORTED_ROW 3
#define TKNN_LANES_MERGE 4
#define TKNN_LANES_KTH 5
#define TKNN_LANES_ROW_TIES 6
#define TKNN_LANES_STRADDLE 7
#define TKNN_LANES_FIRST_LEVEL 8
#define TKNN_LANES_REDUCE 9
#define TKNN_LANES_MOVES 10
#define TKNN_LANES_SORT16_3 11
#define TKNN_LANES_CLEAN16_3 12
#define TKNN_LANES_OPS 13
#define TKNN_LANES_MAX_TEAMS 1048576 /* 2^20 */
TKNN_API int tknnDebugTeamLanes(int op, int variant, const uint32_t *d_in, uint32_t *d_out, int64_t teams, void *stream);

#ifdef __cplusplus
}
#endif
