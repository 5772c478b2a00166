// ransac.hip -- RANSAC over correspondences (tknnRansac, include/owlknn_global.h): the rigid transform most of c pairs agree with.
//
//   0. ransac_stage_kernel gathers the pairs into c records (s, p) and counts the rows out of range; ransac_centroid_kernel, one
//      workgroup, sums the p in double in a fixed order.  The host reads both -- the call is refused here or goes on;
//   per batch of TKNN_RANSAC_BATCH trials:
//   a. ransac_trial_kernel: one lane per trial samples (ransac_sample.h), checks the edges, solves (icp_solve.h, the code tknnIcp
//      runs on the host) and checks the sample's distances; a survivor -- trial, T -- is appended to a compact list;
//   b. ransac_score_wave_kernel, the hot path: a wave per survivor, its T in registers as the fp32 rows, its lanes over all the
//      records, coalesced; the lanes' counts are added by shuffles.  Integers: no order can show.
//      (ransac_score_kernel is the other mapping -- survivors x record chunks, 64 survivors per wave, one per lane, the chunk's
//      records broadcast from LDS, one integer atomicAdd per (survivor, chunk) -- measured 1.1 - 3.2 x slower in score_ms at the few percent of
//      a batch that survive and kept for the measurement of DESIGN 3.4q: TKNN_RANSAC_SCORE=tile.)
//   c. ransac_best_kernel: a 64-bit atomicMax over (inliers, ~trial) -- most inliers, then the smaller trial -- and
//      ransac_pick_kernel copies the winner's T.  The host reads the best and the status counts: the batch's one synchronisation;
//   d. ransac_moment_kernel: the inliers under T, their fp64 moments in tknnIcp's layout, and the mask; per lane, per wave, per
//      workgroup in a fixed order, one row per workgroup summed in index order: bitwise reproducible.  It evaluates the final T
//      and every refit.
// The call's workspace (Engine::workspace): counters | records | survivors | the best T | moment rows.
#include "owlknn_global.h"
#include "icp_solve.h"
#include "ransac_sample.h"
#include "trueknn_engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace owlmi {

namespace {

constexpr int kRansacBlock = 256;
constexpr int kRansacTrialBlock = 64;
constexpr int kRansacScoreChunk = 1024;  // records per LDS chunk: 32 KiB
constexpr int kRansacMomentBlocksPerCu = 4;
// the counters, 64-bit words
enum { kRsBadRows = 0, kRsSurvivors = 1, kRsStatus = 2 /* .. 6 */, kRsBest = 7, kRsWords = 8 };

struct RansacRecord {
  float sx, sy, sz, pad0, px, py, pz, pad1;
};
struct RansacSurvivor {
  double T[12];  // the top three rows
  int32_t trial, inliers;
};

size_t ransac_align(size_t b) { return (b + 255) & ~(size_t)255; }

__device__ __forceinline__ float ransac_sqrt(float x) { return __builtin_sqrtf(x); }

// the fp32 distance of Tf s and p, literally as tknnIcp transforms and measures
__device__ __forceinline__ float ransac_dist(const float *t, float x, float y, float z, float px, float py, float pz) {
#pragma clang fp contract(off)
  const float ax = ((t[0] * x + t[1] * y) + t[2] * z) + t[3];
  const float ay = ((t[4] * x + t[5] * y) + t[6] * z) + t[7];
  const float az = ((t[8] * x + t[9] * y) + t[10] * z) + t[11];
  const float dx = ax - px, dy = ay - py, dz = az - pz;
  return ransac_sqrt((dx * dx + dy * dy) + dz * dz);
}

// ---- 0. staging --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRansacBlock) ransac_stage_kernel(const float *__restrict__ src, int32_t ms, const float *__restrict__ tgt, int32_t mt,
                                                                  const int32_t *__restrict__ pairs, int32_t c, RansacRecord *__restrict__ rec,
                                                                  unsigned long long *__restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * kRansacBlock + threadIdx.x;  // (64 bits: c may be within a block of 2^31)
  if (i >= c) return;
  const int32_t a = pairs[2 * i], b = pairs[2 * i + 1];
  RansacRecord r = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (a < 0 || a >= ms || b < 0 || b >= mt) {
    atomicAdd(&counters[kRsBadRows], 1ull);
  } else {
    r.sx = src[3 * (int64_t)a], r.sy = src[3 * (int64_t)a + 1], r.sz = src[3 * (int64_t)a + 2];
    r.px = tgt[3 * (int64_t)b], r.py = tgt[3 * (int64_t)b + 1], r.pz = tgt[3 * (int64_t)b + 2];
  }
  rec[i] = r;
}

// out[0 .. 2] = the sum of p over the records: lane l takes the records l, l + 256, ... in order, the lanes are added in index order
__global__ void __launch_bounds__(kRansacBlock) ransac_centroid_kernel(const RansacRecord *__restrict__ rec, int32_t c, double *__restrict__ out) {
  __shared__ double part[kRansacBlock][3];
  double x = 0, y = 0, z = 0;
  for (int64_t i = threadIdx.x; i < c; i += kRansacBlock) x += (double)rec[i].px, y += (double)rec[i].py, z += (double)rec[i].pz;
  part[threadIdx.x][0] = x, part[threadIdx.x][1] = y, part[threadIdx.x][2] = z;
  __syncthreads();
  if (threadIdx.x < 3) {
    double v = 0;
    for (int l = 0; l < kRansacBlock; l++) v += part[l][threadIdx.x];
    out[threadIdx.x] = v;
  }
}

// ---- a. the trials -----------------------------------------------------------------------------------------------------------------
struct RansacTrialArgs {
  const RansacRecord *rec;
  int32_t c, n;  // records, ransac_n
  uint32_t seed;
  int32_t first, count;  // the batch: trials first .. first + count
  float max_dist, sim;
  double centre[3];
  RansacSurvivor *survivors;
  unsigned long long *counters;
  int32_t *status;   // the caller's, by trial; may be null
  int32_t *inliers;  // the caller's, by trial; may be null (-1 here: not scored)
};

__device__ int ransac_trial(const RansacTrialArgs &a, int32_t trial, double *T) {
#pragma clang fp contract(off)
  uint32_t idx[4];
  if (!ransac_sample(a.seed, (uint32_t)trial, a.n, (uint32_t)a.c, idx)) return TKNN_RANSAC_DUPLICATE;
  RansacRecord r[4];
  for (int i = 0; i < a.n; i++) r[i] = a.rec[idx[i]];
  if (a.sim > 0.f)
    for (int i = 0; i < a.n; i++)
      for (int j = i + 1; j < a.n; j++) {
        const float sx = r[i].sx - r[j].sx, sy = r[i].sy - r[j].sy, sz = r[i].sz - r[j].sz;
        const float px = r[i].px - r[j].px, py = r[i].py - r[j].py, pz = r[i].pz - r[j].pz;
        const float ds = ransac_sqrt((sx * sx + sy * sy) + sz * sz), dt = ransac_sqrt((px * px + py * py) + pz * pz);
        if (!(ds >= a.sim * dt && dt >= a.sim * ds)) return TKNN_RANSAC_EDGE;
      }
  double mom[kIcpMoments];
  for (int i = 0; i < kIcpMoments; i++) mom[i] = 0.0;
  mom[kIcpPairs] = mom[kIcpPositive] = mom[kIcpSystem] = (double)a.n;
  for (int i = 0; i < a.n; i++) {
    const double sa[3] = {(double)r[i].sx - a.centre[0], (double)r[i].sy - a.centre[1], (double)r[i].sz - a.centre[2]};
    const double pb[3] = {(double)r[i].px - a.centre[0], (double)r[i].py - a.centre[1], (double)r[i].pz - a.centre[2]};
    for (int u = 0; u < 3; u++) {
      mom[5 + u] += sa[u];
      mom[8 + u] += pb[u];
      for (int v = 0; v < 3; v++) mom[11 + 3 * u + v] += sa[u] * pb[v];
    }
  }
  double dT[16];
  if (!icp_solve_point(mom, a.centre, dT)) return TKNN_RANSAC_DEGENERATE;
  float tf[12];
  icp_round_rows(dT, tf);
  for (int i = 0; i < a.n; i++)
    if (!(ransac_dist(tf, r[i].sx, r[i].sy, r[i].sz, r[i].px, r[i].py, r[i].pz) <= a.max_dist)) return TKNN_RANSAC_FAR;
  for (int i = 0; i < 12; i++) T[i] = dT[i];
  return TKNN_RANSAC_OK;
}

__global__ void __launch_bounds__(kRansacTrialBlock) ransac_trial_kernel(RansacTrialArgs a) {
  const int32_t i = blockIdx.x * kRansacTrialBlock + threadIdx.x;
  if (i >= a.count) return;
  const int32_t trial = a.first + i;
  double T[12];
  const int status = ransac_trial(a, trial, T);
  atomicAdd(&a.counters[kRsStatus + status], 1ull);
  if (a.status) a.status[trial] = status;
  if (a.inliers) a.inliers[trial] = -1;
  if (status != TKNN_RANSAC_OK) return;
  const int32_t at = (int32_t)atomicAdd(&a.counters[kRsSurvivors], 1ull);  // (< TKNN_RANSAC_BATCH: one per lane of the batch at most)
  RansacSurvivor sv;
  for (int t = 0; t < 12; t++) sv.T[t] = T[t];
  sv.trial = trial, sv.inliers = 0;
  a.survivors[at] = sv;
}

// ---- b. the scores -----------------------------------------------------------------------------------------------------------------
// the mapping that is not used: grid (survivor tiles of 64 -- all TKNN_RANSAC_BATCH / 64 of them, a tile past the list returns --,
// record chunks)
__global__ void __launch_bounds__(64) ransac_score_kernel(const RansacRecord *__restrict__ rec, int32_t c, float max_dist, RansacSurvivor *__restrict__ survivors,
                                                        const unsigned long long *__restrict__ counters) {
  __shared__ float4 chunk[kRansacScoreChunk][2];
  const int32_t count = (int32_t)counters[kRsSurvivors];
  if ((int32_t)blockIdx.x * 64 >= count) return;
  const int32_t lo = (int32_t)((int64_t)blockIdx.y * kRansacScoreChunk), rows = min(kRansacScoreChunk, c - lo);
  const float4 *in = (const float4 *)(rec + lo);
  for (int i = threadIdx.x; i < 2 * rows; i += 64) chunk[i >> 1][i & 1] = in[i];
  __syncthreads();
  const int32_t sv = blockIdx.x * 64 + threadIdx.x;
  float t[12];
  for (int i = 0; i < 12; i++) t[i] = sv < count ? (float)survivors[sv].T[i] : 0.f;
  int32_t inliers = 0;
  for (int j = 0; j < rows; j++) {
    const float4 s = chunk[j][0], p = chunk[j][1];
    inliers += ransac_dist(t, s.x, s.y, s.z, p.x, p.y, p.z) <= max_dist ? 1 : 0;
  }
  if (sv < count && inliers) atomicAdd(&survivors[sv].inliers, inliers);
}

// a wave per survivor, its lanes over all the records (a workgroup past the list returns)
__global__ void __launch_bounds__(64) ransac_score_wave_kernel(const RansacRecord *__restrict__ rec, int32_t c, float max_dist, RansacSurvivor *__restrict__ survivors,
                                                             const unsigned long long *__restrict__ counters) {
  const int32_t count = (int32_t)counters[kRsSurvivors];
  const int32_t sv = blockIdx.x;
  if (sv >= count) return;
  float t[12];
  for (int i = 0; i < 12; i++) t[i] = (float)survivors[sv].T[i];
  int32_t inliers = 0;
  for (int64_t j = threadIdx.x; j < c; j += 64) {
    const RansacRecord r = rec[j];
    inliers += ransac_dist(t, r.sx, r.sy, r.sz, r.px, r.py, r.pz) <= max_dist ? 1 : 0;
  }
  for (int off = 1; off < 64; off <<= 1) inliers += __shfl_xor(inliers, off, 64);
  if (threadIdx.x == 0) survivors[sv].inliers = inliers;
}

// ---- c. the best -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long ransac_rank(int32_t inliers, int32_t trial) {
  return ((unsigned long long)(uint32_t)inliers << 32) | (unsigned long long)(0xffffffffu - (uint32_t)trial);
}

__global__ void __launch_bounds__(kRansacBlock) ransac_best_kernel(const RansacSurvivor *__restrict__ survivors, unsigned long long *__restrict__ counters,
                                                                 int32_t *__restrict__ trial_inliers) {
  const int32_t sv = blockIdx.x * kRansacBlock + threadIdx.x;
  if (sv >= (int32_t)counters[kRsSurvivors]) return;
  const RansacSurvivor &v = survivors[sv];
  if (trial_inliers) trial_inliers[v.trial] = v.inliers;
  atomicMax(&counters[kRsBest], ransac_rank(v.inliers, v.trial));
}

// (the best of an earlier batch is no survivor of this one: its T stays)
__global__ void __launch_bounds__(kRansacBlock) ransac_pick_kernel(const RansacSurvivor *__restrict__ survivors, const unsigned long long *__restrict__ counters,
                                                                 double *__restrict__ best_T) {
  const int32_t sv = blockIdx.x * kRansacBlock + threadIdx.x;
  if (sv >= (int32_t)counters[kRsSurvivors]) return;
  const RansacSurvivor &v = survivors[sv];
  if (ransac_rank(v.inliers, v.trial) != counters[kRsBest]) return;
  for (int i = 0; i < 12; i++) best_T[i] = v.T[i];
}

// ---- d. the moments of the inliers under T -----------------------------------------------------------------------------------------
struct RansacMomentArgs {
  const RansacRecord *rec;
  int32_t c;
  float max_dist;
  float t[12];
  double centre[3];
  double *rows;   // gridDim.x rows of kIcpMoments doubles, then the total
  uint8_t *mask;  // the caller's, may be null
};

__device__ __forceinline__ double ransac_wave_sum(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ void __launch_bounds__(kRansacBlock) ransac_moment_kernel(RansacMomentArgs a) {
#pragma clang fp contract(off)
  __shared__ double part[kRansacBlock / 64][kIcpMoments];
  double acc[kIcpPointWords];
#pragma unroll
  for (int i = 0; i < kIcpPointWords; i++) acc[i] = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * kRansacBlock + threadIdx.x; j < (int64_t)a.c; j += (int64_t)gridDim.x * kRansacBlock) {
    const RansacRecord r = a.rec[j];
    const float fx = ((a.t[0] * r.sx + a.t[1] * r.sy) + a.t[2] * r.sz) + a.t[3];
    const float fy = ((a.t[4] * r.sx + a.t[5] * r.sy) + a.t[6] * r.sz) + a.t[7];
    const float fz = ((a.t[8] * r.sx + a.t[9] * r.sy) + a.t[10] * r.sz) + a.t[11];
    const float ex = fx - r.px, ey = fy - r.py, ez = fz - r.pz;
    const bool in = ransac_sqrt((ex * ex + ey * ey) + ez * ez) <= a.max_dist;
    if (a.mask) a.mask[j] = in ? 1 : 0;
    if (!in) continue;
    const double dx = (double)fx - (double)r.px, dy = (double)fy - (double)r.py, dz = (double)fz - (double)r.pz;
    acc[kIcpPairs] += 1.0;
    acc[kIcpSumD2] += (dx * dx + dy * dy) + dz * dz;
    acc[kIcpPositive] += 1.0;
    acc[4] += 1.0;
    const double sa[3] = {(double)fx - a.centre[0], (double)fy - a.centre[1], (double)fz - a.centre[2]};
    const double b[3] = {(double)r.px - a.centre[0], (double)r.py - a.centre[1], (double)r.pz - a.centre[2]};
#pragma unroll
    for (int i = 0; i < 3; i++) {
      acc[5 + i] += sa[i];
      acc[8 + i] += b[i];
#pragma unroll
      for (int t = 0; t < 3; t++) acc[11 + 3 * i + t] += sa[i] * b[t];
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < kIcpPointWords; i++) {
    const double v = ransac_wave_sum(acc[i]);
    if (lane == 0) part[wave][i] = v;
  }
  __syncthreads();
  if (threadIdx.x < kIcpMoments) {
    double v = 0.0;
    if ((int)threadIdx.x < kIcpPointWords)
      for (int w = 0; w < kRansacBlock / 64; w++) v += part[w][threadIdx.x];
    a.rows[(int64_t)blockIdx.x * kIcpMoments + threadIdx.x] = v;
  }
}

// rows[nrows] = the sum of rows[0 .. nrows), in index order
__global__ void __launch_bounds__(64) ransac_moment_sum_kernel(double *rows, int32_t nrows) {
  if (threadIdx.x >= kIcpMoments) return;
  double v = 0.0;
  for (int32_t b = 0; b < nrows; b++) v += rows[(int64_t)b * kIcpMoments + threadIdx.x];
  rows[(int64_t)nrows * kIcpMoments + threadIdx.x] = v;
}

}  // namespace

void Engine::ransac(const tknnRansacOptions &o, tknnRansacInfo *info, hipStream_t s) {
  const int32_t c = (int32_t)o.c;
  const bool wave_score = [] {
    const char *e = getenv("TKNN_RANSAC_SCORE");
    return !(e && !std::strcmp(e, "tile"));
  }() || ((int64_t)c + kRansacScoreChunk - 1) / kRansacScoreChunk > 65535;  // (the tile mapping's chunks are grid.y)
  const int moment_blocks = (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)c + kRansacBlock - 1) / kRansacBlock, (int64_t)cu_count_ * kRansacMomentBlocksPerCu));
  const size_t col_counters = ransac_align((kRsWords + 3) * sizeof(unsigned long long)), col_rec = ransac_align((size_t)std::max(c, 1) * sizeof(RansacRecord)),
               col_surv = ransac_align((size_t)TKNN_RANSAC_BATCH * sizeof(RansacSurvivor)), col_best = ransac_align(12 * sizeof(double)),
               col_rows = ransac_align((size_t)(moment_blocks + 1) * kIcpMoments * sizeof(double));
  char *ws = (char *)workspace(col_counters + col_rec + col_surv + col_best + col_rows);
  unsigned long long *counters = (unsigned long long *)ws;
  double *centroid = (double *)(counters + kRsWords);  // three words behind the counters
  RansacRecord *rec = (RansacRecord *)(ws + col_counters);
  RansacSurvivor *survivors = (RansacSurvivor *)((char *)rec + col_rec);
  double *best_T = (double *)((char *)survivors + col_surv);
  double *rows = (double *)((char *)best_T + col_best);
  static_assert(kCounterWords >= kIcpMoments && kCounterWords >= kRsWords + 3, "the host's copy of the counters holds a moment row");

  tknnRansacInfo r;
  std::memset(&r, 0, sizeof r);
  icp_identity(r.transform);
  r.best_trial = -1;
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  // ---- 0. stage, refuse or go on ----
  OWLMI_HIP(hipMemsetAsync(counters, 0, (kRsWords + 3) * sizeof(unsigned long long), s));
  if (c > 0) {
    hipLaunchKernelGGL(ransac_stage_kernel, dim3((unsigned)(((int64_t)c + kRansacBlock - 1) / kRansacBlock)), dim3(kRansacBlock), 0, s, o.d_source, (int32_t)o.ms, o.d_target, (int32_t)o.mt,
                       o.d_pairs, c, rec, counters);
    OWLMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(ransac_centroid_kernel, dim3(1), dim3(kRansacBlock), 0, s, (const RansacRecord *)rec, c, centroid);
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipMemcpyAsync(h_counters_, counters, (kRsWords + 3) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  if (h_counters_[kRsBadRows] > 0)
    throw ArgError{TKNN_E_ARG, "tknnRansac: d_pairs names " + std::to_string(h_counters_[kRsBadRows]) + " rows outside [0, ms) x [0, mt)"};
  double centre[3] = {0, 0, 0};
  if (c > 0) {
    std::memcpy(centre, h_counters_ + kRsWords, sizeof centre);
    for (double &v : centre) v = std::isfinite(v / c) ? v / c : 0.0;
  }
  if (o.d_trial_status) OWLMI_HIP(hipMemsetAsync(o.d_trial_status, 0xff, (size_t)o.max_trials * sizeof(int32_t), s));
  if (o.d_trial_inliers) OWLMI_HIP(hipMemsetAsync(o.d_trial_inliers, 0xff, (size_t)o.max_trials * sizeof(int32_t), s));

  // ---- the batches ----
  RansacTrialArgs ta;
  std::memset(&ta, 0, sizeof ta);
  ta.rec = rec, ta.c = c, ta.n = o.ransac_n, ta.seed = o.seed;
  ta.max_dist = o.max_dist, ta.sim = o.edge_similarity;
  std::memcpy(ta.centre, centre, sizeof centre);
  ta.survivors = survivors, ta.counters = counters;
  ta.status = o.d_trial_status, ta.inliers = o.d_trial_inliers;
  const unsigned score_chunks = (unsigned)(((int64_t)c + kRansacScoreChunk - 1) / kRansacScoreChunk);
  unsigned long long best = 0;
  while (c >= o.ransac_n && r.trials_run < o.max_trials) {
    ta.first = r.trials_run, ta.count = std::min<int32_t>(TKNN_RANSAC_BATCH, o.max_trials - r.trials_run);
    OWLMI_HIP(hipMemsetAsync(counters + kRsSurvivors, 0, sizeof(unsigned long long), s));
    OWLMI_HIP(hipEventRecord(ev_b_, s));
    hipLaunchKernelGGL(ransac_trial_kernel, dim3((ta.count + kRansacTrialBlock - 1) / kRansacTrialBlock), dim3(kRansacTrialBlock), 0, s, ta);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipEventRecord(ev_c_, s));
    if (wave_score)
      hipLaunchKernelGGL(ransac_score_wave_kernel, dim3(ta.count), dim3(64), 0, s, (const RansacRecord *)rec, c, o.max_dist, survivors, (const unsigned long long *)counters);
    else
      hipLaunchKernelGGL(ransac_score_kernel, dim3((ta.count + 63) / 64, score_chunks), dim3(64), 0, s, (const RansacRecord *)rec, c, o.max_dist, survivors,
                         (const unsigned long long *)counters);
    OWLMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(ransac_best_kernel, dim3((ta.count + kRansacBlock - 1) / kRansacBlock), dim3(kRansacBlock), 0, s, (const RansacSurvivor *)survivors, counters,
                       o.d_trial_inliers);
    OWLMI_HIP(hipGetLastError());
    hipLaunchKernelGGL(ransac_pick_kernel, dim3((ta.count + kRansacBlock - 1) / kRansacBlock), dim3(kRansacBlock), 0, s, (const RansacSurvivor *)survivors,
                       (const unsigned long long *)counters, best_T);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipEventRecord(ev_d_, s));
    OWLMI_HIP(hipMemcpyAsync(h_counters_, counters, kRsWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));  // the batch's best: the stopping rule is the host's
    float sample_ms = 0, score_ms = 0;
    OWLMI_HIP(hipEventElapsedTime(&sample_ms, ev_b_, ev_c_));
    OWLMI_HIP(hipEventElapsedTime(&score_ms, ev_c_, ev_d_));
    r.sample_ms += sample_ms, r.score_ms += score_ms;
    r.trials_run += ta.count;
    r.batches++;
    best = h_counters_[kRsBest];
    const double f = (double)(best >> 32) / (double)c;
    double needed = INFINITY;
    if (o.confidence < 1.0 && f > 0.0) {
      const double miss = std::log(1.0 - std::pow(f, (double)o.ransac_n));  // (f = 1: -inf, needed = 0)
      needed = miss < 0.0 ? std::log(1.0 - o.confidence) / miss : INFINITY;
    }
    if ((double)r.trials_run >= needed) break;
  }
  for (int i = 0; i < 5; i++) r.status_counts[i] = (int64_t)h_counters_[kRsStatus + i];

  // ---- evaluate, refit ----
  OWLMI_HIP(hipEventRecord(ev_e_, s));
  if (r.status_counts[TKNN_RANSAC_OK] > 0) {
    r.best_trial = (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffu));
    double T[16];
    icp_identity(T);
    OWLMI_HIP(hipMemcpyAsync(T, best_T, 12 * sizeof(double), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
    RansacMomentArgs ma;
    std::memset(&ma, 0, sizeof ma);
    ma.rec = rec, ma.c = c, ma.max_dist = o.max_dist;
    std::memcpy(ma.centre, centre, sizeof centre);
    ma.rows = rows;
    const double *h_mom = (const double *)h_counters_;
    double mom[kIcpMoments];
    // the moments of the inliers under `at`, into mom
    auto evaluate = [&](const double *at, uint8_t *mask) {
      icp_round_rows(at, ma.t);
      ma.mask = mask;
      hipLaunchKernelGGL(ransac_moment_kernel, dim3(moment_blocks), dim3(kRansacBlock), 0, s, ma);
      OWLMI_HIP(hipGetLastError());
      hipLaunchKernelGGL(ransac_moment_sum_kernel, dim3(1), dim3(64), 0, s, rows, (int32_t)moment_blocks);
      OWLMI_HIP(hipGetLastError());
      OWLMI_HIP(hipMemcpyAsync((void *)h_mom, rows + (size_t)moment_blocks * kIcpMoments, kIcpMoments * sizeof(double), hipMemcpyDeviceToHost, s));
      OWLMI_HIP(hipStreamSynchronize(s));
      std::memcpy(mom, h_mom, sizeof mom);
    };
    evaluate(T, nullptr);
    double kept[kIcpMoments];
    std::memcpy(kept, mom, sizeof kept);
    for (int round = 0; round < o.refit_rounds; round++) {
      double dT[16], next[16];
      if (!icp_solve_point(kept, centre, dT)) break;
      icp_mul(dT, T, next);
      evaluate(next, nullptr);
      if (mom[kIcpPairs] < kept[kIcpPairs]) break;
      std::memcpy(T, next, sizeof T);
      std::memcpy(kept, mom, sizeof kept);
      r.refits_kept++;
    }
    if (o.d_inlier_mask) evaluate(T, o.d_inlier_mask);  // (the same sums once more, for the mask of the T that was kept)
    std::memcpy(r.transform, T, sizeof T);
    r.inliers = (int64_t)kept[kIcpPairs];
    r.fitness = kept[kIcpPairs] / (double)c;
    r.inlier_rmse = kept[kIcpPairs] > 0 ? std::sqrt(kept[kIcpSumD2] / kept[kIcpPairs]) : 0.0;
  } else if (o.d_inlier_mask && c > 0) {
    OWLMI_HIP(hipMemsetAsync(o.d_inlier_mask, 0, (size_t)c, s));
  }
  OWLMI_HIP(hipEventRecord(ev_f_, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  OWLMI_HIP(hipEventElapsedTime(&r.refit_ms, ev_e_, ev_f_));
  OWLMI_HIP(hipEventElapsedTime(&r.solve_ms, ev_a_, ev_f_));
  *info = r;
}

}  // namespace owlmi
