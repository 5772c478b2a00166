// voxel_grid.hip -- voxel-grid downsampling per cloud (tknnVoxelGrid, include/owlknn_voxel.h): one sort and one pass, no tree.
//
//   1. vox_key_kernel: per row the 63-bit cell key cx << 42 | cy << 21 | cz from c = floorf((p - origin) / voxel) in literal fp32
//      (a true division), all ones (bit 63) for a row that is left out, the row's number beside it, and the three counters, one
//      atomic per wave and counter;
//   2. hipcub::DeviceRadixSort::SortPairs over (key, row), all 64 bits: the bits a call needs follow from the largest cell, which
//      only a host read could tell, and bit 63 has to sort the rows left out behind the others.  The sort is stable: rows ascend
//      inside a voxel.  With d_batch a second stable pass over (label, row) follows, label = B for a row left out, over the
//      32 - clz(B) bits that B takes: the cell order of the first pass survives inside each cloud;
//   3. vox_head_kernel flags the first position of every (label, key), hipcub::DeviceScan::InclusiveSum numbers them: position i
//      belongs to voxel number[i] - 1, V = number[n - 1];
//   4. vox_map_kernel writes d_map and the first position of every voxel (start[v], start[V] = the rows in the grid),
//      vox_offsets_kernel searches the clouds' voxel ranges;
//   5. the reduce, three ways that never meet in a voxel (the thresholds: DESIGN 3.4r):
//      vox_lane_kernel: ONE LANE PER VOXEL.  It writes count, cell, label and first of every voxel and, for a voxel of at most
//        `lane_rows` rows, sums (double)p over its rows in ascending row order, rounds the centroid once, walks the rows again for
//        the nearest key (bits of d2, row) and sums the value columns eight at a time.  A longer voxel is appended to a list
//        (an integer atomic; the list's order decides nothing).
//      vox_team_kernel<64>: ONE WAVE PER LISTED VOXEL.  Lane l sums the rows at positions l, l + 64, ... of the run in that order,
//        the 64 partial sums fold by __shfl_down at distances 32, 16 .. 1: an order fixed by the run alone.  The nearest key folds
//        the same way as a 64-bit minimum.  The grid is fixed; a wave strides over the list, whose length it reads on the device.
//      vox_team_kernel<1024>: ONE WORKGROUP PER VOXEL of more than `block_rows` rows (a second list, filled from the back of the
//        first): lane l of 1 024 takes the positions l, l + 1024, ..., every wave folds as above and the 16 waves' sums are added
//        in wave order through LDS.  A voxel that holds every row of the call is served by one workgroup.
//      None depends on how voxels fall on workgroups, and no float is added atomically.
//   6. vox_tail_kernel fills entries V .. capacity - 1 of every per-voxel output.
// The call's workspace (Engine::workspace, one layout): words | key by row | key sorted | row, row sorted | (with d_batch: label,
// label sorted, row sorted again) | head flags | numbers | start | list | the sort's space.  Every word read is written by this call.
#include "owlknn_voxel.h"
#include "trueknn_engine.h"

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>

#include <hipcub/hipcub.hpp>

namespace owlmi {

namespace {

constexpr int kVoxBlock = 256;
constexpr int kVoxChunk = 8;            // value columns summed in one walk over a voxel's rows: C <= 8 takes one walk, 16 two
constexpr int kVoxTeam = 1024;          // the lanes of a workgroup that serves one voxel
constexpr int kVoxWaveBlocksPerCu = 8;  // the wave kernel's fixed grid: this many workgroups of four waves per compute unit
constexpr unsigned long long kVoxLeftOut = ~0ull;
constexpr float kVoxCells = (float)(1 << TKNN_VOXEL_CELL_BITS);
enum { kVoxBadRows = 0, kVoxBadLabels = 1, kVoxOutOfGrid = 2, kVoxMaxCount = 3, kVoxListed = 4, kVoxListedBlock = 5, kVoxWords = 8 };

size_t vox_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct VoxArgs {
  const float *points, *values;
  const int32_t *batch;
  int32_t n, C, B;
  float voxel, ox, oy, oz;
  unsigned long long *words;
  unsigned long long *key_by_row;        // [row]
  const unsigned long long *key_sorted;  // [position]; null with d_batch: the key of a position is key_by_row[rows[position]]
  const uint32_t *rows;                  // [position]: the row, in voxel order
  const uint32_t *labels;                // [position]: the label, B for a row left out; null without d_batch
  int32_t *head, *number;                // [position]
  int32_t *start;                        // [voxel], V + 1 words
  int32_t *list;                         // from the front the voxels of more than lane_rows rows, from the back those of more than block_rows
  int32_t lane_rows, block_rows;
  int64_t capacity;
  int32_t *cell, *count, *first, *nearest, *voxel_label, *map;
  float *centroid, *value_mean;
  int64_t *offsets;
};

__device__ __forceinline__ unsigned long long vox_key_at(const VoxArgs &a, int32_t i) { return a.key_sorted ? a.key_sorted[i] : a.key_by_row[a.rows[i]]; }
__device__ __forceinline__ int32_t vox_total(const VoxArgs &a) { return a.n > 0 ? a.number[a.n - 1] : 0; }

// one atomic per wave for a counter of flagged lanes
__device__ __forceinline__ void vox_count_flag(bool flag, unsigned long long *counter) {
  const unsigned long long m = __ballot(flag);
  if (m != 0ull && (threadIdx.x & 63) == (unsigned)__ffsll((long long)m) - 1u) atomicAdd(counter, (unsigned long long)__popcll(m));
}

__global__ void __launch_bounds__(kVoxBlock) vox_key_kernel(VoxArgs a, uint32_t *__restrict__ row_out, uint32_t *__restrict__ label_out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;  // (64 bits: n may be within a block of 2^31)
  const bool live = i < a.n;
  bool bad = false, bad_label = false, outside = false;
  unsigned long long key = kVoxLeftOut;
  if (live) {
    const float x = a.points[3 * i], y = a.points[3 * i + 1], z = a.points[3 * i + 2];
    const int32_t label = a.batch ? a.batch[i] : 0;
    bad = !(fabsf(x) <= FLT_MAX) || !(fabsf(y) <= FLT_MAX) || !(fabsf(z) <= FLT_MAX);
    bad_label = !bad && (label < 0 || label >= a.B);
    const float cx = floorf((x - a.ox) / a.voxel), cy = floorf((y - a.oy) / a.voxel), cz = floorf((z - a.oz) / a.voxel);
    const bool inside = cx >= 0.f && cx < kVoxCells && cy >= 0.f && cy < kVoxCells && cz >= 0.f && cz < kVoxCells;
    outside = !bad && !bad_label && !inside;
    if (!bad && !bad_label && inside) key = (unsigned long long)(uint32_t)cx << (2 * TKNN_VOXEL_CELL_BITS) | (unsigned long long)(uint32_t)cy << TKNN_VOXEL_CELL_BITS | (unsigned long long)(uint32_t)cz;
    a.key_by_row[i] = key;
    row_out[i] = (uint32_t)i;
    if (label_out) label_out[i] = key == kVoxLeftOut ? (uint32_t)a.B : (uint32_t)label;
  }
  vox_count_flag(bad, a.words + kVoxBadRows);
  vox_count_flag(bad_label, a.words + kVoxBadLabels);
  vox_count_flag(outside, a.words + kVoxOutOfGrid);
}

// the labels in the order of the first sort: what the second sorts by
__global__ void __launch_bounds__(kVoxBlock) vox_gather_label_kernel(const uint32_t *__restrict__ label_by_row, const uint32_t *__restrict__ rows, int32_t n, uint32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (i < n) out[i] = label_by_row[rows[i]];
}

__global__ void __launch_bounds__(kVoxBlock) vox_head_kernel(VoxArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (i >= a.n) return;
  const unsigned long long key = vox_key_at(a, (int32_t)i);
  bool head = key != kVoxLeftOut;
  if (head && i > 0) head = key != vox_key_at(a, (int32_t)i - 1) || (a.labels && a.labels[i] != a.labels[i - 1]);
  a.head[i] = head ? 1 : 0;
}

__global__ void __launch_bounds__(kVoxBlock) vox_map_kernel(VoxArgs a) {
  const int64_t i = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (i >= a.n) return;
  const bool in = vox_key_at(a, (int32_t)i) != kVoxLeftOut;
  const int32_t v = a.number[i] - 1;
  if (a.map) a.map[a.rows[i]] = in ? v : -1;
  if (!in) return;
  if (a.head[i]) a.start[v] = (int32_t)i;
  if (i == a.n - 1 || vox_key_at(a, (int32_t)i + 1) == kVoxLeftOut) a.start[v + 1] = (int32_t)i + 1;  // (the rows in the grid come first)
}

// offsets[b]: the first voxel whose label is not below b
__global__ void __launch_bounds__(kVoxBlock) vox_offsets_kernel(VoxArgs a) {
  const int32_t b = blockIdx.x * kVoxBlock + threadIdx.x;
  if (b > a.B) return;
  const int32_t V = vox_total(a);
  int32_t lo = 0, hi = V;
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo) / 2;
    const int32_t label = a.labels ? (int32_t)a.labels[a.start[mid]] : 0;
    if (label < b) lo = mid + 1;
    else hi = mid;
  }
  a.offsets[b] = lo;
}

__device__ __forceinline__ unsigned long long vox_near_key(float x, float y, float z, float cx, float cy, float cz, uint32_t row) {
#pragma clang fp contract(off)
  const float dx = x - cx, dy = y - cy, dz = z - cz;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  return (unsigned long long)__float_as_uint(d2) << 32 | row;
}

__global__ void __launch_bounds__(kVoxBlock) vox_lane_kernel(VoxArgs a) {
  const int64_t v64 = (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  const int32_t V = vox_total(a);
  int32_t cnt = 0;
  if (v64 < V) {
    const int32_t v = (int32_t)v64, lo = a.start[v], hi = a.start[v + 1];
    cnt = hi - lo;
    const unsigned long long key = vox_key_at(a, lo);
    if (a.count) a.count[v] = cnt;
    if (a.cell) {
      a.cell[3 * v64] = (int32_t)(key >> (2 * TKNN_VOXEL_CELL_BITS));
      a.cell[3 * v64 + 1] = (int32_t)(key >> TKNN_VOXEL_CELL_BITS) & ((1 << TKNN_VOXEL_CELL_BITS) - 1);
      a.cell[3 * v64 + 2] = (int32_t)key & ((1 << TKNN_VOXEL_CELL_BITS) - 1);
    }
    if (a.voxel_label) a.voxel_label[v] = a.labels ? (int32_t)a.labels[lo] : 0;
    if (a.first) a.first[v] = (int32_t)a.rows[lo];
    if (a.centroid || a.nearest || a.value_mean) {
      if (cnt > a.block_rows) {
        a.list[(int64_t)a.n - 1 - (int64_t)atomicAdd(a.words + kVoxListedBlock, 1ull)] = v;  // (from the back: both lists hold at most V <= n voxels)
      } else if (cnt > a.lane_rows) {
        a.list[atomicAdd(a.words + kVoxListed, 1ull)] = v;
      } else {
        if (a.centroid || a.nearest) {
          double sx = 0, sy = 0, sz = 0;
          for (int32_t i = lo; i < hi; i++) {
            const int64_t r = a.rows[i];
            sx += (double)a.points[3 * r], sy += (double)a.points[3 * r + 1], sz += (double)a.points[3 * r + 2];
          }
          const float cx = (float)(sx / (double)cnt), cy = (float)(sy / (double)cnt), cz = (float)(sz / (double)cnt);
          if (a.centroid) a.centroid[3 * v64] = cx, a.centroid[3 * v64 + 1] = cy, a.centroid[3 * v64 + 2] = cz;
          if (a.nearest) {
            unsigned long long best = ~0ull;
            for (int32_t i = lo; i < hi; i++) {
              const uint32_t r = a.rows[i];
              const unsigned long long k = vox_near_key(a.points[3 * (int64_t)r], a.points[3 * (int64_t)r + 1], a.points[3 * (int64_t)r + 2], cx, cy, cz, r);
              best = k < best ? k : best;
            }
            a.nearest[v] = (int32_t)(uint32_t)best;
          }
        }
        if (a.value_mean)
          for (int c0 = 0; c0 < a.C; c0 += kVoxChunk) {
            double s[kVoxChunk] = {};
            for (int32_t i = lo; i < hi; i++) {
              const float *row = a.values + (int64_t)a.rows[i] * a.C + c0;
#pragma unroll
              for (int j = 0; j < kVoxChunk; j++)
                if (c0 + j < a.C) s[j] += (double)row[j];
            }
#pragma unroll
            for (int j = 0; j < kVoxChunk; j++)
              if (c0 + j < a.C) a.value_mean[v64 * a.C + c0 + j] = (float)(s[j] / (double)cnt);
          }
      }
    }
  }
  // the fullest voxel: a maximum per wave, one integer atomic
  int32_t m = cnt;
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_down(m, off));
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(a.words + kVoxMaxCount, (unsigned long long)m);
}

// The sum of x over the W lanes that serve one voxel, the same bits in every lane: inside a wave by __shfl_down at distances
// 32 .. 1; across the 16 waves of a workgroup (W = 1024) the waves' sums go through LDS and are added in wave order.
template <int W>
__device__ __forceinline__ double vox_team_sum(double x, double *part) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
  if constexpr (W == 64) {
    return __shfl(x, 0);
  } else {
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    double sum = part[0];
    for (int w = 1; w < W / 64; w++) sum += part[w];
    __syncthreads();  // (part is free for the next sum)
    return sum;
  }
}

template <int W>
__device__ __forceinline__ unsigned long long vox_team_min(unsigned long long x, unsigned long long *part) {
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long other = __shfl_down(x, off);
    x = other < x ? other : x;
  }
  if constexpr (W == 64) {
    return __shfl(x, 0);
  } else {
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    unsigned long long best = part[0];
    for (int w = 1; w < W / 64; w++) best = part[w] < best ? part[w] : best;
    __syncthreads();
    return best;
  }
}

// W lanes per listed voxel: 64, a wave (four to a workgroup); 1024, a workgroup.  `list` is read forwards (`step` = 1) or
// backwards (-1) from its first entry; the loop is uniform in the team, and with W = 1024 in the workgroup.
template <int W>
__global__ void __launch_bounds__(W > kVoxBlock ? W : kVoxBlock) vox_team_kernel(VoxArgs a, const int32_t *__restrict__ list, int step, int word) {
  __shared__ double part_sum[16];
  __shared__ unsigned long long part_min[16];
  constexpr int kBlock = W > kVoxBlock ? W : kVoxBlock;
  const int lane = threadIdx.x % W;
  const int64_t teams = (int64_t)gridDim.x * (kBlock / W);
  const int64_t listed = (int64_t)a.words[word];
  for (int64_t at = (int64_t)blockIdx.x * (kBlock / W) + threadIdx.x / W; at < listed; at += teams) {
    const int64_t v = list[at * step];
    const int32_t lo = a.start[v], hi = a.start[v + 1];
    const double cnt = (double)(hi - lo);
    if (a.centroid || a.nearest) {
      double sx = 0, sy = 0, sz = 0;
      for (int32_t i = lo + lane; i < hi; i += W) {
        const int64_t r = a.rows[i];
        sx += (double)a.points[3 * r], sy += (double)a.points[3 * r + 1], sz += (double)a.points[3 * r + 2];
      }
      const float cx = (float)(vox_team_sum<W>(sx, part_sum) / cnt), cy = (float)(vox_team_sum<W>(sy, part_sum) / cnt), cz = (float)(vox_team_sum<W>(sz, part_sum) / cnt);
      if (a.centroid && lane == 0) a.centroid[3 * v] = cx, a.centroid[3 * v + 1] = cy, a.centroid[3 * v + 2] = cz;
      if (a.nearest) {
        unsigned long long best = ~0ull;
        for (int32_t i = lo + lane; i < hi; i += W) {
          const uint32_t r = a.rows[i];
          const unsigned long long k = vox_near_key(a.points[3 * (int64_t)r], a.points[3 * (int64_t)r + 1], a.points[3 * (int64_t)r + 2], cx, cy, cz, r);
          best = k < best ? k : best;
        }
        best = vox_team_min<W>(best, part_min);
        if (lane == 0) a.nearest[v] = (int32_t)(uint32_t)best;
      }
    }
    if (a.value_mean)
      for (int c0 = 0; c0 < a.C; c0 += kVoxChunk) {
        double s[kVoxChunk] = {};
        for (int32_t i = lo + lane; i < hi; i += W) {
          const float *row = a.values + (int64_t)a.rows[i] * a.C + c0;
#pragma unroll
          for (int j = 0; j < kVoxChunk; j++)
            if (c0 + j < a.C) s[j] += (double)row[j];
        }
#pragma unroll
        for (int j = 0; j < kVoxChunk; j++) {
          const double sum = vox_team_sum<W>(s[j], part_sum);
          if (lane == 0 && c0 + j < a.C) a.value_mean[v * a.C + c0 + j] = (float)(sum / cnt);
        }
      }
  }
}

__global__ void __launch_bounds__(kVoxBlock) vox_tail_kernel(VoxArgs a) {
  const int64_t v = (int64_t)vox_total(a) + (int64_t)blockIdx.x * kVoxBlock + threadIdx.x;
  if (v >= a.capacity) return;
  const float nan = __builtin_nanf("");
  if (a.count) a.count[v] = 0;
  if (a.cell) a.cell[3 * v] = a.cell[3 * v + 1] = a.cell[3 * v + 2] = -1;
  if (a.voxel_label) a.voxel_label[v] = -1;
  if (a.first) a.first[v] = -1;
  if (a.nearest) a.nearest[v] = -1;
  if (a.centroid) a.centroid[3 * v] = a.centroid[3 * v + 1] = a.centroid[3 * v + 2] = nan;
  if (a.value_mean)
    for (int c = 0; c < a.C; c++) a.value_mean[v * a.C + c] = nan;
}

unsigned vox_blocks(int64_t items) { return (unsigned)((items + kVoxBlock - 1) / kVoxBlock); }

}  // namespace

void Engine::voxel_grid(const tknnVoxelGridOptions &o, tknnVoxelGridInfo *info, hipStream_t s) {
  const int32_t n = (int32_t)o.n, B = o.num_batches;
  const bool batched = o.d_batch != nullptr;
  const bool fill = o.d_cell || o.d_count || o.d_centroid || o.d_value_mean || o.d_first || o.d_nearest || o.d_voxel_label;  // (else: the count pass)
  int lane_rows = TKNN_VOXEL_LANE_ROWS;
  if (const char *e = getenv("TKNN_VOXEL_LANE_ROWS"))
    if (atoi(e) > 0) lane_rows = atoi(e);
  if (const char *e = getenv("TKNN_VOXEL_FORCE_WAVE"))
    if (atoi(e) != 0) lane_rows = 0;
  int block_rows = TKNN_VOXEL_WAVE_ROWS;
  if (const char *e = getenv("TKNN_VOXEL_WAVE_ROWS"))
    if (atoi(e) > 0) block_rows = atoi(e);
  block_rows = std::max(block_rows, lane_rows);
  int label_bits = 1;  // the labels 0 .. B
  while ((1ll << label_bits) <= (int64_t)B) label_bits++;

  const size_t rows1 = (size_t)std::max(n, 1);
  size_t sort_bytes = 0, scan_bytes = 0;
  if (n > 0) {
    unsigned long long *k64 = nullptr;
    uint32_t *k32 = nullptr;
    int32_t *i32 = nullptr;
    size_t label_sort_bytes = 0;
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, k64, k64, k32, k32, (int)n, 0, 64, s));
    if (batched) OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, label_sort_bytes, k32, k32, k32, k32, (int)n, 0, label_bits, s));
    OWLMI_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, i32, i32, (int)n, s));
    sort_bytes = std::max(std::max(sort_bytes, label_sort_bytes), scan_bytes);
  }
  const size_t words_b = vox_align(kVoxWords * sizeof(unsigned long long)), wide_b = vox_align(rows1 * sizeof(unsigned long long)),
               col_b = vox_align((rows1 + 1) * sizeof(uint32_t));
  const int cols = 6 + (batched ? 4 : 0);
  char *ws = (char *)workspace(words_b + 2 * wide_b + (size_t)cols * col_b + vox_align(sort_bytes));
  auto column = [&](int i) { return ws + words_b + 2 * wide_b + (size_t)i * col_b; };
  unsigned long long *key_sorted = (unsigned long long *)(ws + words_b + wide_b);
  uint32_t *row_in = (uint32_t *)column(0), *row_sorted = (uint32_t *)column(1);
  uint32_t *label_by_row = nullptr, *label_in = nullptr, *label_sorted = nullptr, *row_final = row_sorted;
  if (batched) label_by_row = (uint32_t *)column(6), label_in = (uint32_t *)column(7), label_sorted = (uint32_t *)column(8), row_final = (uint32_t *)column(9);
  void *tmp = column(cols);

  VoxArgs a;
  std::memset(&a, 0, sizeof a);
  a.points = o.d_points, a.values = o.d_values, a.batch = o.d_batch;
  a.n = n, a.C = o.channels, a.B = B;
  a.voxel = o.voxel, a.ox = o.origin[0], a.oy = o.origin[1], a.oz = o.origin[2];
  a.words = (unsigned long long *)ws;
  a.key_by_row = (unsigned long long *)(ws + words_b);
  a.key_sorted = batched ? nullptr : key_sorted;
  a.rows = row_final;
  a.labels = label_sorted;
  a.head = (int32_t *)column(2), a.number = (int32_t *)column(3), a.start = (int32_t *)column(4), a.list = (int32_t *)column(5);
  a.lane_rows = lane_rows, a.block_rows = block_rows;
  a.capacity = o.capacity;

  unsigned long long *h = h_counters_;
  OWLMI_HIP(hipEventRecord(ev_a_, s));
  OWLMI_HIP(hipMemsetAsync(a.words, 0, kVoxWords * sizeof(unsigned long long), s));
  if (n > 0) {
    hipLaunchKernelGGL(vox_key_kernel, dim3(vox_blocks(n)), dim3(kVoxBlock), 0, s, a, row_in, label_by_row);
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipEventRecord(ev_b_, s));
  if (n > 0) {
    OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, (const unsigned long long *)a.key_by_row, key_sorted, (const uint32_t *)row_in, row_sorted, (int)n, 0, 64, s));
    if (batched) {
      hipLaunchKernelGGL(vox_gather_label_kernel, dim3(vox_blocks(n)), dim3(kVoxBlock), 0, s, (const uint32_t *)label_by_row, (const uint32_t *)row_sorted, n, label_in);
      OWLMI_HIP(hipGetLastError());
      OWLMI_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, sort_bytes, (const uint32_t *)label_in, label_sorted, (const uint32_t *)row_sorted, row_final, (int)n, 0, label_bits, s));
    }
    hipLaunchKernelGGL(vox_head_kernel, dim3(vox_blocks(n)), dim3(kVoxBlock), 0, s, a);
    OWLMI_HIP(hipGetLastError());
    OWLMI_HIP(hipcub::DeviceScan::InclusiveSum(tmp, scan_bytes, (const int32_t *)a.head, a.number, (int)n, s));
  }
  OWLMI_HIP(hipEventRecord(ev_c_, s));
  // the one read before anything the caller can see is written: V against the capacity (V <= n: no read where n fits)
  if (fill && n > 0 && o.capacity < (int64_t)n) {
    OWLMI_HIP(hipMemcpyAsync(h, a.number + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
    OWLMI_HIP(hipStreamSynchronize(s));
    const int64_t V = (int64_t)*(const int32_t *)h;
    if (V > o.capacity) throw ArgError{TKNN_E_ARG, "tknnVoxelGrid: " + std::to_string(V) + " voxels, capacity " + std::to_string(o.capacity) + " (nothing was written)"};
  }
  a.map = o.d_map, a.offsets = o.d_offsets;
  if (fill) {
    a.cell = o.d_cell, a.count = o.d_count, a.first = o.d_first, a.nearest = o.d_nearest, a.voxel_label = o.d_voxel_label;
    a.centroid = o.d_centroid, a.value_mean = o.d_value_mean;
  }
  if (n > 0) {
    hipLaunchKernelGGL(vox_map_kernel, dim3(vox_blocks(n)), dim3(kVoxBlock), 0, s, a);
    // (a voxel has at least a row: n lanes serve every voxel.  The count pass takes the fullest voxel from here too.)
    hipLaunchKernelGGL(vox_lane_kernel, dim3(vox_blocks(n)), dim3(kVoxBlock), 0, s, a);
    if (a.centroid || a.nearest || a.value_mean) {
      hipLaunchKernelGGL(vox_team_kernel<64>, dim3((unsigned)(cu_count_ * kVoxWaveBlocksPerCu)), dim3(kVoxBlock), 0, s, a, (const int32_t *)a.list, 1, (int)kVoxListed);
      hipLaunchKernelGGL(vox_team_kernel<kVoxTeam>, dim3((unsigned)cu_count_), dim3(kVoxTeam), 0, s, a, (const int32_t *)(a.list + (n - 1)), -1, (int)kVoxListedBlock);
    }
    OWLMI_HIP(hipGetLastError());
  }
  if (o.d_offsets) {
    hipLaunchKernelGGL(vox_offsets_kernel, dim3(vox_blocks((int64_t)B + 1)), dim3(kVoxBlock), 0, s, a);
    OWLMI_HIP(hipGetLastError());
  }
  if (fill && o.capacity > 0) {
    hipLaunchKernelGGL(vox_tail_kernel, dim3(vox_blocks(o.capacity)), dim3(kVoxBlock), 0, s, a);
    OWLMI_HIP(hipGetLastError());
  }
  OWLMI_HIP(hipEventRecord(ev_d_, s));
  OWLMI_HIP(hipMemcpyAsync(h, a.words, kVoxWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  if (n > 0) OWLMI_HIP(hipMemcpyAsync(h + kVoxWords, a.number + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, s));
  OWLMI_HIP(hipStreamSynchronize(s));
  std::memset(info, 0, sizeof *info);
  info->voxels = n > 0 ? (int64_t)*(const int32_t *)(h + kVoxWords) : 0;
  info->bad_rows = (int64_t)h[kVoxBadRows];
  info->bad_labels = (int64_t)h[kVoxBadLabels];
  info->out_of_grid = (int64_t)h[kVoxOutOfGrid];
  info->rows_in_grid = (int64_t)n - info->bad_rows - info->bad_labels - info->out_of_grid;
  info->max_count = (int32_t)h[kVoxMaxCount];
  info->wave_voxels = (int64_t)h[kVoxListed];
  info->block_voxels = (int64_t)h[kVoxListedBlock];
  OWLMI_HIP(hipEventElapsedTime(&info->key_ms, ev_a_, ev_b_));
  OWLMI_HIP(hipEventElapsedTime(&info->sort_ms, ev_b_, ev_c_));
  OWLMI_HIP(hipEventElapsedTime(&info->reduce_ms, ev_c_, ev_d_));
  OWLMI_HIP(hipEventElapsedTime(&info->solve_ms, ev_a_, ev_d_));
}

}  // namespace owlmi
