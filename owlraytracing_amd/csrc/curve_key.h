// curve_key.h -- the sort keys of the LBVH: a space-filling-curve index of a cubic cell, plain integer code
// for host and device (tests/test_curve_key.py compiles it for the host).
//
// Both keys are HIERARCHICAL: with L levels, the top 3 m bits of the key of cell (x, y, z) are the m-level key
// of the cell's level-m parent (x >> (L - m), ...).  That is all the Karras radix tree needs (a common key
// prefix = a common octree cell), and what makes a 10-level key of a query sort like the tree's 21-level one.
//
//   curve_morton3:  bit interleave (Z curve), x the most significant axis.
//   curve_hilbert3: the Hilbert index, by Skilling's transpose ("Programming the Hilbert curve", AIP Conf. Proc.
//                   707, 2004): consecutive keys are face-adjacent cells, so a run of consecutive sorted points
//                   never straddles a jump of the curve and its bounding box stays near the smallest possible.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CURVE_KEY_FN __host__ __device__ inline
#else
#define CURVE_KEY_FN inline
#endif

enum { CURVE_HILBERT = 0, CURVE_MORTON = 1 };

// every third bit of a 21-bit value: bit i -> bit 3 i
CURVE_KEY_FN uint64_t curve_spread21(uint64_t v) {
  v &= 0x1fffffull;
  v = (v | v << 32) & 0x1f00000000ffffull;
  v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full;
  v = (v | v << 4) & 0x10c30c30c30c30c3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}

// cells of `levels` bits per axis (1 <= levels <= 21); the key has 3 * levels bits
CURVE_KEY_FN uint64_t curve_morton3(uint32_t x, uint32_t y, uint32_t z, int levels) {
  (void)levels;
  return (curve_spread21(x) << 2) | (curve_spread21(y) << 1) | curve_spread21(z);
}

CURVE_KEY_FN uint64_t curve_hilbert3(uint32_t x, uint32_t y, uint32_t z, int levels) {
  uint32_t X[3] = {x, y, z};
  const uint32_t top = 1u << (levels - 1);
  // undo the rotations and reflections of every level, the coarsest first: level Q only changes bits below Q
  for (uint32_t Q = top; Q > 1u; Q >>= 1) {
    const uint32_t P = Q - 1u;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      if (X[a] & Q) {
        X[0] ^= P;
      } else {
        const uint32_t t = (X[0] ^ X[a]) & P;
        X[0] ^= t;
        X[a] ^= t;
      }
    }
  }
  // Gray encode
  X[1] ^= X[0];
  X[2] ^= X[1];
  uint32_t t = 0;
  for (uint32_t Q = top; Q > 1u; Q >>= 1)
    if (X[2] & Q) t ^= Q - 1u;
  return (curve_spread21(X[0] ^ t) << 2) | (curve_spread21(X[1] ^ t) << 1) | curve_spread21(X[2] ^ t);
}

CURVE_KEY_FN uint64_t curve_key3(int curve, uint32_t x, uint32_t y, uint32_t z, int levels) {
  return curve == CURVE_MORTON ? curve_morton3(x, y, z, levels) : curve_hilbert3(x, y, z, levels);
}

// The key of a point: cubic cells over the scene box [lo, lo + ext]^3 (ext = the largest extent, one scale for all
// axes; a degenerate scene maps to cell 0), coordinates outside clamped to the faces.  A point with any NaN
// coordinate gets the one key above all others (bit 3 * levels; bit 63 of the tree's 21-level key).
CURVE_KEY_FN uint64_t curve_point_key(int curve, float cx, float cy, float cz, float lox, float loy, float loz, float ext, int levels) {
  const float cells = (float)((1u << levels) - 1u);
  const float scale = (ext > 0.f && ext < INFINITY) ? cells / ext : 0.f;
  const float c[3] = {cx, cy, cz}, lo[3] = {lox, loy, loz};
  uint32_t q[3];
  for (int a = 0; a < 3; a++) {
    float t = (c[a] - lo[a]) * scale;
    t = fminf(fmaxf(t, 0.f), cells);  // NaN -> 0 via fmaxf
    q[a] = (uint32_t)t;
  }
  if (cx != cx || cy != cy || cz != cz) return 1ull << (3 * levels);
  return curve_key3(curve, q[0], q[1], q[2], levels);
}
