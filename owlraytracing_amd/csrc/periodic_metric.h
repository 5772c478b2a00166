// periodic_metric.h -- the two functions tknnPeriodicKnn (include/owlknn_periodic.h, periodic_knn.hip) rests on: the distance of
// two points in a cell that is periodic along some of its axes, and a lower bound of that distance from a query to every point
// of a box.  Plain C++ for host and device (tests/periodic_metric_host.py compiles it for the host).
//
// The cell: lo[3], period[3]; axis a is periodic iff period[a] > 0.  A value x is IN the cell on a periodic axis iff
// x >= lo[a] && fl(x - lo[a]) <= period[a] (periodic_in_cell).  Every operation below is fp32, rounded on its own.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PERIODIC_FN __host__ __device__ inline
#else
#define PERIODIC_FN inline
#endif

struct PeriodicCell {
  float lo[3];
  float period[3];
};

PERIODIC_FN bool periodic_in_cell(float x, float lo, float L) {
  return L > 0.f ? (x >= lo) & (x - lo <= L) : true;  // (a NaN x: not in the cell)
}

// One axis of the metric: a = |fl(p - q)|; open axis: a; periodic axis: min(a, |fl(L - a)|).  The smaller of the two is picked
// with a compare, not with fminf, which would drop a NaN: a NaN a stays a NaN.
PERIODIC_FN float periodic_axis(float p, float q, float L) {
  const float a = fabsf(p - q);
  const float b = fabsf(L - a);
  return L > 0.f ? (b < a ? b : a) : a;
}

// The squared distance: (wx*wx + wy*wy) + wz*wz, knn_dist2's association.  On open axes w*w is (p - q)*(p - q) bit for bit, so
// with no periodic axis this IS knn_dist2.
PERIODIC_FN float periodic_dist2(float px, float py, float pz, float qx, float qy, float qz, const PeriodicCell &c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float wx = periodic_axis(px, qx, c.period[0]), wy = periodic_axis(py, qy, c.period[1]), wz = periodic_axis(pz, qz, c.period[2]);
  return ((wx * wx) + (wy * wy)) + (wz * wz);
}

// The open-axis gap from x to [blo, bhi]: <= |fl(p - x)| for every blo <= p <= bhi (fp32 rounding is monotone).
PERIODIC_FN float periodic_gap(float blo, float bhi, float x) { return fmaxf(fmaxf(blo - x, x - bhi), 0.f); }

// One axis of the bound: a value that is <= periodic_axis(p, q, L) for EVERY in-cell p of [blo, bhi], q in the cell.
//
// In real numbers the wrapped distance is w = min(|p - q|, |L - |p - q||) = min(|p - q|, |p - (q + L)|, |p - (q - L)|) for any
// p, q and L > 0 (d = p - q >= 0: |L - d| = |p - (q + L)| and the third image is farther; d < 0 likewise), so its minimum over
// the box is g = min(gap(q), gap(q + L), gap(q - L)).  In fp32, with u = 2^-24 and p, q in the cell (|p - q| <= L (1 + u)):
//   * the metric: a' = |fl(p - q)| >= |p - q| (1 - u), b' = |fl(L - a')| >= (|L - |p - q|| - u |p - q|) (1 - u), so
//     w' >= (w - u |p - q|) (1 - u): an ABSOLUTE loss E1 <= u L (1 + u) -- the rounding of p - q, carried into L - a;
//   * the images: fl(q +- L) is off by at most E2 = u (|q| + L), about half an ulp of the cell's largest coordinate, and a gap
//     moves by as much as its image does; the gap's own subtraction is off by a factor (1 + u) at most.
// So w' >= g' (1 - 2 u) - (E1 + E2) with g' the computed minimum, and E1 + E2 <= u (|q| + 2 L).  The bound is g' - S with
// S = (|q| + 2 L) * 2^-22 = 4 (E1 + E2), clamped at 0.  That is absolute: next to a gap of a few ulps of the coordinate the
// relative 0.999995 of beyond_gate would not cover it.  It even makes the bound exact per axis: w' - (g' - S) >= 3 S / 4 -
// 2 u g', and a box with an in-cell point has g' <= L (the wrapped distance never exceeds L / 2 (1 + u)), so 2 u g' < 3 S / 4:
// bound <= w' as floats, and monotone rounding carries that through the squares and the sums below.  The direction: a larger S
// only lowers the bound, a lower bound only keeps a box the exact rule would decline -- the walk can only walk more.
PERIODIC_FN float periodic_axis_bound(float blo, float bhi, float q, float L) {
  const float g0 = periodic_gap(blo, bhi, q);
  if (!(L > 0.f)) return g0;
  const float g = fminf(g0, fminf(periodic_gap(blo, bhi, q + L), periodic_gap(blo, bhi, q - L)));
  const float slack = (fabsf(q) + 2.0f * L) * 2.384185791015625e-07f;  // 2^-22
  return fmaxf(g - slack, 0.f);
}

// A lower bound of periodic_dist2(p, q) over every in-cell point p of the box (Box: lo[3], hi[3]), for a query in the cell.
// With no periodic axis it is box_min_dist2 (team_walk.h) bit for bit.
template <class Box>
PERIODIC_FN float periodic_box_min_dist2(const Box &bx, float qx, float qy, float qz, const PeriodicCell &c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float gx = periodic_axis_bound(bx.lo[0], bx.hi[0], qx, c.period[0]), gy = periodic_axis_bound(bx.lo[1], bx.hi[1], qy, c.period[1]),
              gz = periodic_axis_bound(bx.lo[2], bx.hi[2], qz, c.period[2]);
  return ((gx * gx) + (gy * gy)) + (gz * gz);
}
