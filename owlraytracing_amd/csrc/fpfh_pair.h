// fpfh_pair.h -- the one function tknnFpfh (include/owlknn_fpfh.h, fpfh.hip) bins: the three Darboux-frame features of a (point,
// neighbour) pair from their two normals, and the histogram bin of each.  Plain C++ for host and device
// (tests/fpfh_pair_host.py compiles it for the host).
//
// Every operation is fp32 and rounded on its own (the device build and the host test compile with -ffp-contract=off); a dot
// product is (x*x' + y*y') + z*z'.  The steps and their numbers are the header's.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FPFH_FN __host__ __device__ inline
#else
#define FPFH_FN inline
#endif

constexpr int kFpfhBinsPerFeature = 11;
constexpr int kFpfhBins = 3 * kFpfhBinsPerFeature;

struct FpfhFeatures {
  float f1, f2, f3;  // the angle about v in [-pi, pi], and two cosines in [-1, 1] (for unit normals)
  int b1, b2, b3;    // their bins, 0 .. 10 each
};

FPFH_FN float fpfh_dot(float ax, float ay, float az, float bx, float by, float bz) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return ((ax * bx) + (ay * by)) + (az * bz);
}

// (a NaN fails the compare)
FPFH_FN bool fpfh_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }

// floor(t) clamped to 0 .. 10, t finite
FPFH_FN int fpfh_bin(float t) {
  const float f = floorf(t);
  return f < 0.f ? 0 : (f > 10.f ? 10 : (int)f);
}

// The pair of a source with normal ni and a neighbour with normal nj at the offset dp = p_j - p_i, d2 the squared length of dp as
// the walk computed it and f4 its correctly rounded root.  False: the pair is degenerate and enters no histogram.
FPFH_FN bool fpfh_pair(float nix, float niy, float niz, float njx, float njy, float njz, float dx, float dy, float dz, float d2, float f4, FpfhFeatures &out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!(d2 > 0.f)) return false;
  if (!(fpfh_finite(nix) & fpfh_finite(niy) & fpfh_finite(niz) & fpfh_finite(njx) & fpfh_finite(njy) & fpfh_finite(njz))) return false;
  const float a1 = fpfh_dot(nix, niy, niz, dx, dy, dz) / f4, a2 = fpfh_dot(njx, njy, njz, dx, dy, dz) / f4;
  const bool swap = fabsf(a1) < fabsf(a2);
  const float n1x = swap ? njx : nix, n1y = swap ? njy : niy, n1z = swap ? njz : niz;
  const float n2x = swap ? nix : njx, n2y = swap ? niy : njy, n2z = swap ? niz : njz;
  const float px = swap ? -dx : dx, py = swap ? -dy : dy, pz = swap ? -dz : dz;
  const float f3 = swap ? -a2 : a1;
  // v = dp x n1, normalised
  float vx = py * n1z - pz * n1y, vy = pz * n1x - px * n1z, vz = px * n1y - py * n1x;
  const float vn = sqrtf(fpfh_dot(vx, vy, vz, vx, vy, vz));
  if (!(vn > 0.f)) return false;  // (vn == 0, or a NaN)
  vx = vx / vn, vy = vy / vn, vz = vz / vn;
  // w = n1 x v
  const float wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
  const float f2 = fpfh_dot(vx, vy, vz, n2x, n2y, n2z);
  const float f1 = atan2f(fpfh_dot(wx, wy, wz, n2x, n2y, n2z), fpfh_dot(n1x, n1y, n1z, n2x, n2y, n2z));
  if (!(fpfh_finite(f1) & fpfh_finite(f2) & fpfh_finite(f3))) return false;
  out.f1 = f1, out.f2 = f2, out.f3 = f3;
  out.b1 = fpfh_bin((11.f * (f1 + 3.14159274101257324f)) / 6.28318548202514648f);
  out.b2 = fpfh_bin((11.f * (f2 + 1.f)) * 0.5f);
  out.b3 = fpfh_bin((11.f * (f3 + 1.f)) * 0.5f);
  return true;
}
