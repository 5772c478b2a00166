// plane_solve.h -- the host arithmetic of tknnSegmentPlane (include/owlknn_plane.h): the refit's plane from the fp64 moments of the
// inliers, the output plane and its sign.  Plain C++ in double, no fma, no device code: plane.hip includes it, and a stand-alone
// program can run it under a sanitizer.
#pragma once
#include <cmath>

namespace owlmi {

// the moments of a set of points relative to a centre: count, sum d^2, S1 (3), S2 (xx, xy, xz, yy, yz, zz)
enum { kPlCount = 0, kPlSumD2 = 1, kPlS1 = 2, kPlS2 = 5, kPlMoments = 11 };

// cyclic Jacobi, exactly as include/owlknn_plane.h states it: a (symmetric, row-major 3 x 3) is diagonalised in place, v takes the
// eigenvectors as columns
inline void plane_jacobi(double a[3][3], double v[3][3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
  static const int pairs[3][3] = {{0, 1, 2}, {0, 2, 1}, {1, 2, 0}};  // p, q, and the third index r
  for (int sweep = 0; sweep < 12; sweep++)
    for (int k = 0; k < 3; k++) {
      const int p = pairs[k][0], q = pairs[k][1], r = pairs[k][2];
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
      const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
      a[p][p] = a[p][p] - t * apq;
      a[q][q] = a[q][q] + t * apq;
      a[p][q] = a[q][p] = 0.0;
      const double arp = a[r][p], arq = a[r][q];
      a[r][p] = a[p][r] = c * arp - s * arq;
      a[r][q] = a[q][r] = s * arp + c * arq;
      for (int i = 0; i < 3; i++) {
        const double vip = v[i][p], viq = v[i][q];
        v[i][p] = c * vip - s * viq;
        v[i][q] = s * vip + c * viq;
      }
    }
}

// The refit: normal and anchor (fp32) from the moments `mom` about `centre`; false where the refit stops (no inlier, an entry that
// is not finite, or the two smallest eigenvalues equal up to 2^-40 of the largest).
inline bool plane_refit(const double *mom, const double *centre, float *normal, float *anchor) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double m = mom[kPlCount];
  if (!(m >= 1.0)) return false;
  const double mean[3] = {mom[kPlS1] / m, mom[kPlS1 + 1] / m, mom[kPlS1 + 2] / m};
  double a[3][3], v[3][3];
  a[0][0] = mom[kPlS2 + 0] / m - mean[0] * mean[0];
  a[0][1] = a[1][0] = mom[kPlS2 + 1] / m - mean[0] * mean[1];
  a[0][2] = a[2][0] = mom[kPlS2 + 2] / m - mean[0] * mean[2];
  a[1][1] = mom[kPlS2 + 3] / m - mean[1] * mean[1];
  a[1][2] = a[2][1] = mom[kPlS2 + 4] / m - mean[1] * mean[2];
  a[2][2] = mom[kPlS2 + 5] / m - mean[2] * mean[2];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++)
      if (!std::isfinite(a[i][j])) return false;
  plane_jacobi(a, v);
  int order[3] = {0, 1, 2};  // by eigenvalue, ties to the smaller column
  for (int i = 0; i < 3; i++)
    for (int j = i + 1; j < 3; j++)
      if (a[order[j]][order[j]] < a[order[i]][order[i]]) {
        const int tmp = order[i];
        order[i] = order[j], order[j] = tmp;
      }
  const double l0 = a[order[0]][order[0]], l1 = a[order[1]][order[1]], l2 = a[order[2]][order[2]];
  if (!std::isfinite(l0) || !std::isfinite(l1) || !std::isfinite(l2)) return false;
  if (!(l1 - l0 > 0x1p-40 * l2)) return false;
  const double x = v[0][order[0]], y = v[1][order[0]], z = v[2][order[0]];
  const double len = std::sqrt((x * x + y * y) + z * z);
  if (!(len > 0.0) || !std::isfinite(len)) return false;
  normal[0] = (float)(x / len), normal[1] = (float)(y / len), normal[2] = (float)(z / len);
  for (int i = 0; i < 3; i++) anchor[i] = (float)(mean[i] + centre[i]);
  return std::isfinite(anchor[0]) && std::isfinite(anchor[1]) && std::isfinite(anchor[2]);
}

// the axis as the trials take it: normalised in double, rounded to fp32; false for an all-zero axis (no constraint)
inline bool plane_axis(const float *axis, float *unit) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double x = axis[0], y = axis[1], z = axis[2];
  unit[0] = unit[1] = unit[2] = 0.f;
  if (x == 0.0 && y == 0.0 && z == 0.0) return false;
  const double len = std::sqrt((x * x + y * y) + z * z);
  unit[0] = (float)(x / len), unit[1] = (float)(y / len), unit[2] = (float)(z / len);
  return true;
}

// The output plane (a, b, c, d) of the fp32 normal and anchor, and the sign it was given: towards `unit` where has_axis and the
// dot is not zero, else the first nonzero of the normal positive.
inline double plane_output(const float *normal, const float *anchor, bool has_axis, const float *unit, double *plane) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double sign = 0.0;
  if (has_axis) {
    const double dot = ((double)normal[0] * (double)unit[0] + (double)normal[1] * (double)unit[1]) + (double)normal[2] * (double)unit[2];
    sign = dot > 0.0 ? 1.0 : (dot < 0.0 ? -1.0 : 0.0);
  }
  for (int i = 0; i < 3 && sign == 0.0; i++) sign = normal[i] > 0.f ? 1.0 : (normal[i] < 0.f ? -1.0 : 0.0);
  if (sign == 0.0) sign = 1.0;
  for (int i = 0; i < 3; i++) plane[i] = sign * (double)normal[i];
  plane[3] = -((plane[0] * (double)anchor[0] + plane[1] * (double)anchor[1]) + plane[2] * (double)anchor[2]);
  return sign;
}

}  // namespace owlmi
