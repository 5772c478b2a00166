// icp_solve.h -- the host half of tknnIcp (include/owlknn_icp.h): one step's rigid transform from the moments the device summed, and
// the update of T.  Plain C++ with no HIP in it but ICP_HD: icp.hip and ransac.hip include it, and tests/icp_solve_host.py compiles it with the host compiler.
//
// A moment row is kIcpMoments doubles, the coordinates taken relative to a centre c (the centre of the target's scene box):
//   [0] N, the pairs          [1] sum of d^2          [2] pairs left out of the system (normal not finite)
//   [3] pairs of the system with w > 0
//   point-to-point, a = s' - c, b = p - c:  [4] W = sum w   [5..7] sum w a   [8..10] sum w b   [11..19] sum w a_i b_j, row-major
//   point-to-plane, J = [a x n, n], r = (a - b) . n:  [4..24] the upper triangle of sum w J^T J, row by row   [25..30] sum w J^T r
#pragma once
#include <cmath>

// tknnRansac solves a trial's sample on the device with the same code: the functions are host and device under hipcc
#if defined(__HIPCC__)
#define ICP_HD __host__ __device__
#else
#define ICP_HD
#endif

namespace owlmi {

constexpr int kIcpMoments = 32;
enum { kIcpPairs = 0, kIcpSumD2 = 1, kIcpSkipped = 2, kIcpPositive = 3, kIcpSystem = 4, kIcpPlaneRhs = 25 };
constexpr int kIcpPointWords = 20, kIcpPlaneWords = 31;  // the words of a row each method uses

ICP_HD inline void icp_identity(double *T) {
  for (int i = 0; i < 16; i++) T[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

// C = A B, 4 x 4 row-major (C may be neither A nor B)
ICP_HD inline void icp_mul(const double *A, const double *B, double *C) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = 0;
      for (int t = 0; t < 4; t++) s += A[4 * i + t] * B[4 * t + j];
      C[4 * i + j] = s;
    }
}

// the top three rows of T as the device applies them
ICP_HD inline void icp_round_rows(const double *T, float *Tf) {
  for (int i = 0; i < 12; i++) Tf[i] = (float)T[i];
}

ICP_HD inline void icp_rigid(const double R[3][3], const double t[3], double *dT) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) dT[4 * i + j] = R[i][j];
    dT[4 * i + 3] = t[i];
  }
  dT[12] = dT[13] = dT[14] = 0.0;
  dT[15] = 1.0;
}

// Cyclic Jacobi on a symmetric 4 x 4: A becomes diagonal, the columns of V its eigenvectors.
ICP_HD inline void icp_jacobi4(double A[4][4], double V[4][4]) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; sweep++) {
    double off = 0;
    for (int p = 0; p < 4; p++)
      for (int q = p + 1; q < 4; q++) off += A[p][q] * A[p][q];
    if (!(off > 0)) break;  // (also: a NaN)
    for (int p = 0; p < 4; p++)
      for (int q = p + 1; q < 4; q++) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; k++) {  // A <- A G
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; k++) {  // A <- G^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = A[q][p] = 0.0;
        for (int k = 0; k < 4; k++) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

// Point-to-point.  The rotation that maximises sum w (p - mu_p) . R (s' - mu_s) is the unit quaternion of the largest eigenvalue
// of Horn's 4 x 4 matrix of H; it is V diag(1, 1, det(V U^T)) U^T of H = U S V^T, a proper rotation by construction.  The
// eigenvalues are s1 + s2 + s3', s1 - s2 - s3', -s1 + s2 - s3', -s1 - s2 + s3' (s3' = +-s3, the sign of det H), so the singular
// values the degeneracy rule needs are sums of two of them.  false: degenerate, dT untouched.
ICP_HD inline bool icp_solve_point(const double *mom, const double *c, double *dT) {
  const double W = mom[kIcpSystem];
  if (!(mom[kIcpPositive] >= 3.0) || !(W > 0.0)) return false;
  for (int i = kIcpSystem; i < kIcpPointWords; i++)
    if (!std::isfinite(mom[i])) return false;
  const double *Sa = mom + 5, *Sb = mom + 8, *Sab = mom + 11;
  double H[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) H[i][j] = Sab[3 * i + j] - Sa[i] * Sb[j] / W;
  double N[4][4] = {{H[0][0] + H[1][1] + H[2][2], H[1][2] - H[2][1], H[2][0] - H[0][2], H[0][1] - H[1][0]},
                    {0, H[0][0] - H[1][1] - H[2][2], H[0][1] + H[1][0], H[2][0] + H[0][2]},
                    {0, 0, -H[0][0] + H[1][1] - H[2][2], H[1][2] + H[2][1]},
                    {0, 0, 0, -H[0][0] - H[1][1] + H[2][2]}};
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < i; j++) N[i][j] = N[j][i];
  double V[4][4];
  icp_jacobi4(N, V);
  int idx[4] = {0, 1, 2, 3};
  for (int i = 0; i < 4; i++)
    for (int j = i + 1; j < 4; j++)
      if (N[idx[j]][idx[j]] > N[idx[i]][idx[i]]) {
        const int t = idx[i];
        idx[i] = idx[j];
        idx[j] = t;
      }
  const double l1 = N[idx[0]][idx[0]], l2 = N[idx[1]][idx[1]], l3 = N[idx[2]][idx[2]];
  const double s1 = 0.5 * (l1 + l2), s2 = 0.5 * (l1 + l3);
  if (!(s2 > std::ldexp(s1, -40)) || !std::isfinite(s1)) return false;
  double q0 = V[0][idx[0]], qx = V[1][idx[0]], qy = V[2][idx[0]], qz = V[3][idx[0]];
  const double qn = std::sqrt(q0 * q0 + qx * qx + qy * qy + qz * qz);
  q0 /= qn, qx /= qn, qy /= qn, qz /= qn;
  const double R[3][3] = {{q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)},
                          {2 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)},
                          {2 * (qz * qx - q0 * qy), 2 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz}};
  double mus[3], mup[3], t[3];
  for (int i = 0; i < 3; i++) mus[i] = c[i] + Sa[i] / W, mup[i] = c[i] + Sb[i] / W;
  for (int i = 0; i < 3; i++) t[i] = mup[i] - (R[i][0] * mus[0] + R[i][1] * mus[1] + R[i][2] * mus[2]);
  for (int i = 0; i < 3; i++)
    if (!std::isfinite(t[i])) return false;
  icp_rigid(R, t, dT);
  return true;
}

// Point-to-plane.  The system is the one the sums were taken for, J = [a x n, n] with a = s' - c: the step turns about c, so its
// condition does not depend on where the cloud sits; at the origin it is x -> dR (x - c) + c + t.  Cholesky in double; false: a
// pivot not above 2^-40 times its diagonal entry (0 up to the rounding of the sums), or not finite.
ICP_HD inline bool icp_solve_plane(const double *mom, const double *c, double *dT) {
  double Ao[6][6], b[6];
  int w = kIcpSystem;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) Ao[i][j] = Ao[j][i] = mom[w++];
  for (int i = 0; i < 6; i++) b[i] = -mom[kIcpPlaneRhs + i];
  double L[6][6] = {};
  for (int j = 0; j < 6; j++) {
    double d = Ao[j][j];
    for (int t = 0; t < j; t++) d -= L[j][t] * L[j][t];
    if (!(d > std::ldexp(Ao[j][j], -40)) || !std::isfinite(d)) return false;  // (<= 0 included: d <= Ao[j][j])
    L[j][j] = std::sqrt(d);
    for (int i = j + 1; i < 6; i++) {
      double s = Ao[i][j];
      for (int t = 0; t < j; t++) s -= L[i][t] * L[j][t];
      L[i][j] = s / L[j][j];
    }
  }
  double y[6], x[6];
  for (int i = 0; i < 6; i++) {
    double s = b[i];
    for (int t = 0; t < i; t++) s -= L[i][t] * y[t];
    y[i] = s / L[i][i];
  }
  for (int i = 5; i >= 0; i--) {
    double s = y[i];
    for (int t = i + 1; t < 6; t++) s -= L[t][i] * x[t];
    x[i] = s / L[i][i];
  }
  for (int i = 0; i < 6; i++)
    if (!std::isfinite(x[i])) return false;
  const double ca = std::cos(x[0]), sa = std::sin(x[0]), cb = std::cos(x[1]), sb = std::sin(x[1]), cg = std::cos(x[2]), sg = std::sin(x[2]);
  // Rz(gamma) Ry(beta) Rx(alpha)
  const double R[3][3] = {{cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa},
                          {sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa},
                          {-sb, cb * sa, cb * ca}};
  double t[3];
  for (int i = 0; i < 3; i++) t[i] = c[i] - (R[i][0] * c[0] + R[i][1] * c[1] + R[i][2] * c[2]) + x[3 + i];
  icp_rigid(R, t, dT);
  return true;
}

}  // namespace owlmi
